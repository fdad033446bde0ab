"""Semantic segmentation and the panoptic merge (csrc/sem_seg.hip): the
fused loss, the resized argmax and combine_semantic_and_instance_outputs."""
import torch

from ... import _C
from ._common import _f32c, _i32c


def _sem_seg_args(logits, image_shapes, num_classes, scale):
    logits = _f32c(logits)
    image_shapes = _i32c(image_shapes)
    _C.require_device(logits, image_shapes)
    N, h, w, ldc = logits.shape
    C = ldc if num_classes is None else int(num_classes)
    if not 1 <= C <= ldc:
        raise ValueError(f"num_classes {C} does not fit the {ldc}-channel logit rows")
    if tuple(image_shapes.shape) != (N, 2):
        raise ValueError(f"image_shapes must be [{N}, 2], got {tuple(image_shapes.shape)}")
    return logits, image_shapes, (N, h, w, C, ldc), int(scale)


class _SemSegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, image_shapes, ignore_value, scale, loss_weight, num_classes):
        logits, image_shapes, dims, scale = _sem_seg_args(logits, image_shapes, num_classes, scale)
        labels = _i32c(labels)
        _C.require_device(labels)
        N = dims[0]
        if labels.dim() != 3 or labels.shape[0] != N:
            raise ValueError(f"labels must be [{N}, H, W], got {tuple(labels.shape)}")
        Hl, Wl = labels.shape[1:]
        dev = logits.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.int32, device=dev)
        lib = _C.lib()
        wsb = lib.d2mi_sem_seg_loss_workspace_size(N, dims[1], dims[2])
        ws = _C.scratch(wsb, dev)
        rc = lib.d2mi_sem_seg_loss_fwd(_C.ptr(logits), *dims, _C.ptr(labels), Hl, Wl,
                                       _C.ptr(image_shapes), int(ignore_value), scale,
                                       float(loss_weight), _C.ptr(loss), _C.ptr(count),
                                       _C.ptr(ws), wsb, _C.stream_of(dev))
        _C.check(rc, "d2mi_sem_seg_loss_fwd")
        ctx.save_for_backward(logits, labels, image_shapes, count)
        ctx.conf = (dims, Hl, Wl, int(ignore_value), scale, float(loss_weight))
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, image_shapes, count = ctx.saved_tensors
        dims, Hl, Wl, ignore_value, scale, loss_weight = ctx.conf
        g = _f32c(g)
        gl = torch.empty_like(logits)
        rc = _C.lib().d2mi_sem_seg_loss_bwd(_C.ptr(logits), *dims, _C.ptr(labels), Hl, Wl,
                                            _C.ptr(image_shapes), ignore_value, scale,
                                            loss_weight, _C.ptr(count), _C.ptr(g), _C.ptr(gl),
                                            _C.stream_of(logits.device))
        _C.check(rc, "d2mi_sem_seg_loss_bwd")
        return gl, None, None, None, None, None, None


def sem_seg_loss(logits, labels, image_shapes, ignore_value, scale, loss_weight,
                 num_classes=None):
    """SemSegFPNHead's loss (lib/modeling/meta_arch/semantic_seg.py:197-218)
    from the head's own low-resolution logits (d2mi_sem_seg_loss_fwd / _bwd):
    the x ``scale`` half-pixel bilinear resize and the mean softmax
    cross-entropy over the not-ignored pixels, times loss_weight, without the
    full-resolution logits or their gradient in memory.  logits [N, h, w, ldc]
    whose first ``num_classes`` channels are the classes (default: all);
    labels [N, Hl, Wl] integer on the [h*scale, w*scale] grid (pixels past
    Hl / Wl, past image_shapes [N, 2] or equal to ignore_value do not count).
    Returns the 0-d loss (0 when nothing counts); differentiable in logits
    (pad channels get a zero gradient).  No host sync, no allocation but the
    outputs: capture-safe."""
    return _SemSegLossFn.apply(logits, labels, image_shapes, int(ignore_value), int(scale),
                               float(loss_weight), num_classes)


def sem_seg_argmax(logits, image_shapes, scale, num_classes=None):
    """sem_seg_postprocess("conventional") + tf.argmax on the low-resolution
    logits (d2mi_sem_seg_argmax; lib/modeling/postprocessing.py:62-95,
    panoptic_fpn.py:118-131): [N, h*scale, w*scale] int64, the argmax of the
    x ``scale`` bilinear resize inside image_shapes[n], 0 outside."""
    logits, image_shapes, dims, scale = _sem_seg_args(logits, image_shapes, num_classes, scale)
    N, h, w = dims[:3]
    out = torch.empty((N, h * scale, w * scale), dtype=torch.int64, device=logits.device)
    rc = _C.lib().d2mi_sem_seg_argmax(_C.ptr(logits), *dims, _C.ptr(image_shapes), scale,
                                      _C.ptr(out), _C.stream_of(logits.device))
    _C.check(rc, "d2mi_sem_seg_argmax")
    return out


def panoptic_combine(masks, scores, classes, boxes, is_valid, sem_seg, overlap_thresh,
                     stuff_area_limit, conf_thresh, num_stuff_classes):
    """combine_semantic_and_instance_outputs (panoptic_fpn.py:160-296,
    d2mi_panoptic_combine) over a batch: masks [N, D, H, W] uint8 pasted
    masks, scores / classes / is_valid [N, D], boxes [N, D, 4], sem_seg
    [N, H, W] class map.  Returns the reference's dict: panoptic_seg
    [N, H, W] int32 and, per image, D + num_stuff_classes - 1 rows of id,
    isthing, score, category_id, instance_id, bbox, is_valid, area."""
    masks = masks.to(torch.uint8).contiguous()
    scores, boxes = _f32c(scores), _f32c(boxes)
    classes = classes.to(torch.int64).contiguous()
    is_valid = is_valid.to(torch.uint8).contiguous()
    sem_seg = sem_seg.to(torch.int64).contiguous()
    _C.require_device(masks, scores, classes, boxes, is_valid, sem_seg)
    N, D, H, W = masks.shape
    if tuple(sem_seg.shape) != (N, H, W):
        raise ValueError(f"sem_seg must be {(N, H, W)}, got {tuple(sem_seg.shape)}")
    if (tuple(scores.shape) != (N, D) or tuple(classes.shape) != (N, D)
            or tuple(is_valid.shape) != (N, D) or tuple(boxes.shape) != (N, D, 4)):
        raise ValueError("panoptic_combine: instance fields do not match the masks' [N, D]")
    S = int(num_stuff_classes)
    R = D + S - 1
    dev = masks.device

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    pan = new((N, H, W), torch.int32)
    out = {"id": new((N, R), torch.int32), "isthing": new((N, R), torch.uint8),
           "score": new((N, R), torch.float32), "category_id": new((N, R), torch.int64),
           "instance_id": new((N, R), torch.int32), "bbox": new((N, R, 4), torch.float32),
           "is_valid": new((N, R), torch.uint8), "area": new((N, R), torch.float32)}
    lib = _C.lib()
    wsb = lib.d2mi_panoptic_combine_workspace_size(N, D, S)
    ws = _C.scratch(wsb, dev)
    rc = lib.d2mi_panoptic_combine(
        _C.ptr(masks), _C.ptr(scores), _C.ptr(classes), _C.ptr(boxes), _C.ptr(is_valid),
        _C.ptr(sem_seg), N, D, H, W, float(overlap_thresh), float(stuff_area_limit),
        float(conf_thresh), S, _C.ptr(pan), _C.ptr(out["id"]), _C.ptr(out["isthing"]),
        _C.ptr(out["score"]), _C.ptr(out["category_id"]), _C.ptr(out["instance_id"]),
        _C.ptr(out["bbox"]), _C.ptr(out["is_valid"]), _C.ptr(out["area"]), _C.ptr(ws), wsb,
        _C.stream_of(dev))
    _C.check(rc, "d2mi_panoptic_combine")
    out["isthing"] = out["isthing"].bool()
    out["is_valid"] = out["is_valid"].bool()
    out["panoptic_seg"] = pan
    return out
