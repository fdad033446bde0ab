"""The fused training losses: RPN, Fast R-CNN, mask, RetinaNet and YOLOv4
(csrc/rpn_loss.hip, roi_losses.hip, retina_loss.hip, yolo_loss.hip), and the
cascade's gradient scaling."""
import torch

from ... import _C
from ._common import _f32c, _mask_u8
from .detect import _yolo_levels, yolo_host_arrays


class _ScaleGradFn(torch.autograd.Function):
    """Identity forward, gradient * scale backward (cascade_rcnn.py:35-39)."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None


def scale_gradient(x, scale):
    """x unchanged; the gradient reaching x is multiplied by scale."""
    return _ScaleGradFn.apply(x, float(scale))


class _RPNLossFn(torch.autograd.Function):
    """(loss_cls_sum, loss_loc_sum) * scale of the RPN (d2mi_rpn_loss_fwd /
    d2mi_rpn_loss_bwd_ex); differentiable w.r.t. logits and deltas.  The scale
    (the normaliser x loss weight) is applied to the two sums here and to the
    upstream gradients inside the backward kernel: no multiply launches."""

    @staticmethod
    def forward(ctx, logits, deltas, anchors, gt_boxes, matches, pos, sampled, weights, beta,
                scale=1.0):
        N, P = logits.shape
        G = gt_boxes.shape[1]
        nb = _C.lib().d2mi_rpn_loss_blocks()
        part = torch.empty((N * nb, 2), dtype=torch.float32, device=logits.device)
        w = _C.host_array(_C.c_float, [float(v) for v in weights])
        rc = _C.lib().d2mi_rpn_loss_fwd(_C.ptr(logits), _C.ptr(deltas), _C.ptr(anchors),
                                        _C.ptr(gt_boxes), _C.ptr(matches), _C.ptr(pos),
                                        _C.ptr(sampled), N, P, G, w, float(beta), _C.ptr(part),
                                        _C.stream_of(logits.device))
        _C.check(rc, "d2mi_rpn_loss_fwd")
        ctx.save_for_backward(logits, deltas, anchors, gt_boxes, matches, pos, sampled)
        ctx.conf = (tuple(float(v) for v in weights), float(beta), float(scale))
        ctx.set_materialize_grads(False)  # a missing gradient is a zero one (null pointer)
        # fixed-size reduction of the partials (deterministic order), scaled
        out = part.sum(0)
        if scale != 1.0:
            out.mul_(scale)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cls, g_loc):
        logits, deltas, anchors, gt_boxes, matches, pos, sampled = ctx.saved_tensors
        weights, beta, scale = ctx.conf
        N, P = logits.shape
        dev = logits.device
        g_cls = _f32c(g_cls) if g_cls is not None else None
        g_loc = _f32c(g_loc) if g_loc is not None else None
        d_logits = torch.empty_like(logits)
        d_deltas = torch.empty_like(deltas)
        w = _C.host_array(_C.c_float, list(weights))
        rc = _C.lib().d2mi_rpn_loss_bwd_ex(_C.ptr(logits), _C.ptr(deltas), _C.ptr(anchors),
                                           _C.ptr(gt_boxes), _C.ptr(matches), _C.ptr(pos),
                                           _C.ptr(sampled), N, P, gt_boxes.shape[1], w, beta,
                                           _C.ptr(g_cls), _C.ptr(g_loc), float(scale),
                                           _C.ptr(d_logits), _C.ptr(d_deltas), _C.stream_of(dev))
        _C.check(rc, "d2mi_rpn_loss_bwd_ex")
        return d_logits, d_deltas, None, None, None, None, None, None, None, None


class _FastRCNNLossFn(torch.autograd.Function):
    """(loss_cls, loss_box_reg) of FastRCNNOutputs.losses on dense rows
    (d2mi_fast_rcnn_loss_fwd / _bwd, csrc/roi_losses.hip); differentiable
    w.r.t. logits and deltas."""

    @staticmethod
    def forward(ctx, logits, deltas, proposals, gt_classes, gt_boxes, valid, weights, beta):
        B, K1 = logits.shape
        nreg = deltas.shape[1] // 4
        dev = logits.device
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        lib = _C.lib()
        wsb = lib.d2mi_fast_rcnn_loss_workspace_size(B)
        ws = _C.scratch(wsb, dev)
        w = _C.host_array(_C.c_float, [float(v) for v in weights])
        rc = lib.d2mi_fast_rcnn_loss_fwd(_C.ptr(logits), _C.ptr(deltas), _C.ptr(proposals),
                                         _C.ptr(gt_classes), _C.ptr(gt_boxes), _C.ptr(valid), B,
                                         K1, nreg, w, float(beta), _C.ptr(stats), _C.ptr(ws), wsb,
                                         _C.stream_of(dev))
        _C.check(rc, "d2mi_fast_rcnn_loss_fwd")
        ctx.save_for_backward(logits, deltas, proposals, gt_classes, gt_boxes, valid, stats)
        ctx.conf = (tuple(float(v) for v in weights), float(beta))
        ctx.set_materialize_grads(False)
        return stats[0], stats[1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        logits, deltas, proposals, gt_classes, gt_boxes, valid, stats = ctx.saved_tensors
        weights, beta = ctx.conf
        dev = logits.device
        z = torch.zeros((), dtype=torch.float32, device=dev)
        grads = torch.stack([g_cls if g_cls is not None else z,
                             g_box if g_box is not None else z]).float().contiguous()
        d_logits = torch.empty_like(logits)
        d_deltas = torch.empty_like(deltas)
        B, K1 = logits.shape
        w = _C.host_array(_C.c_float, list(weights))
        rc = _C.lib().d2mi_fast_rcnn_loss_bwd(_C.ptr(logits), _C.ptr(deltas), _C.ptr(proposals),
                                              _C.ptr(gt_classes), _C.ptr(gt_boxes), _C.ptr(valid),
                                              B, K1, deltas.shape[1] // 4, w, beta, _C.ptr(stats),
                                              _C.ptr(grads), _C.ptr(d_logits), _C.ptr(d_deltas),
                                              _C.stream_of(dev))
        _C.check(rc, "d2mi_fast_rcnn_loss_bwd")
        return d_logits, d_deltas, None, None, None, None, None, None


def fast_rcnn_loss(logits, deltas, proposals, gt_classes, gt_boxes, valid, weights, beta):
    """Fused Fast R-CNN losses on dense rows: logits [B, K+1], deltas
    [B, nreg*4], proposals / gt_boxes [B, 4], gt_classes [B], valid [B] ->
    (loss_cls, loss_box_reg), both already / max(1, #valid)."""
    logits, deltas = _f32c(logits), _f32c(deltas)
    proposals, gt_boxes = _f32c(proposals), _f32c(gt_boxes)
    gt_classes = gt_classes.to(torch.int64).contiguous()
    valid = valid.to(torch.uint8).contiguous()
    _C.require_device(logits, deltas, proposals, gt_classes, gt_boxes, valid)
    return _FastRCNNLossFn.apply(logits, deltas, proposals, gt_classes, gt_boxes, valid,
                                 tuple(weights), float(beta))


class _MaskLossFn(torch.autograd.Function):
    """mask_rcnn_loss's sigmoid BCE of the gt-class channel over foreground
    rows, mean over fg x Hm x Wm (d2mi_mask_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logits, target, classes, fg):
        B, Hm, Wm, C = logits.shape
        dev = logits.device
        stats = torch.empty(3, dtype=torch.float32, device=dev)
        lib = _C.lib()
        wsb = lib.d2mi_mask_loss_workspace_size(B)
        ws = _C.scratch(wsb, dev)
        rc = lib.d2mi_mask_loss_fwd(_C.ptr(logits), _C.ptr(target), _C.ptr(classes), _C.ptr(fg), B,
                                    Hm * Wm, C, _C.ptr(stats), _C.ptr(ws), wsb, _C.stream_of(dev))
        _C.check(rc, "d2mi_mask_loss_fwd")
        ctx.save_for_backward(logits, target, classes, fg, stats)
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, classes, fg, stats = ctx.saved_tensors
        B, Hm, Wm, C = logits.shape
        grads = g.reshape(1).float().contiguous()
        d_logits = torch.empty_like(logits)
        rc = _C.lib().d2mi_mask_loss_bwd(_C.ptr(logits), _C.ptr(target), _C.ptr(classes),
                                         _C.ptr(fg), B, Hm * Wm, C, _C.ptr(stats), _C.ptr(grads),
                                         _C.ptr(d_logits), _C.stream_of(logits.device))
        _C.check(rc, "d2mi_mask_loss_bwd")
        return d_logits, None, None, None


def mask_loss(logits, target, classes, fg):
    """Fused mask loss: logits [B, Hm, Wm, C], target [B, Hm, Wm] (0 / 1),
    classes [B], fg [B] -> mean sigmoid BCE of each fg row's class channel."""
    logits, target = _f32c(logits), _f32c(target)
    classes = classes.to(torch.int64).contiguous()
    fg = fg.to(torch.uint8).contiguous()
    _C.require_device(logits, target, classes, fg)
    return _MaskLossFn.apply(logits, target, classes, fg)


def rpn_loss(logits, deltas, anchors, gt_boxes, matches, pos, sampled, weights, beta,
             scale=1.0):
    """Fused RPN losses: logits [N, P], deltas [N, P, 4], anchors [P, 4],
    gt_boxes [N, G, 4], matches [N, P], pos / sampled [N, P] bool ->
    (loss_cls_sum * scale, loss_loc_sum * scale); scale = the caller's
    normaliser (1.0: the plain sums)."""
    logits, deltas = _f32c(logits), _f32c(deltas)
    anchors, gt_boxes = _f32c(anchors), _f32c(gt_boxes)
    matches = matches.to(torch.int64).contiguous()
    pos, sampled = _mask_u8(pos), _mask_u8(sampled)
    _C.require_device(logits, deltas, anchors, gt_boxes, matches, pos, sampled)
    return _RPNLossFn.apply(logits, deltas, anchors, gt_boxes, matches, pos, sampled,
                            tuple(weights), float(beta), float(scale))


class _RetinaLossFn(torch.autograd.Function):
    """(focal loss sum, smooth-L1 sum) of RetinaNet.losses over the head's
    per-level outputs (d2mi_retina_loss_fwd / _bwd, csrc/retina_loss.hip);
    differentiable w.r.t. every level's class logits and box deltas."""

    @staticmethod
    def forward(ctx, conf, anchors, gt_boxes, gt_classes, matches, labels, *levels):
        L = len(levels) // 2
        cls, box = levels[:L], levels[L:]
        N, K, A = cls[0].shape[0], conf[0], conf[1]
        lvl = [int(c.shape[1] * c.shape[2] * A) for c in cls]
        nb = _C.lib().d2mi_retina_loss_blocks()
        dev = anchors.device
        part = torch.empty((N * nb, 2), dtype=torch.float32, device=dev)
        la = _C.host_array(_C.ctypes.c_longlong, lvl)
        w = _C.host_array(_C.c_float, list(conf[5]))
        cp = _C.host_array(_C.c_void_p, [c.data_ptr() for c in cls])
        bp = _C.host_array(_C.c_void_p, [b.data_ptr() for b in box])
        rc = _C.lib().d2mi_retina_loss_fwd(cp, bp, la, L, N, K, A, _C.ptr(anchors),
                                           _C.ptr(gt_boxes), _C.ptr(gt_classes),
                                           gt_boxes.shape[1], _C.ptr(matches), _C.ptr(labels),
                                           conf[2], conf[3], conf[4], w, _C.ptr(part),
                                           _C.stream_of(dev))
        _C.check(rc, "d2mi_retina_loss_fwd")
        ctx.save_for_backward(anchors, gt_boxes, gt_classes, matches, labels, *levels)
        ctx.conf = (conf, lvl)
        ctx.set_materialize_grads(False)  # a missing gradient is a zero one (null pointer)
        out = part.sum(0)  # fixed-size reduction of the partials: deterministic order
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        anchors, gt_boxes, gt_classes, matches, labels, *levels = ctx.saved_tensors
        conf, lvl = ctx.conf
        L = len(levels) // 2
        cls, box = levels[:L], levels[L:]
        N, K, A = cls[0].shape[0], conf[0], conf[1]
        d = [torch.empty_like(t) for t in levels]
        g_cls = _f32c(g_cls) if g_cls is not None else None
        g_box = _f32c(g_box) if g_box is not None else None
        rc = _C.lib().d2mi_retina_loss_bwd(
            _C.host_array(_C.c_void_p, [c.data_ptr() for c in cls]),
            _C.host_array(_C.c_void_p, [b.data_ptr() for b in box]),
            _C.host_array(_C.c_void_p, [t.data_ptr() for t in d[:L]]),
            _C.host_array(_C.c_void_p, [t.data_ptr() for t in d[L:]]),
            _C.host_array(_C.ctypes.c_longlong, lvl), L, N, K, A, _C.ptr(anchors),
            _C.ptr(gt_boxes), _C.ptr(gt_classes), gt_boxes.shape[1], _C.ptr(matches),
            _C.ptr(labels), conf[2], conf[3], conf[4], _C.host_array(_C.c_float, list(conf[5])),
            _C.ptr(g_cls), _C.ptr(g_box), _C.stream_of(anchors.device))
        _C.check(rc, "d2mi_retina_loss_bwd")
        return (None,) * 6 + tuple(d)


def retina_loss(cls_levels, box_levels, anchors, gt_boxes, gt_classes, matches, labels,
                num_classes, num_anchors, alpha, gamma, beta, weights):
    """Fused RetinaNet losses (retinanet.py:147-210, before the normaliser):
    cls_levels [N, H, W, A*K] / box_levels [N, H, W, A*4] per level, anchors
    [R, 4] (levels concatenated, (h, w, a) order), gt_boxes [N, G, 4],
    gt_classes [N, G], matches / labels [N, R] (the Matcher's; labels 1 fg,
    0 bg, -1 ignore) -> (sum of sigmoid_focal_loss over every valid anchor and
    class, sum of smooth_l1 over the foreground anchors' deltas)."""
    cls_levels = [_f32c(c) for c in cls_levels]
    box_levels = [_f32c(b) for b in box_levels]
    anchors, gt_boxes = _f32c(anchors), _f32c(gt_boxes)
    gt_classes = gt_classes.to(torch.int64).contiguous()
    matches = matches.to(torch.int64).contiguous()
    labels = labels.to(torch.int64).contiguous()
    _C.require_device(anchors, gt_boxes, gt_classes, matches, labels, *cls_levels, *box_levels)
    for c, b in zip(cls_levels, box_levels):
        if c.shape[-1] != num_anchors * num_classes or b.shape[-1] != num_anchors * 4 \
                or c.shape[:3] != b.shape[:3]:
            raise ValueError(f"retina loss: level outputs {tuple(c.shape)} / {tuple(b.shape)} do "
                             f"not match A={num_anchors}, K={num_classes}")
    R = sum(int(c.shape[1] * c.shape[2]) * num_anchors for c in cls_levels)
    if anchors.shape[0] != R or labels.shape[-1] != R:
        raise ValueError(f"retina loss: {anchors.shape[0]} anchors / {labels.shape[-1]} labels "
                         f"for {R} head outputs")
    conf = (int(num_classes), int(num_anchors), float(alpha), float(gamma), float(beta),
            tuple(float(v) for v in weights))
    return _RetinaLossFn.apply(conf, anchors, gt_boxes, gt_classes, matches, labels,
                               *cls_levels, *box_levels)


class _YoloLossFn(torch.autograd.Function):
    """(conf, cls, box) losses of YOLOV4Outputs.losses over the head's
    per-level logits (d2mi_yolov4_loss_fwd / _bwd, csrc/yolo_loss.hip);
    differentiable w.r.t. every level's logits.  Also returns the counts of
    positives and negatives (no gradient)."""

    @staticmethod
    def forward(ctx, conf, gt_boxes, gt_classes, valid, slot, owner, state, *logits):
        geo, K, image_area, thr, cls_norm, iou_norm = conf
        lhw, st, chw, sc, L, A = geo
        N, G = valid.shape
        dev = logits[0].device
        lib = _C.lib()
        nb = lib.d2mi_yolov4_loss_blocks()
        part = torch.empty((N * nb, 5), dtype=torch.float64, device=dev)
        rc = lib.d2mi_yolov4_loss_fwd(
            _C.host_array(_C.c_void_p, [t.data_ptr() for t in logits]), lhw, st, chw, sc, L, A, K,
            N, _C.ptr(gt_boxes), _C.ptr(gt_classes), _C.ptr(valid), G, _C.ptr(slot),
            _C.ptr(owner), image_area, thr, iou_norm, _C.ptr(part), _C.ptr(state),
            _C.stream_of(dev))
        _C.check(rc, "d2mi_yolov4_loss_fwd")
        ctx.save_for_backward(gt_boxes, gt_classes, slot, owner, state, *logits)
        ctx.conf = conf
        ctx.set_materialize_grads(False)  # a missing gradient is a zero one (null pointer)
        # fixed-size reduction of the float64 partials (deterministic order)
        out = part.sum(0)
        # 1 / N and CLS_NORMALIZER / N (yolov4_outputs.py:288, :318); the box
        # weight carries IOU_NORMALIZER / N per element (:309)
        conf_loss = (out[0] * (1.0 / N)).float()
        cls_loss = (out[1] * (cls_norm / N)).float()
        npos, nneg = out[3].to(torch.int64), out[4].to(torch.int64)
        ctx.mark_non_differentiable(npos, nneg)
        return conf_loss, cls_loss, out[2].float(), npos, nneg

    @staticmethod
    def backward(ctx, g_conf, g_cls, g_box, _gp, _gn):
        gt_boxes, gt_classes, slot, owner, state, *logits = ctx.saved_tensors
        geo, K, image_area, thr, cls_norm, iou_norm = ctx.conf
        lhw, st, chw, sc, L, A = geo
        N, G = slot.shape
        dev = logits[0].device
        d = [torch.empty_like(t) for t in logits]
        g_conf = _f32c(g_conf) if g_conf is not None else None
        g_cls = _f32c(g_cls) if g_cls is not None else None
        g_box = _f32c(g_box) if g_box is not None else None
        rc = _C.lib().d2mi_yolov4_loss_bwd(
            _C.host_array(_C.c_void_p, [t.data_ptr() for t in logits]),
            _C.host_array(_C.c_void_p, [t.data_ptr() for t in d]), lhw, st, chw, sc, L, A, K, N,
            _C.ptr(gt_boxes), _C.ptr(gt_classes), G, _C.ptr(slot), _C.ptr(owner), _C.ptr(state),
            image_area, iou_norm, 1.0 / N, cls_norm / N, _C.ptr(g_conf), _C.ptr(g_cls),
            _C.ptr(g_box), _C.stream_of(dev))
        _C.check(rc, "d2mi_yolov4_loss_bwd")
        return (None,) * 7 + tuple(d)


def yolov4_loss(pred_logits, strides, cell_anchors, scale_yx, num_classes, gt_boxes, gt_classes,
                valid, image_hw, iou_threshold, cls_normalizer, iou_normalizer, debug=None):
    """Fused YOLOv4 targets and losses (yolov4_outputs.py:59-206, :266-329;
    d2mi_yolov4_assign + d2mi_yolov4_loss_fwd / _bwd): pred_logits[l]
    [N, H, W, A * (5 + K)], gt_boxes [N, G, 4], gt_classes [N, G], valid
    [N, G] = is_valid & ~crowd & ~difficult, image_hw the padded batch
    tensor's (H, W) -> (conf_loss, cls_loss, box_loss, num_pos, num_neg),
    device tensors, no host synchronisation.  ``debug``: a dict that receives
    slot [N, G] and owner [N, P] (int32) and state [N, P] (uint8: 0 neither,
    1 negative, 2 positive)."""
    hw = [(t.shape[1], t.shape[2]) for t in pred_logits]
    geo = yolo_host_arrays(hw, strides, cell_anchors, scale_yx)
    lhw, st, chw, sc, L, A = geo
    logits, N = _yolo_levels(pred_logits, num_classes, A)
    dev = logits[0].device
    gt_boxes = _f32c(gt_boxes)
    gt_classes = gt_classes.to(torch.int64).contiguous()
    valid = _mask_u8(valid)
    _C.require_device(gt_boxes, gt_classes, valid)
    G = valid.shape[1]
    if gt_boxes.shape != (N, G, 4) or gt_classes.shape != (N, G) or valid.shape[0] != N:
        raise ValueError(f"yolov4 loss: gt_boxes {tuple(gt_boxes.shape)} / gt_classes "
                         f"{tuple(gt_classes.shape)} / valid {tuple(valid.shape)} for N={N}")
    P = sum(h * w for h, w in hw) * A
    slot = torch.empty((N, G), dtype=torch.int32, device=dev)
    owner = torch.empty((N, P), dtype=torch.int32, device=dev)
    state = torch.empty((N, P), dtype=torch.uint8, device=dev)
    rc = _C.lib().d2mi_yolov4_assign(lhw, st, chw, L, A, N, _C.ptr(gt_boxes), _C.ptr(valid), G,
                                     _C.ptr(slot), _C.ptr(owner), _C.stream_of(dev))
    _C.check(rc, "d2mi_yolov4_assign")
    conf = (geo, int(num_classes), float(image_hw[0]) * float(image_hw[1]), float(iou_threshold),
            float(cls_normalizer), float(iou_normalizer))
    out = _YoloLossFn.apply(conf, gt_boxes, gt_classes, valid, slot, owner, state, *logits)
    if debug is not None:
        debug.update(slot=slot, owner=owner, state=state)
    return out
