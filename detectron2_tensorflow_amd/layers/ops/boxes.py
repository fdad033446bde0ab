"""Box-level ops: NMS, top-k, the samplers, anchors and deltas, the matcher
and the cascade stage hand-over (csrc/nms.hip, topk.hip, sample.hip,
roi_sample.hip, match.hip, cascade.hip; grid_anchors / apply_deltas live in
proposals.hip)."""
import torch

from ... import _C
from ._common import _DEFAULT_SCALE_CLAMP, _f32c, _i32c, _mask_u8


# ----------------------------------------------------------------------- NMS
def nms_segments(boxes, scores, seg_offsets, max_output_size, iou_threshold, seg_capacity=None):
    """Segmented TF NonMaxSuppressionV3.  boxes [T,4], scores [T], seg_offsets
    int [S+1] (device).  Returns keep [S, max_out] int32 (segment-relative,
    -1 padded) and num_keep [S] int32."""
    if not 0.0 <= float(iou_threshold) <= 1.0:
        raise ValueError("iou_threshold must be in [0, 1], got %r" % (iou_threshold,))
    if max_output_size < 0:
        raise ValueError("max_output_size must be non-negative, got %r" % (max_output_size,))
    boxes, scores, seg_offsets = _f32c(boxes), _f32c(scores), _i32c(seg_offsets)
    _C.require_device(boxes, scores, seg_offsets)
    S = seg_offsets.shape[0] - 1
    if seg_capacity is None:
        seg_capacity = int(boxes.shape[0])
    dev = boxes.device
    keep = torch.empty((S, max(int(max_output_size), 1)), dtype=torch.int32, device=dev)
    num = torch.empty((S,), dtype=torch.int32, device=dev)
    wsb = _C.lib().d2mi_nms_workspace_size(S, int(seg_capacity))
    ws = _C.workspace(wsb, dev)
    rc = _C.lib().d2mi_nms(_C.ptr(boxes), _C.ptr(scores), _C.ptr(seg_offsets), S,
                           int(seg_capacity), int(max_output_size), float(iou_threshold),
                           _C.ptr(keep), _C.ptr(num), _C.ptr(ws), wsb, _C.stream_of(dev))
    _C.check(rc, "d2mi_nms")
    return keep[:, :max_output_size], num


def non_max_suppression(boxes, scores, max_output_size, iou_threshold=0.5):
    """tf.image.non_max_suppression: selected indices (int32, selection order)."""
    n = boxes.shape[0]
    off = torch.tensor([0, n], dtype=torch.int32, device=boxes.device)
    keep, num = nms_segments(boxes, scores, off, max_output_size, iou_threshold, seg_capacity=n)
    return keep[0, : int(num[0].item())]


# --------------------------------------------------------------------- top-k
TOPK_MAX_K = 8192  # d2mi_topk's largest k (kCap in csrc/topk.hip)


def topk_segments(values, seg_start, seg_len, k, max_seg_len, sigmoid=False):
    """Exact segmented top-k (tf.nn.top_k sorted=True order)."""
    values = _f32c(values)
    seg_start = seg_start.to(torch.int64).contiguous()
    seg_len = _i32c(seg_len)
    _C.require_device(values, seg_start, seg_len)
    S = seg_len.shape[0]
    dev = values.device
    vals = torch.empty((S, max(k, 1)), dtype=torch.float32, device=dev)
    idx = torch.empty((S, max(k, 1)), dtype=torch.int32, device=dev)
    cnt = torch.empty((S,), dtype=torch.int32, device=dev)
    wsb = _C.lib().d2mi_topk_workspace_size(S, k)
    ws = _C.workspace(wsb, dev)
    rc = _C.lib().d2mi_topk(_C.ptr(values), _C.ptr(seg_start), _C.ptr(seg_len), S,
                            int(max_seg_len), int(k), int(bool(sigmoid)), _C.ptr(vals),
                            _C.ptr(idx), _C.ptr(cnt), _C.ptr(ws), wsb, _C.stream_of(dev))
    _C.check(rc, "d2mi_topk")
    return vals[:, :k], idx[:, :k], cnt


def subsample(labels, num_samples, num_pos, bg_label, seed, order_slots=0):
    """d2mi_subsample: (pos, neg) [N, P] bool -- a uniformly random
    min(num_pos, #pos) positives and min(num_samples - that, #neg) negatives
    per row (labels int64: -1 ignore, bg_label negative, else positive);
    with order_slots = S also (order [N, S] int64, valid [N, S] bool): the
    selected indices positives first, each kind in index order.  seed: a
    device int64 tensor [1]."""
    if labels.dtype is not torch.int64 or not labels.is_contiguous():
        labels = labels.to(torch.int64).contiguous()
    _C.require_device(labels, seed)
    N, P = labels.shape
    dev = labels.device
    # bool outputs written directly (one byte, 0 / 1: the kernel's uint8)
    pos = torch.empty((N, P), dtype=torch.bool, device=dev)
    neg = torch.empty((N, P), dtype=torch.bool, device=dev)
    S = int(order_slots)
    order = torch.empty((N, S), dtype=torch.int64, device=dev) if S else None
    valid = torch.empty((N, S), dtype=torch.bool, device=dev) if S else None
    wsb = _C.lib().d2mi_subsample_workspace_size(N, P)
    ws = _C.workspace(wsb, dev)
    rc = _C.lib().d2mi_subsample(_C.ptr(labels), N, P, int(bg_label), int(num_samples),
                                 int(num_pos), _C.ptr(seed), _C.ptr(pos), _C.ptr(neg),
                                 _C.ptr(order), _C.ptr(valid), S, _C.ptr(ws), wsb,
                                 _C.stream_of(dev))
    _C.check(rc, "d2mi_subsample")
    if S:
        return pos, neg, order, valid
    return pos, neg


def roi_gt_classes(labels, matches, gt_classes, pvalid, num_classes):
    """d2mi_roi_gt_classes: the training class of every proposal, [N, M] int64
    (roi_heads.py:160-216): the matched GT class for label 1, num_classes
    (background) for 0, -1 for ignored rows and invalid proposal slots."""
    _C.require_device(labels, matches, gt_classes, pvalid)
    if labels.dtype is not torch.int64 or matches.dtype is not torch.int64:
        raise ValueError("roi_gt_classes: labels / matches must be int64")
    labels, matches = labels.contiguous(), matches.contiguous()
    if gt_classes.dtype not in (torch.int32, torch.int64):
        gt_classes = gt_classes.to(torch.int64)
    gt_classes = gt_classes.contiguous()
    pv = pvalid.to(torch.bool).contiguous()
    N, M = labels.shape
    G = gt_classes.shape[1]
    out = torch.empty((N, M), dtype=torch.int64, device=labels.device)
    rc = _C.lib().d2mi_roi_gt_classes(_C.ptr(labels), _C.ptr(matches), _C.ptr(gt_classes),
                                      int(gt_classes.dtype is torch.int64), _C.ptr(pv), N, M, G,
                                      int(num_classes), _C.ptr(out), _C.stream_of(labels.device))
    _C.check(rc, "d2mi_roi_gt_classes")
    return out


def roi_sample_take(order, valid, boxes, gt_classes, matches, gt_boxes, num_classes, mask_slots):
    """d2mi_roi_sample_take: the sampled dict of label_and_sample_proposals
    (boxes, gt_classes, gt_index, gt_boxes [N, S(, 4)]) and, mask_slots = F >
    0, the mask branch's inputs over the first F slots per image in stable
    foreground-first order: ((boxes, classes, fg, image, mask index, gt boxes),
    fg [N*F] in slot order, count [1] int64)."""
    _C.require_device(order, valid, boxes, gt_classes, matches, gt_boxes)
    order, valid = order.contiguous(), valid.to(torch.bool).contiguous()
    boxes, gt_boxes = _f32c(boxes), _f32c(gt_boxes)
    gt_classes, matches = gt_classes.contiguous(), matches.contiguous()
    N, S = order.shape
    M, G, F = boxes.shape[1], gt_boxes.shape[1], int(mask_slots)
    dev = order.device
    s_boxes = torch.empty((N, S, 4), dtype=torch.float32, device=dev)
    s_cls = torch.empty((N, S), dtype=torch.int64, device=dev)
    s_gidx = torch.empty((N, S), dtype=torch.int64, device=dev)
    s_gtb = torch.empty((N, S, 4), dtype=torch.float32, device=dev)
    R = N * F
    m = None
    if F:
        m = (torch.empty((R, 4), dtype=torch.float32, device=dev),
             torch.empty((R,), dtype=torch.int64, device=dev),
             torch.empty((R,), dtype=torch.bool, device=dev),
             torch.empty((R,), dtype=torch.int32, device=dev),
             torch.empty((R,), dtype=torch.int64, device=dev),
             torch.empty((R, 4), dtype=torch.float32, device=dev),
             torch.empty((R,), dtype=torch.bool, device=dev),
             torch.empty((1,), dtype=torch.int64, device=dev))
    mp = [_C.ptr(t) for t in m] if m else [None] * 8
    rc = _C.lib().d2mi_roi_sample_take(_C.ptr(order), _C.ptr(valid), _C.ptr(boxes),
                                       _C.ptr(gt_classes), _C.ptr(matches), _C.ptr(gt_boxes), N,
                                       M, S, G, F, int(num_classes), _C.ptr(s_boxes),
                                       _C.ptr(s_cls), _C.ptr(s_gidx), _C.ptr(s_gtb), *mp,
                                       _C.stream_of(dev))
    _C.check(rc, "d2mi_roi_sample_take")
    sampled = {"boxes": s_boxes, "gt_classes": s_cls, "gt_index": s_gidx, "gt_boxes": s_gtb,
               "is_valid": valid}
    return sampled, ((m[:6], m[6], m[7]) if m else None)


# ------------------------------------------------------------ anchors/deltas
def grid_anchors(H, W, stride, cell_anchors, device):
    """DefaultAnchorGenerator.grid_anchors for one level -> [H*W*A, 4]."""
    cell = [float(v) for v in torch.as_tensor(cell_anchors, dtype=torch.float32).reshape(-1)]
    A = len(cell) // 4
    out = torch.empty((H * W * A, 4), dtype=torch.float32, device=device)
    rc = _C.lib().d2mi_grid_anchors(int(H), int(W), float(stride),
                                    _C.host_array(_C.c_float, cell), A, _C.ptr(out),
                                    _C.stream_of(device))
    _C.check(rc, "d2mi_grid_anchors")
    return out


def apply_deltas(deltas, boxes, weights, scale_clamp=_DEFAULT_SCALE_CLAMP):
    """Box2BoxTransform.apply_deltas: deltas [N, K*4], boxes [N, 4]."""
    deltas, boxes = _f32c(deltas), _f32c(boxes)
    _C.require_device(deltas, boxes)
    N = boxes.shape[0]
    K = deltas.shape[1] // 4
    out = torch.empty_like(deltas)
    if N == 0:
        return out
    rc = _C.lib().d2mi_apply_deltas(_C.ptr(deltas), _C.ptr(boxes), N, K,
                                    _C.host_array(_C.c_float, [float(w) for w in weights]),
                                    float(scale_clamp), _C.ptr(out), _C.stream_of(boxes.device))
    _C.check(rc, "d2mi_apply_deltas")
    return out


def match_boxes(gt_boxes, gt_flags, boxes, thresholds, labels_of, allow_low_quality,
                crowd_thr=1e-3, difficult_thr=float("inf")):
    """Fused pairwise IoU + Matcher (d2mi_match_boxes): gt_boxes [N, G, 4],
    gt_flags [N, G] int (bit0 matchable, bit1 crowd, bit2 difficult), boxes
    [P, 4] (shared) or [N, P, 4]; thresholds with the -inf / +inf ends.
    Returns (matches int64 [N, P], labels int64 [N, P])."""
    gt_boxes = _f32c(gt_boxes)
    boxes = _f32c(boxes)
    gt_flags = _i32c(gt_flags)
    _C.require_device(gt_boxes, gt_flags, boxes)
    N, G = gt_flags.shape
    per_image = boxes.dim() == 3
    P = boxes.shape[-2]
    matches = torch.empty((N, P), dtype=torch.int64, device=boxes.device)
    labels = torch.empty((N, P), dtype=torch.int64, device=boxes.device)
    thr = _C.host_array(_C.c_float, [float(t) for t in thresholds])
    lab = _C.host_array(_C.ctypes.c_int32, [int(v) for v in labels_of])
    wsb = _C.lib().d2mi_match_workspace_size(N, G)
    ws = _C.workspace(wsb, boxes.device)
    rc = _C.lib().d2mi_match_boxes(_C.ptr(gt_boxes), _C.ptr(gt_flags), _C.ptr(boxes),
                                   int(per_image), N, G, P, thr, lab, len(labels_of),
                                   int(bool(allow_low_quality)), float(crowd_thr),
                                   float(difficult_thr), _C.ptr(matches), _C.ptr(labels),
                                   _C.ptr(ws), wsb, _C.stream_of(boxes.device))
    _C.check(rc, "d2mi_match_boxes")
    return matches, labels


def match_boxes_masks(gt_boxes, valid, boxes, thresholds, labels_of, allow_low_quality,
                      crowd=None, difficult=None, crowd_thr=1e-3, difficult_thr=float("inf")):
    """match_boxes with the GT flags as [N, G] masks (d2mi_match_boxes_ex):
    valid required, crowd / difficult optional -- the bool tensors are passed
    as they are, no int32 packing launches; the matchable GT are valid and
    neither crowd nor difficult."""
    gt_boxes = _f32c(gt_boxes)
    boxes = _f32c(boxes)
    m, c, d = _mask_u8(valid), _mask_u8(crowd), _mask_u8(difficult)
    _C.require_device(gt_boxes, m, boxes, *[t for t in (c, d) if t is not None])
    N, G = m.shape
    for t in (c, d):
        if t is not None and tuple(t.shape) != (N, G):
            raise ValueError("match_boxes_masks: crowd / difficult must be [N, G] like matchable")
    per_image = boxes.dim() == 3
    P = boxes.shape[-2]
    matches = torch.empty((N, P), dtype=torch.int64, device=boxes.device)
    labels = torch.empty((N, P), dtype=torch.int64, device=boxes.device)
    thr = _C.host_array(_C.c_float, [float(t) for t in thresholds])
    lab = _C.host_array(_C.ctypes.c_int32, [int(v) for v in labels_of])
    wsb = _C.lib().d2mi_match_workspace_size(N, G)
    ws = _C.workspace(wsb, boxes.device)
    rc = _C.lib().d2mi_match_boxes_ex(_C.ptr(gt_boxes), _C.ptr(m), _C.ptr(c), _C.ptr(d),
                                      _C.ptr(boxes), int(per_image), N, G, P, thr, lab,
                                      len(labels_of),
                                      int(bool(allow_low_quality)), float(crowd_thr),
                                      float(difficult_thr), _C.ptr(matches), _C.ptr(labels),
                                      _C.ptr(ws), wsb, _C.stream_of(boxes.device))
    _C.check(rc, "d2mi_match_boxes_ex")
    return matches, labels


def _cascade_refine_tensor(deltas, boxes, valid, image_hw, weights, scale_clamp, gt, iou_thr,
                           num_classes):
    """cascade_refine as tensor ops (any device): the float sequences of
    apply_delta / clip_box (csrc/common.h) and the matcher's tensor code."""
    N, S = valid.shape
    b = boxes.reshape(N * S, 4)
    d = deltas.reshape(N * S, 4)
    wy, wx, wh, ww = (float(w) for w in weights)
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cy, cx = b[:, 0] + 0.5 * h, b[:, 1] + 0.5 * w
    dh = (d[:, 2] / wh).clamp(max=scale_clamp)
    dw = (d[:, 3] / ww).clamp(max=scale_clamp)
    pcy, pcx = (d[:, 0] / wy) * h + cy, (d[:, 1] / wx) * w + cx
    ph, pw = torch.exp(dh) * h, torch.exp(dw) * w
    dec = torch.stack([pcy - 0.5 * ph, pcx - 0.5 * pw, pcy + 0.5 * ph, pcx + 0.5 * pw], dim=1)
    hw = image_hw.to(torch.float32)
    win = torch.stack([hw[:, 0], hw[:, 1], hw[:, 0], hw[:, 1]], dim=1)[:, None, :]  # [N, 1, 4]
    out = torch.minimum(dec.reshape(N, S, 4), win).clamp(min=0.0)
    if gt is None:
        return {"boxes": out, "is_valid": valid}
    from ...modeling.matcher import Matcher, match_boxes as match_tensor
    gt_boxes, gt_valid, gt_classes, crowd, difficult = gt
    area = (out[..., 2] - out[..., 0]) * (out[..., 3] - out[..., 1])
    ok = valid & (area > 0)
    matches, labels = match_tensor(Matcher([float(iou_thr)], [0, 1], False), gt_boxes, gt_valid,
                                   out, crowd=crowd, difficult=difficult)
    gcls = torch.gather(gt_classes.long(), 1, matches)
    cls = torch.where(labels == 1, gcls, torch.where(labels == 0, int(num_classes), -1))
    cls = torch.where(ok, cls, -1)
    return {"boxes": out, "is_valid": ok, "gt_classes": cls, "gt_index": matches,
            "gt_boxes": torch.gather(gt_boxes, 1, matches[..., None].expand(-1, -1, 4)),
            "loss_valid": ok & (cls >= 0)}


def cascade_refine(deltas, boxes, valid, image_hw, weights, scale_clamp=_DEFAULT_SCALE_CLAMP,
                   gt_boxes=None, gt_valid=None, gt_classes=None, gt_crowd=None,
                   gt_difficult=None, iou_thr=None, num_classes=None):
    """The stage hand-over of a cascade (cascade_rcnn.py:141-215, :244-273;
    d2mi_cascade_refine, one launch): the previous stage's class-agnostic
    deltas [N*S, 4] decoded on its boxes [N, S, 4] with its weights, clipped
    to the image.  Inference (gt_boxes None): {boxes, is_valid = valid}.
    Training: is_valid = valid & (area > 0), and the boxes re-matched against
    the ground truth at iou_thr (labels [0, 1], no low-quality matches,
    Matcher's crowd / difficult rules): gt_classes (class / num_classes / -1
    for ignored or invalid rows), gt_index (into the [G] list), gt_boxes,
    loss_valid = is_valid & (gt_classes >= 0).  Nothing is differentiable."""
    training = gt_boxes is not None
    if training and (gt_valid is None or gt_classes is None or iou_thr is None
                     or num_classes is None):
        raise ValueError("cascade_refine: training mode needs gt_valid, gt_classes, iou_thr and "
                         "num_classes")
    deltas, boxes = deltas.detach(), boxes.detach()
    N, S = valid.shape
    if tuple(boxes.shape) != (N, S, 4) or deltas.numel() != N * S * 4:
        raise ValueError("cascade_refine: boxes [N, S, 4], class-agnostic deltas [N*S, 4], "
                         "valid [N, S]")
    valid = valid.to(torch.bool)
    if not boxes.is_cuda:
        gt = ((gt_boxes.to(torch.float32), gt_valid.to(torch.bool), gt_classes,
               gt_crowd.to(torch.bool) if gt_crowd is not None else None,
               gt_difficult.to(torch.bool) if gt_difficult is not None else None)
              if training else None)
        return _cascade_refine_tensor(deltas.to(torch.float32), boxes.to(torch.float32), valid,
                                      image_hw, weights, scale_clamp, gt, iou_thr, num_classes)
    deltas, boxes, image_hw = _f32c(deltas), _f32c(boxes), _i32c(image_hw)
    v = _mask_u8(valid)
    _C.require_device(deltas, boxes, v, image_hw)
    dev = boxes.device
    ob = torch.empty((N, S, 4), dtype=torch.float32, device=dev)
    ov = torch.empty((N, S), dtype=torch.bool, device=dev)
    w4 = _C.host_array(_C.c_float, [float(w) for w in weights])
    nul = _C.c_void_p(None)
    if not training:
        rc = _C.lib().d2mi_cascade_refine(_C.ptr(deltas), _C.ptr(boxes), _C.ptr(v),
                                          _C.ptr(image_hw), N, S, w4, float(scale_clamp), 0, nul,
                                          nul, nul, nul, nul, 0, 0, 0.0, 0, _C.ptr(ob), _C.ptr(ov),
                                          nul, nul, nul, nul, _C.stream_of(dev))
        _C.check(rc, "d2mi_cascade_refine")
        return {"boxes": ob, "is_valid": ov}
    gt_boxes = _f32c(gt_boxes)
    m, c, d = _mask_u8(gt_valid), _mask_u8(gt_crowd), _mask_u8(gt_difficult)
    if gt_classes.dtype not in (torch.int32, torch.int64):
        gt_classes = gt_classes.to(torch.int64)
    gt_classes = gt_classes.contiguous()
    _C.require_device(gt_boxes, m, gt_classes, *[t for t in (c, d) if t is not None])
    G = m.shape[1]
    for t in (gt_classes, c, d):
        if t is not None and tuple(t.shape) != (N, G):
            raise ValueError("cascade_refine: gt_classes / crowd / difficult must be [N, G]")
    if tuple(gt_boxes.shape) != (N, G, 4):
        raise ValueError("cascade_refine: gt_boxes must be [N, G, 4]")
    ocls = torch.empty((N, S), dtype=torch.int64, device=dev)
    oidx = torch.empty((N, S), dtype=torch.int64, device=dev)
    ogtb = torch.empty((N, S, 4), dtype=torch.float32, device=dev)
    olv = torch.empty((N, S), dtype=torch.bool, device=dev)
    rc = _C.lib().d2mi_cascade_refine(
        _C.ptr(deltas), _C.ptr(boxes), _C.ptr(v), _C.ptr(image_hw), N, S, w4, float(scale_clamp),
        1, _C.ptr(gt_boxes), _C.ptr(m), _C.ptr(c), _C.ptr(d), _C.ptr(gt_classes),
        int(gt_classes.dtype is torch.int64), G, float(iou_thr), int(num_classes), _C.ptr(ob),
        _C.ptr(ov), _C.ptr(ocls), _C.ptr(oidx), _C.ptr(ogtb), _C.ptr(olv), _C.stream_of(dev))
    _C.check(rc, "d2mi_cascade_refine")
    return {"boxes": ob, "is_valid": ov, "gt_classes": ocls, "gt_index": oidx, "gt_boxes": ogtb,
            "loss_valid": olv}
