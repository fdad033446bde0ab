"""Fused post-processing: Matrix NMS and SOLOv2 inference (csrc/matrix_nms.hip,
solo.hip), the RPN proposals, Fast R-CNN and RetinaNet inference
(proposals.hip, retina_post.hip), the RPN head's gather / scatter
(rpn_loss.hip), YOLOv4 (yolo.hip) and mask pasting (paste_masks.hip)."""
import numpy as np
import torch

from ... import _C
from ...utils import host_sync
from ._common import _DEFAULT_SCALE_CLAMP, _f32c, _i32c, get_tuning
from .conv import conv2d_nhwc
from .timing import KernelTimer


# -------------------------------------------------------------- matrix NMS
def matrix_nms_scores(masks, classes, scores, sum_masks=None, kernel="gaussian", sigma=2.0):
    if kernel not in ("gaussian", "linear"):
        raise NotImplementedError(f"NMS kernel {kernel} not implemented yet.")
    M = masks.shape[0]
    masks2 = _f32c(masks.reshape(M, -1))
    classes = classes.to(torch.int64).contiguous()
    scores = _f32c(scores)
    _C.require_device(masks2, classes, scores)
    sm = _f32c(sum_masks) if sum_masks is not None else None
    out = torch.empty_like(scores)
    wsb = _C.lib().d2mi_matrix_nms_workspace_size(M)
    ws = _C.workspace(wsb, masks.device)
    rc = _C.lib().d2mi_matrix_nms(_C.ptr(masks2), _C.ptr(classes), _C.ptr(scores), _C.ptr(sm), M,
                                  masks2.shape[1], 0 if kernel == "gaussian" else 1, float(sigma),
                                  _C.ptr(out), _C.ptr(ws), wsb, _C.stream_of(masks.device))
    _C.check(rc, "d2mi_matrix_nms")
    return out


def solo_inference(cate_logits, kernels, mask_features, strides, out_hw, score_thresh=0.1,
                   mask_thresh=0.5, update_thresh=0.05, pre_nms_topk=500, max_detections=100,
                   nms_kernel="gaussian", nms_sigma=2.0, debug=None):
    """MaskKernelBranch.inference (solo_v2.py:476-627) on the HIP stages of
    csrc/solo.hip.  cate_logits[l] [N,S_l,S_l,K] (pre-sigmoid), kernels[l]
    [N,S_l,S_l,D], mask_features [N,Hm,Wm,D], strides[l] (the per-level
    sum_masks floor), out_hw the padded image size.  Returns masks uint8
    [N,max_det,OH,OW], boxes [N,max_det,4], scores, classes int64, is_valid.
    One host read (the live-cell counts that size the dynamic-conv GEMMs).
    debug: a dict to receive the intermediates (tests)."""
    if nms_kernel not in ("gaussian", "linear"):
        raise NotImplementedError(f"NMS kernel {nms_kernel} not implemented yet.")
    cate = [_f32c(t) for t in cate_logits]
    kern = [_f32c(t) for t in kernels]
    feats = _f32c(mask_features)
    _C.require_device(feats, *cate, *kern)
    N, K = cate[0].shape[0], cate[0].shape[-1]
    D = kern[0].shape[-1]
    _, Hm, Wm, D2 = feats.shape
    if D != D2:
        raise ValueError(f"kernel dims {D} != mask feature dims {D2}")
    P = Hm * Wm
    L = len(cate)
    grids = [int(t.shape[1]) for t in cate]
    T = sum(g * g for g in grids)
    dev = feats.device
    st = _C.stream_of(dev)
    lib = _C.lib()
    g_arr = _C.host_array(_C.ctypes.c_int32, grids)
    s_arr = _C.host_array(_C.c_float, [float(s) for s in strides])
    probs = torch.empty((N, T, K), dtype=torch.float32, device=dev)
    live_cells = torch.empty((N, T), dtype=torch.int32, device=dev)
    live_row = torch.empty((N, T), dtype=torch.int32, device=dev)
    live_count = torch.empty((N,), dtype=torch.int32, device=dev)
    rc = lib.d2mi_solo_cells(_C.host_array(_C.c_void_p, [t.data_ptr() for t in cate]), g_arr, L,
                             N, K, float(score_thresh), _C.ptr(probs), _C.ptr(live_cells),
                             _C.ptr(live_row), _C.ptr(live_count), st)
    _C.check(rc, "d2mi_solo_cells")
    counts = host_sync.read_ints(live_count)  # the one host synchronisation
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    R = offs[-1]
    row_off = torch.tensor(offs[:-1], dtype=torch.int32, device=dev)
    kern_all = torch.cat([k.reshape(N, -1, D) for k in kern], 1)  # [N, T, D]
    logits = torch.empty((max(R, 1), P), dtype=torch.float32, device=dev)
    for n in range(N):
        c = counts[n]
        if c == 0:
            continue
        rows = kern_all[n].index_select(0, live_cells[n, :c].long()).reshape(1, 1, c, D)
        # dynamic 1x1 conv (solo_v2.py:509-511): one MFMA GEMM per image,
        # [c, D] x [P, D]^T -> [c, P] written straight into the shared buffer
        conv2d_nhwc(rows, feats[n].reshape(1, 1, P, D), out=logits[offs[n]:offs[n + 1]].view(
            1, 1, c, P))
    sum_masks = torch.empty((max(R, 1),), dtype=torch.float32, device=dev)
    sum_scores = torch.empty_like(sum_masks)
    ev = KernelTimer.start()
    rc = lib.d2mi_solo_mask_stats(_C.ptr(logits), R, P, float(mask_thresh), _C.ptr(sum_masks),
                                  _C.ptr(sum_scores), st)
    KernelTimer.stop(ev, "solo_mask_stats", 4 * R * P)  # the dynamic-conv logits read once
    _C.check(rc, "d2mi_solo_mask_stats")
    k = int(min(pre_nms_topk, T * K))
    top_scores = torch.empty((N, k), dtype=torch.float32, device=dev)
    top_classes = torch.empty((N, k), dtype=torch.int64, device=dev)
    top_sum = torch.empty((N, k), dtype=torch.float32, device=dev)
    top_count = torch.empty((N,), dtype=torch.int32, device=dev)
    W64 = (P + 63) // 64
    bits = torch.empty((N, k, W64), dtype=torch.int64, device=dev)
    wsb = lib.d2mi_solo_select_workspace_size(N, T, K, k)
    ws = _C.workspace(wsb, dev)
    rc = lib.d2mi_solo_select(_C.ptr(probs), _C.ptr(live_row), _C.ptr(row_off), _C.ptr(logits),
                              _C.ptr(sum_masks), _C.ptr(sum_scores), g_arr, s_arr, L, N, K, P,
                              float(score_thresh), float(mask_thresh), k, _C.ptr(top_scores),
                              _C.ptr(top_classes), _C.ptr(top_sum), _C.ptr(top_count),
                              _C.ptr(bits), _C.ptr(ws), wsb, st)
    _C.check(rc, "d2mi_solo_select")
    # Matrix NMS (solo_v2.py:541-545) over the padded top-k rows, all images
    decayed = torch.empty((N, k), dtype=torch.float32, device=dev)
    mwsb = lib.d2mi_solo_matrix_nms_workspace_size(N, k)
    mws = _C.workspace(mwsb, dev)
    ev = KernelTimer.start()
    rc = lib.d2mi_solo_matrix_nms(_C.ptr(bits), _C.ptr(top_classes), _C.ptr(top_scores),
                                  _C.ptr(top_sum), N, k, P, 0 if nms_kernel == "gaussian" else 1,
                                  float(nms_sigma), _C.ptr(decayed), _C.ptr(mws), mwsb, st)
    if get_tuning("solo_mfma"):
        # the int8 MFMA intersections (r6): SURVEY 8d D4's 2 N^2 HW ops per
        # image (the reference's full M M^T; the kernel forms the upper
        # triangle) against the I8 MFMA peak
        KernelTimer.stop(ev, "solo_matrix_nms", 2 * N * k * k * P)
    else:
        # the AND + popcount tiles: the bit-packed masks read once (bytes)
        KernelTimer.stop(ev, "solo_matrix_nms_popcount", N * k * W64 * 8)
    _C.check(rc, "d2mi_solo_matrix_nms")
    OH, OW = int(out_hw[0]), int(out_hw[1])
    out_masks = torch.empty((N, max_detections, OH, OW), dtype=torch.uint8, device=dev)
    out_boxes = torch.empty((N, max_detections, 4), dtype=torch.float32, device=dev)
    out_scores = torch.empty((N, max_detections), dtype=torch.float32, device=dev)
    out_classes = torch.empty((N, max_detections), dtype=torch.int64, device=dev)
    out_valid = torch.empty((N, max_detections), dtype=torch.uint8, device=dev)
    fwsb = lib.d2mi_solo_finalize_workspace_size(N, max_detections, OH)
    fws = _C.workspace(fwsb, dev)
    ev = KernelTimer.start()
    rc = lib.d2mi_solo_finalize(_C.ptr(decayed), _C.ptr(top_classes), _C.ptr(top_count),
                                _C.ptr(bits), N, k, Hm, Wm, float(update_thresh),
                                int(max_detections), float(mask_thresh), OH, OW,
                                _C.ptr(out_masks), _C.ptr(out_boxes), _C.ptr(out_scores),
                                _C.ptr(out_classes), _C.ptr(out_valid), _C.ptr(fws), fwsb, st)
    # algorithmic bytes: the uint8 canvas written once (the bit masks are L2-resident)
    KernelTimer.stop(ev, "solo_paste", N * max_detections * OH * OW)
    _C.check(rc, "d2mi_solo_finalize")
    if debug is not None:
        debug.update(probs=probs, live_cells=live_cells, live_row=live_row, counts=counts,
                     row_off=offs, logits=logits[:R], sum_masks=sum_masks[:R],
                     sum_scores=sum_scores[:R], top_scores=top_scores, top_classes=top_classes,
                     top_sum=top_sum, top_count=top_count, mask_bits=bits, decayed=decayed)
    return out_masks, out_boxes, out_scores, out_classes, out_valid.bool()


# ------------------------------------------------------- fused post-processing
# host copies of the cell anchors (constant buffers, often on the GPU: one
# read per element was ~60 device-to-host syncs per training step)
_CELLS = {}


def _cell_values(c):
    """The float32 values of one level's cell anchors as a tuple.  A tensor
    keeps its host copy as an attribute of the tensor object itself (checked
    against its in-place version counter), so the copy lives and dies with
    that tensor: no cache key that another tensor at a reused address could
    match."""
    if not torch.is_tensor(c):
        return tuple(np.asarray(c, np.float32).reshape(-1).tolist())
    got = getattr(c, "_d2mi_host_cells", None)
    if got is None or got[0] != c._version:
        got = (c._version, tuple(c.detach().to(torch.float32).reshape(-1).cpu().tolist()))
        c._d2mi_host_cells = got
    return got[1]


def _cell_host_array(cell_anchors):
    """ctypes array of every level's cell anchors, cached by VALUE (tens of
    floats per level)."""
    key = tuple(_cell_values(c) for c in cell_anchors)
    got = _CELLS.get(key)
    if got is None:
        cells = [v for lv in key for v in lv]
        got = (_C.host_array(_C.c_float, cells), len(cells))
        if len(_CELLS) > 64:
            _CELLS.clear()
        _CELLS[key] = got
    return got


def _level_arrays(tensors, hw, strides, cell_anchors):
    L = len(tensors)
    ptrs = _C.host_array(_C.c_void_p, [t.data_ptr() for t in tensors])
    lhw = _C.host_array(_C.ctypes.c_int32, [v for h, w in hw for v in (int(h), int(w))])
    st = _C.host_array(_C.c_float, [float(s) for s in strides])
    cells, n = _cell_host_array(cell_anchors)
    return ptrs, lhw, st, cells, n // (4 * L)


def _image_strided(t):
    """t [N, H, W, C] f32 on the device, dense within each image (any image
    stride, e.g. a level view of a concatenated [N, sum HWC] buffer)."""
    N, H, W, C = t.shape
    return (t.dtype == torch.float32 and t.stride(3) == 1 and t.stride(2) == C
            and t.stride(1) == W * C and t.stride(0) >= H * W * C)


def rpn_proposals(logits, deltas, strides, cell_anchors, image_hw, pre_nms_topk, post_nms_topk,
                  nms_thresh, min_box_side_len=0.0, weights=(1.0, 1.0, 1.0, 1.0),
                  scale_clamp=_DEFAULT_SCALE_CLAMP):
    """find_top_rpn_proposals (rpn_outputs.py:29-132) fused with anchor
    generation and decode.  logits[l] [N,H,W,A], deltas[l] [N,H,W,A*4]; each
    dense within an image, any image stride (level views of the training
    head's concatenated outputs go in without copies: d2mi_rpn_proposals_ex)."""
    strided = (all(_image_strided(t) for t in list(logits) + list(deltas))
               and all(t.data_ptr() % 16 == 0 for t in deltas))
    if not strided:
        logits = [_f32c(t) for t in logits]
        deltas = [_f32c(t) for t in deltas]
    image_hw = _i32c(image_hw)
    _C.require_device(image_hw, *logits, *deltas)
    N = logits[0].shape[0]
    L = len(logits)
    hw = [(t.shape[1], t.shape[2]) for t in logits]
    lp, lhw, st, cells, A = _level_arrays(logits, hw, strides, cell_anchors)
    dp = _C.host_array(_C.c_void_p, [t.data_ptr() for t in deltas])
    dev = logits[0].device
    ob = torch.empty((N, post_nms_topk, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((N, post_nms_topk), dtype=torch.float32, device=dev)
    ov = torch.empty((N, post_nms_topk), dtype=torch.uint8, device=dev)
    wsb = _C.lib().d2mi_rpn_proposals_workspace_size(N, L, lhw, A, pre_nms_topk, post_nms_topk)
    ws = _C.workspace(wsb, dev)
    sl = _C.host_array(_C.ctypes.c_int64, [t.stride(0) for t in logits])
    sd = _C.host_array(_C.ctypes.c_int64, [t.stride(0) for t in deltas])
    rc = _C.lib().d2mi_rpn_proposals_ex(lp, dp, sl, sd, lhw, st, cells, L, A, N, _C.ptr(image_hw),
                                     int(pre_nms_topk), int(post_nms_topk), float(nms_thresh),
                                     float(min_box_side_len),
                                     _C.host_array(_C.c_float, [float(w) for w in weights]),
                                     float(scale_clamp), _C.ptr(ob), _C.ptr(os_), _C.ptr(ov),
                                     _C.ptr(ws), wsb, _C.stream_of(dev))
    _C.check(rc, "d2mi_rpn_proposals")
    return ob, os_, ov.bool()


def rpn_head_gather(ys, A):
    """d2mi_rpn_head_gather: the fused head's per-level outputs ys[l] [N, H, W, C]
    -> (logits [N, T*A], deltas [N, T*A, 4]) in the RPNOutputs layout."""
    ys = [_f32c(y) for y in ys]
    _C.require_device(*ys)
    N, C = ys[0].shape[0], ys[0].shape[-1]
    hw = [y.shape[1] * y.shape[2] for y in ys]
    T = sum(hw)
    dev = ys[0].device
    pl = torch.empty((N, T * A), dtype=torch.float32, device=dev)
    pd = torch.empty((N, T * A, 4), dtype=torch.float32, device=dev)
    rc = _C.lib().d2mi_rpn_head_gather(_C.host_array(_C.c_void_p, [y.data_ptr() for y in ys]),
                                       _C.host_array(_C.ctypes.c_int32, hw), len(ys), N, A, C,
                                       _C.ptr(pl), _C.ptr(pd), _C.stream_of(dev))
    _C.check(rc, "d2mi_rpn_head_gather")
    return pl, pd


def rpn_head_scatter(g_logits, g_deltas, shapes, A):
    """Adjoint of rpn_head_gather: -> per-level [N, H, W, C] gradients (every
    element written; either input may be None = zero)."""
    g_logits = _f32c(g_logits) if g_logits is not None else None
    g_deltas = _f32c(g_deltas) if g_deltas is not None else None
    ref = g_logits if g_logits is not None else g_deltas
    dev = ref.device
    N, C = shapes[0][0], shapes[0][-1]
    outs = [torch.empty(tuple(s), dtype=torch.float32, device=dev) for s in shapes]
    hw = [s[1] * s[2] for s in shapes]
    rc = _C.lib().d2mi_rpn_head_scatter(_C.ptr(g_logits), _C.ptr(g_deltas),
                                        _C.host_array(_C.ctypes.c_int32, hw), len(shapes), N, A, C,
                                        _C.host_array(_C.c_void_p, [o.data_ptr() for o in outs]),
                                        _C.stream_of(dev))
    _C.check(rc, "d2mi_rpn_head_scatter")
    return outs


def _fast_rcnn_inference(entry, what, logits, lead, deltas, proposals, roi_img, roi_slot,
                         num_images, P, image_hw, weights, score_thresh, nms_thresh,
                         topk_per_image, cls_agnostic, scale_clamp, nms_cls_agnostic):
    """The body of the two Fast R-CNN inference ops.  entry: the op's own C
    entry point (``what``: its name); logits: its contiguous f32 [R, K+1] logit
    tensors; lead: the arguments the entry takes for them, ahead of the rest."""
    deltas, proposals = _f32c(deltas), _f32c(proposals)
    roi_img, roi_slot, image_hw = _i32c(roi_img), _i32c(roi_slot), _i32c(image_hw)
    _C.require_device(*logits, deltas, proposals, roi_img, roi_slot, image_hw)
    R, K1 = logits[0].shape
    K = K1 - 1
    N = int(num_images)
    dev = deltas.device
    ob = torch.empty((N, topk_per_image, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((N, topk_per_image), dtype=torch.float32, device=dev)
    oc = torch.empty((N, topk_per_image), dtype=torch.int64, device=dev)
    ov = torch.empty((N, topk_per_image), dtype=torch.uint8, device=dev)
    oroi = torch.empty((N, topk_per_image), dtype=torch.int32, device=dev)
    wsb = _C.lib().d2mi_fast_rcnn_workspace_size(N, int(P), K, float(score_thresh),
                                                 int(topk_per_image))
    ws = _C.workspace(wsb, dev)
    rc = entry(
        *lead, _C.ptr(deltas), _C.ptr(proposals), _C.ptr(roi_img), _C.ptr(roi_slot), R, N,
        int(P), K, int(bool(cls_agnostic)) | (int(bool(nms_cls_agnostic)) << 1), _C.ptr(image_hw),
        _C.host_array(_C.c_float, [float(w) for w in weights]), float(scale_clamp),
        float(score_thresh), float(nms_thresh), int(topk_per_image), _C.ptr(ob), _C.ptr(os_),
        _C.ptr(oc), _C.ptr(ov), _C.ptr(oroi), _C.ptr(ws), wsb, _C.stream_of(dev))
    _C.check(rc, what)
    return ob, os_, oc, ov.bool(), oroi


def fast_rcnn_inference(logits, deltas, proposals, roi_img, roi_slot, num_images, P, image_hw,
                        weights, score_thresh, nms_thresh, topk_per_image,
                        cls_agnostic=False, scale_clamp=_DEFAULT_SCALE_CLAMP, nms_cls_agnostic=False):
    """FastRCNNOutputs.inference + fast_rcnn_inference (fast_rcnn.py:28-187,
    :359-395): softmax, decode, clip, threshold, class-offset NMS (plain NMS
    with nms_cls_agnostic, fast_rcnn.py:138-139), pad.  cls_agnostic: one
    class-agnostic box per ROI (deltas [R, 4])."""
    logits = _f32c(logits)
    return _fast_rcnn_inference(
        _C.lib().d2mi_fast_rcnn_inference, "d2mi_fast_rcnn_inference", [logits],
        [_C.ptr(logits)], deltas, proposals, roi_img, roi_slot, num_images, P, image_hw, weights,
        score_thresh, nms_thresh, topk_per_image, cls_agnostic, scale_clamp, nms_cls_agnostic)


def fast_rcnn_inference_stages(stage_logits, deltas, proposals, roi_img, roi_slot, num_images, P,
                               image_hw, weights, score_thresh, nms_thresh, topk_per_image,
                               cls_agnostic=False, scale_clamp=_DEFAULT_SCALE_CLAMP,
                               nms_cls_agnostic=False):
    """fast_rcnn_inference on the class scores of a cascade averaged over its
    stages (cascade_rcnn.py:123-139; d2mi_fast_rcnn_inference_stages):
    stage_logits is the list of 1..4 per-stage logits [R, K+1]; deltas,
    proposals and weights are the last stage's."""
    stage_logits = [_f32c(t) for t in stage_logits]
    if not 1 <= len(stage_logits) <= 4:
        raise ValueError(f"fast_rcnn_inference_stages: 1..4 stages (got {len(stage_logits)})")
    if any(t.shape != stage_logits[0].shape for t in stage_logits):
        raise ValueError("fast_rcnn_inference_stages: every stage's logits must be [R, K+1]")
    lead = [_C.ptr(t) for t in stage_logits] + [None] * (4 - len(stage_logits))
    return _fast_rcnn_inference(
        _C.lib().d2mi_fast_rcnn_inference_stages, "d2mi_fast_rcnn_inference_stages",
        stage_logits, lead + [len(stage_logits)], deltas, proposals, roi_img, roi_slot,
        num_images, P, image_hw, weights, score_thresh, nms_thresh, topk_per_image, cls_agnostic,
        scale_clamp, nms_cls_agnostic)


def retinanet_inference(box_cls, box_delta, strides, cell_anchors, num_classes, topk_candidates,
                        score_threshold, nms_threshold, max_detections,
                        weights=(1.0, 1.0, 1.0, 1.0), scale_clamp=_DEFAULT_SCALE_CLAMP):
    """RetinaNetHead.inference (retinanet.py:285-387).  box_cls[l] [N,H,W,A*K],
    box_delta[l] [N,H,W,A*4]."""
    box_cls = [_f32c(t) for t in box_cls]
    box_delta = [_f32c(t) for t in box_delta]
    _C.require_device(*box_cls, *box_delta)
    N = box_cls[0].shape[0]
    L = len(box_cls)
    hw = [(t.shape[1], t.shape[2]) for t in box_cls]
    cp, lhw, st, cells, A = _level_arrays(box_cls, hw, strides, cell_anchors)
    bp = _C.host_array(_C.c_void_p, [t.data_ptr() for t in box_delta])
    dev = box_cls[0].device
    ob = torch.empty((N, max_detections, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((N, max_detections), dtype=torch.float32, device=dev)
    oc = torch.empty((N, max_detections), dtype=torch.int32, device=dev)
    ov = torch.empty((N, max_detections), dtype=torch.uint8, device=dev)
    wsb = _C.lib().d2mi_retinanet_workspace_size(N, L, lhw, A, int(num_classes),
                                                 int(topk_candidates))
    ws = _C.workspace(wsb, dev)
    ev = KernelTimer.start()
    rc = _C.lib().d2mi_retinanet_inference(
        cp, bp, lhw, st, cells, L, A, int(num_classes), N, int(topk_candidates),
        float(score_threshold), float(nms_threshold), int(max_detections),
        _C.host_array(_C.c_float, [float(w) for w in weights]), float(scale_clamp), _C.ptr(ob),
        _C.ptr(os_), _C.ptr(oc), _C.ptr(ov), _C.ptr(ws), wsb, _C.stream_of(dev))
    # algorithmic bytes: the dense logit scan, 4 B per (anchor, class) score
    # (64.5 MB per image at 1333x800)
    KernelTimer.stop(ev, "retinanet_postprocess", 4 * sum(t.numel() for t in box_cls))
    _C.check(rc, "d2mi_retinanet_inference")
    return ob, os_, oc, ov.bool()


# -------------------------------------------------------------------- YOLOv4
def yolo_host_arrays(level_hw, strides, cell_anchors, scale_yx):
    """The host arrays of the two YOLOv4 entry points (d2mi.h): level_hw,
    strides, the (h, w) of each [0, 0, h, w] cell anchor, and per level
    (scale_yx, 0.5 * (scale_yx - 1)) formed in double as the reference's Python
    scalars are.  Returns (lhw, strides, cell_hw, scale, L, A)."""
    L = len(level_hw)
    cells = [torch.as_tensor(c, dtype=torch.float32).reshape(-1, 4) for c in cell_anchors]
    if len(cells) != L or len(strides) != L or len(scale_yx) != L:
        raise ValueError("yolov4: one stride, cell-anchor set and scale_yx per level")
    A = cells[0].shape[0]
    if any(c.shape[0] != A for c in cells):
        raise ValueError("yolov4: every level must have the same number of anchors")
    lhw = _C.host_array(_C.ctypes.c_int32, [v for h, w in level_hw for v in (int(h), int(w))])
    st = _C.host_array(_C.c_float, [float(s) for s in strides])
    chw = _C.host_array(_C.c_float, [float(v) for c in cells for v in c[:, 2:].reshape(-1)])
    sc = _C.host_array(_C.c_float, [v for s in scale_yx
                                    for v in (float(s), 0.5 * (float(s) - 1))])
    return lhw, st, chw, sc, L, A


def _yolo_levels(pred_logits, num_classes, A):
    logits = [_f32c(t) for t in pred_logits]
    _C.require_device(*logits)
    N = logits[0].shape[0]
    for t in logits:
        if t.dim() != 4 or t.shape[0] != N or t.shape[3] != A * (5 + int(num_classes)):
            raise ValueError(f"yolov4: logits must be [N, H, W, A * (5 + K)], got {tuple(t.shape)}")
    return logits, N


def yolov4_predictions(pred_logits, strides, cell_anchors, scale_yx, num_classes):
    """YOLOV4Outputs._get_predictions (yolov4_outputs.py:208-264), dense:
    pred_logits[l] [N, H, W, A * (5 + K)] -> boxes [N, P, 4], conf [N, P],
    score [N, P] (the max-class probability) and cls [N, P] int32."""
    hw = [(t.shape[1], t.shape[2]) for t in pred_logits]
    lhw, st, chw, sc, L, A = yolo_host_arrays(hw, strides, cell_anchors, scale_yx)
    logits, N = _yolo_levels(pred_logits, num_classes, A)
    P = sum(h * w for h, w in hw) * A
    dev = logits[0].device
    boxes = torch.empty((N, P, 4), dtype=torch.float32, device=dev)
    conf = torch.empty((N, P), dtype=torch.float32, device=dev)
    score = torch.empty((N, P), dtype=torch.float32, device=dev)
    cls = torch.empty((N, P), dtype=torch.int32, device=dev)
    rc = _C.lib().d2mi_yolov4_predictions(
        _C.host_array(_C.c_void_p, [t.data_ptr() for t in logits]), lhw, st, chw, sc, L, A,
        int(num_classes), N, _C.ptr(boxes), _C.ptr(conf), _C.ptr(score), _C.ptr(cls),
        _C.stream_of(dev))
    _C.check(rc, "d2mi_yolov4_predictions")
    return boxes, conf, score, cls


def yolov4_inference(pred_logits, strides, cell_anchors, scale_yx, num_classes, score_threshold,
                     nms_threshold, max_detections):
    """YOLOV4Outputs.inference (yolov4_outputs.py:331-390) fused
    (d2mi_yolov4_inference): boxes [N, D, 4], scores [N, D], classes [N, D]
    int32, is_valid [N, D] bool, D = max_detections."""
    hw = [(t.shape[1], t.shape[2]) for t in pred_logits]
    lhw, st, chw, sc, L, A = yolo_host_arrays(hw, strides, cell_anchors, scale_yx)
    logits, N = _yolo_levels(pred_logits, num_classes, A)
    dev = logits[0].device
    ob = torch.empty((N, max_detections, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((N, max_detections), dtype=torch.float32, device=dev)
    oc = torch.empty((N, max_detections), dtype=torch.int32, device=dev)
    ov = torch.empty((N, max_detections), dtype=torch.uint8, device=dev)
    wsb = _C.lib().d2mi_yolov4_workspace_size(N, L, lhw, A)
    ws = _C.workspace(wsb, dev)
    ev = KernelTimer.start()
    rc = _C.lib().d2mi_yolov4_inference(
        _C.host_array(_C.c_void_p, [t.data_ptr() for t in logits]), lhw, st, chw, sc, L, A,
        int(num_classes), N, float(score_threshold), float(nms_threshold), int(max_detections),
        _C.ptr(ob), _C.ptr(os_), _C.ptr(oc), _C.ptr(ov), _C.ptr(ws), wsb, _C.stream_of(dev))
    # algorithmic bytes: the dense logit read, 4 B per logit
    KernelTimer.stop(ev, "yolov4_postprocess", 4 * sum(t.numel() for t in logits))
    _C.check(rc, "d2mi_yolov4_inference")
    return ob, os_, oc, ov.bool()


def spp_pool(x):
    """The SPP block's pools and concat (necks/yolov4.py:175-178) in one
    launch: x [N, H, W, C] -> [N, H, W, 4C] = [pool13, pool9, pool5, x], the
    pools stride 1 over the zero-padded map.  No autograd."""
    x = _f32c(x)
    _C.require_device(x)
    N, H, W, C = x.shape
    out = torch.empty((N, H, W, 4 * C), dtype=torch.float32, device=x.device)
    rc = _C.lib().d2mi_spp_pool(_C.ptr(x), N, H, W, C, _C.ptr(out), _C.stream_of(x.device))
    _C.check(rc, "d2mi_spp_pool")
    return out


ACT_LEAKY_RELU, ACT_MISH = 1, 2


def activation_(x, code, alpha=0.0):
    """In-place leaky_relu(alpha) (code ACT_LEAKY_RELU) or mish (ACT_MISH) over
    a dense float32 tensor (d2mi_activation).  No autograd.  Returns x."""
    _C.require_device(x)
    if x.dtype is not torch.float32 or not x.is_contiguous():
        raise ValueError("activation_: a contiguous float32 tensor")
    rc = _C.lib().d2mi_activation(_C.ptr(x), x.numel(), int(code), float(alpha),
                                  _C.stream_of(x.device))
    _C.check(rc, "d2mi_activation")
    return x


# ------------------------------------------------------------- mask pasting
def paste_masks(box_masks, boxes, out_shape, valid=None, yx_scale=None, threshold=0.5):
    """reframe_box_masks_to_image_masks (lib/structures/mask_ops.py:7-56) with
    the threshold of detector_postprocess (postprocessing.py:47-49) fused:
    box_masks [D, mh, mw] f32 probabilities, boxes [D, 4] yxyx absolute,
    out_shape (H, W) canvas; valid [D] bool (False rows -> zeros); yx_scale
    [D, 2] f32 per-box (sy, sx) applied first ("fixed" format).
    Returns [D, H, W] uint8."""
    box_masks = _f32c(box_masks)
    boxes = _f32c(boxes)
    tensors = [box_masks, boxes]
    if valid is not None:
        valid = valid.to(torch.uint8).contiguous()
        tensors.append(valid)
    if yx_scale is not None:
        yx_scale = _f32c(yx_scale)
        tensors.append(yx_scale)
    _C.require_device(*tensors)
    D, mh, mw = box_masks.shape
    H, W = int(out_shape[0]), int(out_shape[1])
    out = torch.empty((D, H, W), dtype=torch.uint8, device=boxes.device)
    ev = KernelTimer.start()
    rc = _C.lib().d2mi_paste_masks(_C.ptr(box_masks), _C.ptr(boxes), _C.ptr(yx_scale),
                                   _C.ptr(valid), D, mh, mw, H, W, float(threshold),
                                   _C.ptr(out), _C.stream_of(boxes.device))
    # algorithmic bytes: the u8 canvas written + the box masks read
    KernelTimer.stop(ev, "paste_masks", D * H * W + box_masks.numel() * 4)
    _C.check(rc, "d2mi_paste_masks")
    return out
