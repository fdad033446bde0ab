"""ROIAlign forward / backward over the feature pyramid (csrc/roi_align.hip)
and its unique-bytes traffic model.  Owns the MERGED_BWD and DEFER_PIXELS
toggles: readers and writers use ops.roi.<name>."""
import math

import numpy as np
import torch

from ... import _C
from .. import handoff
from ._common import BOX_MODE_ALIGNED, BOX_MODE_RAW, BOX_MODE_UNALIGNED, _f32c, _i32c
from .timing import KernelTimer


def roi_touched_rows(boxes, box_ind, params, shapes, return_ids=False):
    """Distinct feature rows (level, image, y, x) that one ROIAlign forward
    reads (the 4 bilinear corners of every in-range sample): the unique-bytes
    model of bench.py's roofline (rows x C x 4 bytes is the least HBM
    traffic that can deliver the launch's inputs, however many samples share
    a row).  A float32 torch restatement of roi_geom / make_tap in
    csrc/roi_align.hip, for the byte count only (a log-boundary box may land
    on the other level here: immaterial for a traffic model)."""
    (oh, ow, scales, sr, mode, pad, assign, min_l, max_l, canon_s, canon_l, _) = params
    dev = boxes.device
    b = boxes.detach().float().reshape(-1, 4)
    R = b.shape[0]
    if R == 0:
        return torch.zeros(0, dtype=torch.long, device=dev) if return_ids else 0
    if assign and len(shapes) > 1:
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        v = canon_l + torch.log(torch.sqrt(area) / canon_s + 2.220446049250313e-16) / math.log(2)
        lv = torch.nan_to_num(torch.floor(v), nan=min_l).clamp(min_l, max_l).long() - min_l
    else:
        lv = torch.zeros(R, dtype=torch.long, device=dev)
    Hs = torch.tensor([s[1] for s in shapes], device=dev)[lv]
    Ws = torch.tensor([s[2] for s in shapes], device=dev)[lv]
    sc = torch.tensor(list(scales), dtype=torch.float32, device=dev)[lv]
    S = max(sr, 1)
    ch, cw = oh * S, ow * S
    y1, x1, y2, x2 = b.unbind(1)
    if mode != BOX_MODE_RAW:
        y1, x1, y2, x2 = y1 * sc, x1 * sc, y2 * sc, x2 * sc
    Hp, Wp = (Hs + 2, Ws + 2) if pad else (Hs, Ws)
    if pad:
        y1, x1, y2, x2 = y1 + 1, x1 + 1, y2 + 1, x2 + 1
    i0, i1 = (Hp - 1).float(), (Wp - 1).float()
    if mode == BOX_MODE_ALIGNED:
        sh, sw = (y2 - y1) / ch, (x2 - x1) / cw
        ny, nx = (y1 + sh / 2 - 0.5) / i0, (x1 + sw / 2 - 0.5) / i1
        y1, x1, y2, x2 = ny, nx, ny + sh * (ch - 1) / i0, nx + sw * (cw - 1) / i1
    elif mode == BOX_MODE_UNALIGNED:
        y1, y2, x1, x2 = y1 / Hp.float(), y2 / Hp.float(), x1 / Wp.float(), x2 / Wp.float()

    def taps(c1, c2, img_p, img, crop):
        i = torch.arange(crop, device=dev, dtype=torch.float32)
        if crop > 1:
            pos = c1[:, None] * (img_p - 1).float()[:, None] + i * (
                (c2 - c1) * (img_p - 1).float() / (crop - 1))[:, None]
        else:
            pos = (0.5 * (c1 + c2) * (img_p - 1).float())[:, None]
        ok = (pos >= 0) & (pos <= (img_p - 1).float()[:, None])
        lo, hi = torch.floor(pos).long(), torch.ceil(pos).long()
        d = 1 if pad else 0
        top = img[:, None] - 1
        return ok, (lo - d).clamp(min=0).minimum(top), (hi - d).clamp(min=0).minimum(top)

    oky, ylo, yhi = taps(y1, y2, Hp, Hs, ch)
    okx, xlo, xhi = taps(x1, x2, Wp, Ws, cw)
    n = box_ind.detach().long().reshape(-1)
    base = torch.tensor([0] + [s[0] * s[1] * s[2] for s in shapes], device=dev).cumsum(0)
    img0 = (base[lv] + n * Hs * Ws)[:, None, None]
    ok = (oky[:, :, None] & okx[:, None, :]).reshape(-1)
    ids = []
    for yy in (ylo, yhi):
        for xx in (xlo, xhi):
            ids.append((img0 + yy[:, :, None] * Ws[:, None, None] + xx[:, None, :]).reshape(-1)[ok])
    u = torch.unique(torch.cat(ids))
    return u if return_ids else int(u.numel())


class _RoIAlignFn(torch.autograd.Function):
    """ROIAlign forward/backward over 1..8 feature levels.  Boxes carry no
    gradient (crop_and_resize stop_gradient, lib/layers/functional.py:120).

    grad_share (a handoff.PoolerShare of two poolings of the SAME feature maps,
    the box and mask poolers of a training step, both of whose backwards always
    run): the first backward writes the full maps and leaves them there,
    returning no gradient for the features; the second adds its
    contributions into them (d2mi_roi_align_bwd_ex accumulate: no second
    183 MB clear at 1333x800, no autograd add of two maps) and returns the
    sum — bit-identical to autograd's add of the two maps."""

    @staticmethod
    def forward(ctx, boxes, box_ind, params, grad_share, *feats):
        feats = [_f32c(f) for f in feats]
        boxes = _f32c(boxes)
        box_ind = _i32c(box_ind)
        _C.require_device(boxes, box_ind, *feats)
        (out_h, out_w, scales, sr, mode, pad, assign, min_l, max_l, canon_s, canon_l,
         want_level) = params
        L = len(feats)
        C = feats[0].shape[-1]
        R = boxes.shape[0]
        out = torch.empty((R, out_h, out_w, C), dtype=torch.float32, device=boxes.device)
        level = torch.empty((R,), dtype=torch.int32, device=boxes.device) if want_level else None
        fp = _C.host_array(_C.c_void_p, [f.data_ptr() for f in feats])
        dims = _C.host_array(_C.ctypes.c_int32,
                             [v for f in feats for v in (f.shape[0], f.shape[1], f.shape[2])])
        sc = _C.host_array(_C.c_float, list(scales))
        ev = KernelTimer.start()
        rc = _C.lib().d2mi_roi_align_fwd(fp, dims, sc, L, C, _C.ptr(boxes), _C.ptr(box_ind), R,
                                         out_h, out_w, sr, mode, pad, assign, min_l, max_l,
                                         canon_s, canon_l, _C.ptr(level), _C.ptr(out),
                                         _C.stream_of(boxes.device))
        S = max(sr, 1) ** 2
        # algorithmic bytes: 4 f32 corner reads per sample + 1 f32
        # write per output.  Feature-pyramid pooling (C >= 64, the hot path) and
        # narrow crops (the C = 1 mask-target crop_and_resize) are timed apart,
        # and the box pooler (7x7) apart from the mask pooler (14x14, a few
        # dozen ROIs per step: latency-bound)
        name = ("crop_and_resize_fwd_narrow" if C < 64 else
                "roi_align_fwd" if out_h * out_w <= 49 else "roi_align_fwd_mask")
        shapes = [tuple(f.shape) for f in feats]
        KernelTimer.stop(ev, name, R * out_h * out_w * C * (16 * S + 4),
                         extra=lambda: {"unique_bytes": C * 4 * (
                             roi_touched_rows(boxes, box_ind, params, shapes) + R * out_h * out_w)})
        _C.check(rc, "d2mi_roi_align_fwd")
        ctx.params = params
        ctx.share = grad_share
        ctx.shapes = [f.shape for f in feats]
        # per-level input-gradient hand-off with another consumer of the same
        # maps (the RPN head conv: a handoff.Pair per level)
        ctx.pairs = [handoff.tagged(f, handoff.LEVEL_PAIR) for f in feats]
        ctx.save_for_backward(boxes, box_ind)
        ctx.set_materialize_grads(False)  # level (non-differentiable): no zero grad
        if level is not None:
            ctx.mark_non_differentiable(level)
        return out, level

    @staticmethod
    def backward(ctx, grad_out, _grad_level):
        if grad_out is None:
            return (None,) * (4 + len(ctx.shapes))
        boxes, box_ind = ctx.saved_tensors
        (out_h, out_w, scales, sr, mode, pad, assign, min_l, max_l, canon_s, canon_l,
         _) = ctx.params
        share = ctx.share
        if share is not None and MERGED_BWD and grad_out.shape[-1] >= 64:
            # a pair of poolings of the same maps: the first backward only
            # leaves its grad_out; the second runs ONE backward over both ROI
            # sets (one emit per set, one sort, one gather pass summing each
            # set's run apart, set 0 + set 1)
            first = share.rois.take()
            g = _f32c(grad_out)
            if first is None:
                share.rois.put((boxes, box_ind, g, ctx.params))
                return (None,) * (4 + len(ctx.shapes))
            # levels whose other consumer already left its input gradient:
            # accumulate into it; the others: their pixel pass is deferred
            # into that consumer's backward, which writes the level's full
            # map (DEFER_PIXELS), or the map is written here and left for it
            given = [pr.take() if pr is not None else None for pr in ctx.pairs]
            defer = [DEFER_PIXELS and pr is not None and gv is None
                     for pr, gv in zip(ctx.pairs, given)]
            grads = _roi_align_bwd2(first, (boxes, box_ind, g, ctx.params), ctx.shapes, given,
                                    defer)
            out = []
            for pr, gv, gr in zip(ctx.pairs, given, grads):
                if pr is not None and gv is None:
                    # the other consumer adds it: a deferred pixel pass into its
                    # dgrad, or the map in its dgrad epilogue
                    pr.deposit(gr, "RPN head / ROI pooler level")
                    out.append(None)
                else:
                    out.append(gr)
            return (None, None, None, None, *out)
        prior = share.maps.take() if share is not None else None
        if prior is not None:  # second of a pair: add into the first's maps
            grads = prior
        else:
            # every element is written by d2mi_roi_align_bwd (zero-fill + touched pixels)
            grads = [torch.empty(s, dtype=torch.float32, device=boxes.device) for s in ctx.shapes]
        g = _f32c(grad_out)
        gp = _C.host_array(_C.c_void_p, [x.data_ptr() for x in grads])
        dims = _C.host_array(_C.ctypes.c_int32, [v for s in ctx.shapes for v in (s[0], s[1], s[2])])
        sc = _C.host_array(_C.c_float, list(scales))
        R, C = boxes.shape[0], ctx.shapes[0][-1]
        wsb = _C.lib().d2mi_roi_align_bwd_workspace_size(dims, len(grads), C, R, out_h, out_w, sr)
        ws = _C.workspace(wsb, boxes.device)
        ev = KernelTimer.start()
        rc = _C.lib().d2mi_roi_align_bwd_ex(gp, dims, sc, len(grads), C, _C.ptr(boxes),
                                            _C.ptr(box_ind), R, out_h, out_w, sr, mode, pad,
                                            assign, min_l, max_l, canon_s, canon_l, _C.ptr(g),
                                            int(prior is not None), _C.ptr(ws), wsb,
                                            _C.stream_of(boxes.device))
        # algorithmic bytes: R*oh*ow*C*(4 + 32*S) = the grad_out read
        # + 4 corner read-modify-writes per sample of the reference's scatter
        S = max(sr, 1) ** 2
        maps = sum(int(np.prod(s)) for s in ctx.shapes) * 4
        KernelTimer.stop(ev, "roi_align_bwd" if C >= 64 else "crop_and_resize_bwd_narrow",
                         R * out_h * out_w * C * (4 + 32 * S),
                         extra=lambda: {"unique_bytes": R * out_h * out_w * C * 4 + maps})
        _C.check(rc, "d2mi_roi_align_bwd")
        if share is not None and prior is None:  # first of a pair: hand the maps over
            share.maps.put(grads)
            return (None,) * (4 + len(grads))
        return (None, None, None, None, *grads)


# The box and mask poolers' backwards as one merged backward (False: two
# backwards, the second accumulating into the first's maps; tests compare).
MERGED_BWD = True
# r4: a merged backward whose level is also read by another consumer that has
# not run its backward yet (the RPN head conv) prepares the contributions
# once (d2mi_roi_align_bwd2_ex phase 1) and leaves each such level's pixel
# pass (phase 2) to that consumer, which runs it into its own full dgrad map
# (DeferredPixels.add_into): the level's map is neither cleared here nor
# written twice nor read again by the consumer's epilogue.  False: the full
# maps are written here and added in the consumer's dgrad epilogue (A/B).
DEFER_PIXELS = True


DeferredPixels = handoff.DeferredPixels  # (one level's pixel pass, handed to its consumer)


def _roi_align_bwd2(set0, set1, shapes, given=None, defer=None):
    """d2mi_roi_align_bwd2 over two (boxes, box_ind, grad_out, params) sets
    of the same feature maps (equal level / box-mode parameters).  given[l]:
    a gradient map of level l to accumulate into (returned), or None.
    defer[l]: level l's pixel pass is left to a DeferredPixels (returned in
    its place; d2mi_roi_align_bwd2_ex phase 1 now, phase 2 later)."""
    b0, i0, g0, p0 = set0
    b1, i1, g1, p1 = set1
    if p0[2] != p1[2] or p0[4:11] != p1[4:11]:  # scales, box mode .. canonical level
        raise ValueError("merged ROIAlign backward: the two poolings differ beyond their crops")
    (oh0, ow0, scales, sr0, mode, pad, assign, min_l, max_l, canon_s, canon_l, _) = p0
    oh1, ow1, sr1 = p1[0], p1[1], p1[3]
    dev = b0.device
    L = len(shapes)
    given = given or [None] * L
    defer = defer or [False] * L
    grads, acc_mask = [], 0
    for l, (s, gv) in enumerate(zip(shapes, given)):
        if defer[l]:
            grads.append(None)
            acc_mask |= 1 << l  # (phase 1 leaves the deferred maps alone)
        elif gv is not None and tuple(gv.shape) == tuple(s) and gv.dtype == torch.float32 \
                and gv.is_contiguous():
            grads.append(gv)
            acc_mask |= 1 << l
        elif gv is not None:
            grads.append(_f32c(gv).clone())
            acc_mask |= 1 << l
        else:
            grads.append(torch.empty(s, dtype=torch.float32, device=dev))
    dims = _C.host_array(_C.ctypes.c_int32, [v for s in shapes for v in (s[0], s[1], s[2])])
    sc = _C.host_array(_C.c_float, list(scales))
    C = shapes[0][-1]
    R0, R1 = b0.shape[0], b1.shape[0]
    lib = _C.lib()
    wsb = lib.d2mi_roi_align_bwd2_workspace_size(dims, L, C, R0, oh0, ow0, sr0, R1, oh1, ow1, sr1)
    ws = _C.workspace(wsb, dev)
    st = _C.stream_of(dev)
    S0, S1 = max(sr0, 1) ** 2, max(sr1, 1) ** 2
    d4 = R0 * oh0 * ow0 * C * (4 + 32 * S0) + R1 * oh1 * ow1 * C * (4 + 32 * S1)
    gout_bytes = (R0 * oh0 * ow0 + R1 * oh1 * ow1) * C * 4

    def touched_bytes(levels):
        """unique bytes of a pixel pass: 2 x C x 4 per touched pixel of these
        levels (read + write of an accumulated map) -- the union of the pixels
        the two sets' sample corners touch (roi_touched_rows)."""
        base = np.cumsum([0] + [int(s[0] * s[1] * s[2]) for s in shapes])
        ids = torch.cat([roi_touched_rows(b, i, p, shapes, return_ids=True)
                         for b, i, _, p in (set0, set1)]).unique()
        lo, hi = int(base[min(levels)]), int(base[max(levels) + 1])
        return 2 * C * 4 * int(((ids >= lo) & (ids < hi)).sum())

    def call(maps, acc, phase, lo, hi):
        gp = _C.host_array(_C.c_void_p, [m.data_ptr() if m is not None else None for m in maps])
        return lib.d2mi_roi_align_bwd2_ex(gp, dims, sc, L, C, mode, pad, assign, min_l, max_l,
                                          canon_s, canon_l, _C.ptr(b0), _C.ptr(i0), R0, oh0, ow0,
                                          sr0, _C.ptr(g0), _C.ptr(b1), _C.ptr(i1), R1, oh1, ow1,
                                          sr1, _C.ptr(g1), acc, phase, lo, hi, _C.ptr(ws), wsb, st)

    ev = KernelTimer.start()
    if not any(defer):
        rc = call(grads, acc_mask, 3, 0, L - 1)
        maps = sum(int(np.prod(s)) for s in shapes) * 4
        # unique-bytes model: both grad_out sets read once + every element of
        # the dense gradient maps written once
        KernelTimer.stop(ev, "roi_align_bwd", d4,
                         extra=lambda: {"unique_bytes": gout_bytes + maps})
        _C.check(rc, "d2mi_roi_align_bwd2")
        return grads
    rc = call(grads, acc_mask, 1, 0, L - 1)
    fresh = [l for l in range(L) if not defer[l]]
    # the prepare launches: the grad_out reads (the contributions' records)
    KernelTimer.stop(ev, "roi_align_bwd", d4, extra=lambda: {"unique_bytes": gout_bytes})
    _C.check(rc, "d2mi_roi_align_bwd2_ex (prepare)")

    def run(level, m, accumulate):
        maps = [None] * L
        maps[level] = m
        ev = KernelTimer.start()
        rc = call(maps, (1 << level) if accumulate else 0, 2, level, level)
        KernelTimer.stop(ev, "roi_align_bwd", 0.0,
                         extra=lambda: {"unique_bytes": touched_bytes([level])})
        _C.check(rc, "d2mi_roi_align_bwd2_ex (pixels)")

    for l in fresh:  # levels without a deferral: their passes now (maps zeroed or given)
        run(l, grads[l], True)
    for l in range(L):
        if defer[l]:
            grads[l] = DeferredPixels(run, l, shapes[l], dev)
    return grads


def roi_align(features, boxes, box_ind, output_size, scales, sampling_ratio=0, aligned=True,
              pad_border=True, assign_levels=True, min_level=None, max_level=None,
              canonical_box_size=224, canonical_level=4, return_levels=False,
              box_mode=None, grad_share=None):
    """Multi-level ROIAlign (poolers.py:134-180 + roi_align.py:45-66 +
    functional.py:100-166) in one launch; output rows in input order.
    grad_share: see _RoIAlignFn (two poolings of one set of maps)."""
    if not isinstance(features, (list, tuple)):
        features = [features]
    L = len(features)
    if min_level is None:
        min_level = int(round(-math.log2(scales[0]))) if L > 1 else 0
        max_level = int(round(-math.log2(scales[-1]))) if L > 1 else 0
    if box_mode is None:
        box_mode = BOX_MODE_ALIGNED if aligned else BOX_MODE_UNALIGNED
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    params = (int(oh), int(ow), tuple(float(s) for s in scales), int(sampling_ratio),
              int(box_mode), int(bool(pad_border)), int(bool(assign_levels and L > 1)),
              int(min_level), int(max_level), int(canonical_box_size), int(canonical_level),
              bool(return_levels))
    out, level = _RoIAlignFn.apply(boxes, box_ind, params, grad_share, *features)
    return (out, level) if return_levels else out
