"""The conv family: weight packing, the MFMA implicit-GEMM conv and its
multi-level and row-list forms, the row census, the weight gradients and the
planner queries (csrc/conv_mfma.hip, conv_rows.hip, conv_wgrad.hip,
wgrad_skinny.hip), the stem (stem.hip) and the FPN / strided-conv adjoints
(resample_grad.hip).  Owns the CONV_MATH toggle: readers and writers use
ops.conv.CONV_MATH."""
import os

import numpy as np
import torch

from ... import _C
from ._common import _CONV_WS, _WGRAD_WS, _f32c, _HostTable
from .timing import KernelTimer, bound_of, conv_bytes


def pack_conv_weights(w_hwio):
    """HWIO -> [KH, KW, Cout, Cin] for d2mi_conv2d_nhwc."""
    w = _f32c(w_hwio)
    _C.require_device(w)
    KH, KW, Cin, Cout = w.shape
    out = torch.empty((KH, KW, Cout, Cin), dtype=torch.float32, device=w.device)
    rc = _C.lib().d2mi_conv_pack_weights(_C.ptr(w), KH, KW, Cin, Cout, _C.ptr(out),
                                         _C.stream_of(w.device))
    _C.check(rc, "d2mi_conv_pack_weights")
    return out


def pack_conv_weights_many(ws):
    """pack_conv_weights of every HWIO tensor in ``ws`` (d2mi_conv_pack_weights_many:
    one launch for all Cin % 64 == 0 tensors); bit-identical copies."""
    ws = [_f32c(w) for w in ws]
    if not ws:
        return []
    _C.require_device(*ws)
    outs = [torch.empty((w.shape[0], w.shape[1], w.shape[3], w.shape[2]), dtype=torch.float32,
                        device=w.device) for w in ws]
    wp = _C.host_array(_C.c_void_p, [w.data_ptr() for w in ws])
    op = _C.host_array(_C.c_void_p, [o.data_ptr() for o in outs])
    dims = _C.host_array(_C.ctypes.c_int32, [int(v) for w in ws for v in w.shape])
    rc = _C.lib().d2mi_conv_pack_weights_many(len(ws), wp, dims, op, _C.stream_of(ws[0].device))
    _C.check(rc, "d2mi_conv_pack_weights_many")
    return outs


# Conv MFMA product form: "f32" = v_mfma_f32_32x32x2_f32 (exact f32 products);
# "split" = the same f32 operands split exactly into three bf16 terms
# (h + m + l == x) and multiplied with six v_mfma_f32_32x32x16_bf16 products
# (f32-class error, see csrc/conv_mfma.hip), split while the kernel stages
# its tiles.  Process-wide default from D2MI_CONV_MATH.
CONV_MATH = os.environ.get("D2MI_CONV_MATH", "split")


def split_bf16x3(x):
    """f32 tensor -> int16 [3, *x.shape]: bf16 bit patterns of the exact split
    x = h + m + l (truncation; csrc/conv_mfma.hip split3)."""
    x = _f32c(x)
    _C.require_device(x)
    if x.numel() % 4:
        raise ValueError("split_bf16x3: numel must be a multiple of 4")
    out = torch.empty((3,) + tuple(x.shape), dtype=torch.int16, device=x.device)
    rc = _C.lib().d2mi_split_bf16x3(_C.ptr(x), x.numel(), _C.ptr(out), _C.stream_of(x.device))
    _C.check(rc, "d2mi_split_bf16x3")
    return out


def conv2d_nhwc(x, w_packed, bias=None, stride=1, pad=(0, 0), relu=False, topdown=None,
                residual=None, relu_after_add=False, math_mode=None, flip_taps=False,
                relu_gate=None, out=None, census=None):
    """MFMA implicit-GEMM conv: x [N,H,W,Cin], w_packed [KH,KW,Cout,Cin].
    census: a RowCensus of x's pixel rows whose list was dilated by this
    conv's window (a stride-1 same-size dgrad of a sparse gradient, no bias /
    relu / top-down): d2mi_conv2d_nhwc_rows computes the listed output rows
    only and fills the rest with the epilogue of zero -- bit-identical; timed
    as "conv2d_rows" when the row-list launch ran.
    relu_after_add: relu(conv + bias + residual/topdown) instead of
    relu(conv + bias) + residual/topdown.  math_mode: "f32" | "split" (None:
    CONV_MATH).  flip_taps: use the spatially flipped kernel (w_packed[KH-1-i, KW-1-j]).
    relu_gate: a ReLU output of the result's shape: out = gate > 0 ? conv
    (+ residual) : 0 (a dgrad with its producer's ReLU backward fused, and the
    gradient of the producer's other consumer added first)."""
    math_mode = math_mode or CONV_MATH
    if math_mode not in ("f32", "split"):
        raise ValueError(f"conv math must be 'f32' or 'split', got {math_mode!r}")
    x = _f32c(x)
    _C.require_device(x, w_packed)
    N, H, W, Cin = x.shape
    KH, KW, Cout, Cin2 = w_packed.shape
    if Cin != Cin2:
        raise ValueError(f"conv input has {Cin} channels, weights expect {Cin2}")
    pb, pe = pad
    OH = (H + pb + pe - KH) // stride + 1
    OW = (W + pb + pe - KW) // stride + 1
    if out is not None:
        if (tuple(out.shape) != (N, OH, OW, Cout) or out.dtype != torch.float32
                or not out.is_contiguous() or out.device != x.device):
            raise ValueError(f"out must be a contiguous f32 {(N, OH, OW, Cout)} tensor on {x.device}")
        y = out
    else:
        y = torch.empty((N, OH, OW, Cout), dtype=torch.float32, device=x.device)
    if topdown is not None:
        topdown = _f32c(topdown)
        if topdown.shape != (N, (OH + 1) // 2, (OW + 1) // 2, Cout):
            raise ValueError(f"top-down map {tuple(topdown.shape)} does not upsample to "
                             f"{(N, OH, OW, Cout)}")
    if residual is not None:
        residual = _f32c(residual)
    if relu_gate is not None:
        if topdown is not None or relu:
            raise ValueError("relu_gate excludes topdown / relu")
        relu_gate = _f32c(relu_gate)
        if relu_gate.shape != y.shape:
            raise ValueError(f"relu_gate {tuple(relu_gate.shape)} != output {tuple(y.shape)}")
    if residual is not None and residual.shape != y.shape:
        raise ValueError(f"residual {tuple(residual.shape)} != output {tuple(y.shape)}")
    flags = (1 if relu else 0) | (2 if relu_after_add else 0) | (8 if flip_taps else 0)
    if math_mode == "split":
        flags |= 4
    lib = _C.lib()
    wkey = (N, H, W, Cin, Cout, KH, KW, stride, pb, pe)
    wsb = _CONV_WS.get(wkey)
    if wsb is None:
        wsb = _CONV_WS[wkey] = lib.d2mi_conv2d_workspace_size(N, H, W, Cin, Cout, KH, KW,
                                                              int(stride), int(pb), int(pe))
    ws = _C.scratch(wsb, x.device) if wsb else None
    st = _C.stream_of(x.device)
    if (census is not None and census.dilate is not None and bias is None and topdown is None
            and not relu and math_mode == "split" and census.shape == (N, H, W)):
        ev = KernelTimer.start()
        rc = lib.d2mi_conv2d_nhwc_rows(_C.ptr(x), _C.ptr(w_packed), _C.ptr(residual),
                                       _C.ptr(relu_gate), _C.ptr(y), N, H, W, Cin, Cout, KH, KW,
                                       int(stride), int(pb), int(pe), flags, _C.ptr(census.ws),
                                       census.ws.numel(), census.capacity, census.dilate[0],
                                       census.dilate[1], _C.ptr(ws), wsb, st)
        if rc == 1:  # the row-list launch ran: not a dense launch (its own timing name)
            KernelTimer.stop(ev, "conv2d_rows", 0.0)
            if KernelTimer.detail and ev is not None:
                KernelTimer.stop(ev, f"conv_rows {N}x{H}x{W}x{Cin}->{Cout} k{KH} s{stride}", 0.0)
            census.used()
            return y
        rc = min(rc, 0)
    elif relu_gate is not None:
        ev = KernelTimer.start()
        rc = lib.d2mi_conv2d_nhwc_gated(_C.ptr(x), _C.ptr(w_packed), _C.ptr(bias),
                                        _C.ptr(residual), _C.ptr(relu_gate), _C.ptr(y), N,
                                        H, W, Cin, Cout, KH, KW, int(stride), int(pb),
                                        int(pe), flags, _C.ptr(ws), wsb, st)
    else:
        ev = KernelTimer.start()
        rc = lib.d2mi_conv2d_nhwc_ex(_C.ptr(x), _C.ptr(w_packed), _C.ptr(bias),
                                     _C.ptr(topdown), _C.ptr(residual), _C.ptr(y), N, H, W,
                                     Cin, Cout, KH, KW, int(stride), int(pb), int(pe), flags,
                                     _C.ptr(ws), wsb, st)
    fl = 2.0 * N * OH * OW * Cout * KH * KW * Cin
    group = "conv2d_split" if math_mode == "split" else "conv2d_mfma"
    KernelTimer.stop(ev, group, fl)
    if ev is not None:
        # the launch's own roofline: its least HBM traffic (every operand read
        # once, the output written once) against its flops, classified at the
        # split ridge (416.7 TF/s / 8 TB/s = 52 flop/B) -- verdict r4: the
        # short-K 1x1s are memory-bound launches, not low-MFMA ones
        byts = conv_bytes(x, w_packed, y, bias, topdown, residual, relu_gate)
        KernelTimer.stop(ev, f"{group}_{bound_of(fl, byts, math_mode)}_bound", fl,
                         extra=lambda: {"bytes": byts})
    if KernelTimer.detail and ev is not None:
        tag = ("g" if relu_gate is not None else "") + ("r" if residual is not None else "") + (
            "f" if flip_taps else "")
        KernelTimer.stop(ev, f"conv {N}x{H}x{W}x{Cin}->{Cout} k{KH} s{stride} p{pb}{pe} {tag}", fl,
                         extra=lambda: {"bytes": byts})
    _C.check(rc, "d2mi_conv2d_nhwc")
    return y


def conv2d_nhwc_levels(xs, w_packed, bias=None, stride=1, pad=(0, 0), relu=False, math_mode=None):
    """One launch of the same conv over up to 6 feature levels (a head shared
    across FPN levels: RetinaNet / SOLOv2 towers): xs[l] [N_l, H_l, W_l, Cin]
    -> [N_l, OH_l, OW_l, Cout] each (d2mi_conv2d_nhwc_levels).  Every level's
    tiles run in one grid, so the small levels neither serialise behind the
    big one nor need split-K; per-tile arithmetic is conv2d_nhwc's."""
    math_mode = math_mode or CONV_MATH
    if math_mode not in ("f32", "split"):
        raise ValueError(f"conv math must be 'f32' or 'split', got {math_mode!r}")
    xs = [_f32c(x) for x in xs]
    _C.require_device(w_packed, *xs)
    if not 1 <= len(xs) <= 6:
        raise ValueError(f"conv2d_nhwc_levels takes 1..6 levels, got {len(xs)}")
    KH, KW, Cout, Cin = w_packed.shape
    pb, pe = pad
    ys, dims = [], []
    for x in xs:
        N, H, W, C = x.shape
        if C != Cin:
            raise ValueError(f"conv input has {C} channels, weights expect {Cin}")
        OH = (H + pb + pe - KH) // stride + 1
        OW = (W + pb + pe - KW) // stride + 1
        ys.append(torch.empty((N, OH, OW, Cout), dtype=torch.float32, device=x.device))
        dims += [N, H, W]
    flags = (1 if relu else 0) | (4 if math_mode == "split" else 0)
    xp = _C.host_array(_C.c_void_p, [x.data_ptr() for x in xs])
    yp = _C.host_array(_C.c_void_p, [y.data_ptr() for y in ys])
    dm = _C.host_array(_C.ctypes.c_int32, dims)
    lib = _C.lib()
    wsb = lib.d2mi_conv2d_levels_workspace_size(dm, len(xs), Cin, Cout, KH, KW, int(stride),
                                                int(pb), int(pe))
    ws = _C.scratch(wsb, xs[0].device) if wsb else None
    ev = KernelTimer.start()
    rc = lib.d2mi_conv2d_nhwc_levels(xp, dm, len(xs), _C.ptr(w_packed), _C.ptr(bias), yp, Cin,
                                     Cout, KH, KW, int(stride), int(pb), int(pe), flags,
                                     _C.ptr(ws), wsb, _C.stream_of(xs[0].device))
    fl = sum(2.0 * y.shape[0] * y.shape[1] * y.shape[2] * Cout * KH * KW * Cin for y in ys)
    KernelTimer.stop(ev, "conv2d_split" if math_mode == "split" else "conv2d_mfma", fl)
    _C.check(rc, "d2mi_conv2d_nhwc_levels")
    return ys


class RowCensus:
    """The row census of a sparse gradient map [N, H, W, C] (d2mi_row_census):
    its device workspace ``ws`` and, for tests and tools, views of its parts.
    ``dilate``: (k, pad) of the stride-1 conv window its row list was dilated
    by, or None (no list).  ``owner``: an object whose ``sparse_launches``
    counts the launches that used this census (a handoff.RowBound), or None."""
    __slots__ = ("ws", "shape", "capacity", "dilate", "owner", "_layout")

    def __init__(self, ws, shape, capacity, dilate=None, owner=None):
        self.ws, self.shape, self.capacity = ws, tuple(shape), int(capacity)
        self.dilate, self.owner = dilate, owner
        self._layout = None

    def _parts(self):
        if self._layout is None:
            out = (_C.ctypes.c_int64 * 7)()
            k = self.dilate[0] if self.dilate else 0
            _C.check(_C.lib().d2mi_row_census_layout(*self.shape, self.capacity, k, out, 7),
                     "d2mi_row_census_layout")
            self._layout = tuple(out)
        return self._layout

    def _i32(self, off, n):
        return self.ws[off:off + 4 * n].view(torch.int32)

    @property
    def bitmap(self):
        """int32 [words]: bit c % 32 of word c // 32 = chunk c holds a non-zero row."""
        return self._i32(self._parts()[0], self._parts()[1])

    @property
    def count(self):
        """int32 [1]: the number of non-zero rows."""
        return self._i32(self._parts()[3], 1)

    @property
    def list_capacity(self):
        return self._parts()[6]

    @property
    def nrows(self):
        """int32 [1]: the number of listed (dilated) rows, clamped to list_capacity."""
        return self._i32(self._parts()[4], 1)

    @property
    def rows(self):
        """int32 [list_capacity]: the listed rows, ascending (the first nrows are valid)."""
        return self._i32(self._parts()[5], self._parts()[6])

    def used(self):
        if self.owner is not None:
            self.owner.sparse_launches += 1


_CENSUS_WS = {}


def row_census_workspace_size(N, H, W, capacity=0, dilate_k=0):
    key = (int(N), int(H), int(W), int(capacity), int(dilate_k))
    n = _CENSUS_WS.get(key)
    if n is None:
        n = _CENSUS_WS[key] = _C.lib().d2mi_row_census_workspace_size(*key)
    return n


def row_census(g, capacity, dilate=None, owner=None):
    """RowCensus of g [N, H, W, C] (C % 4 == 0): which 32-pixel chunks hold a
    non-zero row, how many rows are non-zero (more than ``capacity`` sets the
    device error word: a declared bound was false) and, with dilate = (k, pad),
    the sorted list of the output rows of a k x k stride-1 conv over g (pad
    leading zeros) whose window holds a non-zero row.  The census owns its
    workspace: it lives until its last reader has run."""
    g = _f32c(g)
    _C.require_device(g)
    N, H, W, C = g.shape
    k, pad = (int(dilate[0]), int(dilate[1])) if dilate else (0, 0)
    nbytes = row_census_workspace_size(N, H, W, capacity, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
    ev = KernelTimer.start()
    rc = _C.lib().d2mi_row_census(_C.ptr(g), N, H, W, C, int(capacity), k, pad, _C.ptr(ws), nbytes,
                                  _C.stream_of(g.device))
    KernelTimer.stop(ev, "row_census", 4.0 * g.numel())
    _C.check(rc, "d2mi_row_census")
    return RowCensus(ws, (N, H, W), capacity, (k, pad) if k else None, owner)


def conv2d_wgrad(x, dy, kernel_size, stride=1, pad=(0, 0), with_bias=False, math_mode=None,
                 accumulate_into=None, census=None):
    """HWIO weight gradient of conv2d_nhwc on the MFMA wgrad kernel; with_bias
    also returns the bias gradient (dy summed over pixels) from the same pass.
    math_mode: "f32" | "split" (None: CONV_MATH), as conv2d_nhwc.
    accumulate_into: the (dw, db) -- or dw -- of an earlier call to add this
    one's gradient into (d2mi_conv2d_wgrad_ex bit 3: old + new in the reduce
    pass, autograd's order for a weight shared by several calls).
    census: a RowCensus of dy's pixel rows (or of a superset of its non-zero
    rows): d2mi_conv2d_wgrad_rows walks only the set chunks -- the same plan,
    bit-identical for finite x; timed as "conv2d_wgrad_rows" when the bitmap
    kernel ran (the plan's other kernels run dense and are timed as such)."""
    math_mode = math_mode or CONV_MATH
    if math_mode not in ("f32", "split"):
        raise ValueError(f"conv math must be 'f32' or 'split', got {math_mode!r}")
    x, dy = _f32c(x), _f32c(dy)
    _C.require_device(x, dy)
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    if census is not None and census.shape != tuple(dy.shape[:3]):
        raise ValueError(f"row census of {census.shape} pixels for a gradient of {tuple(dy.shape[:3])}")
    KH = KW = int(kernel_size)
    pb, pe = pad
    if accumulate_into is not None:
        dw, db = accumulate_into if with_bias else (accumulate_into, None)
        if (dw.shape != (KH, KW, Cin, Cout) or dw.dtype != torch.float32
                or not dw.is_contiguous() or (with_bias and (db is None or db.shape != (Cout,)))):
            raise ValueError("accumulate_into must be the (dw, db) of a wgrad of this shape")
    else:
        dw = torch.empty((KH, KW, Cin, Cout), dtype=torch.float32, device=x.device)
        db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if with_bias else None
    args = (N, H, W, Cin, Cout, KH, KW, int(stride), int(pb), int(pe))
    wsb = _WGRAD_WS.get(args)
    if wsb is None:
        wsb = _WGRAD_WS[args] = _C.lib().d2mi_conv2d_wgrad_workspace_size(*args)
    if accumulate_into is not None:  # (the reduce pass adds: one slab at least)
        wsb = max(wsb, (KH * KW * Cin * Cout + Cout) * 4)
    ws = _C.scratch(wsb, x.device) if wsb else None
    ev = KernelTimer.start()
    flags = (4 if math_mode == "split" else 0) | (8 if accumulate_into is not None else 0)
    if census is not None:
        rc = _C.lib().d2mi_conv2d_wgrad_rows(_C.ptr(x), _C.ptr(dy), _C.ptr(dw), _C.ptr(db), *args,
                                             flags, _C.ptr(census.ws), census.ws.numel(),
                                             _C.ptr(ws), wsb, _C.stream_of(x.device))
        if rc == 1:  # the bitmap kernel ran: not a dense launch (its own timing name)
            KernelTimer.stop(ev, "conv2d_wgrad_rows", 0.0)
            if KernelTimer.detail and ev is not None:
                KernelTimer.stop(ev, f"wgrad_rows {N}x{H}x{W}x{Cin}->{Cout} k{KH} s{stride}", 0.0)
            census.used()
            return (dw, db) if with_bias else dw
        rc = min(rc, 0)
    else:
        rc = _C.lib().d2mi_conv2d_wgrad_ex(_C.ptr(x), _C.ptr(dy), _C.ptr(dw), _C.ptr(db), *args,
                                           flags, _C.ptr(ws), wsb, _C.stream_of(x.device))
    fl = 2.0 * dy.numel() * KH * KW * Cin
    group = "conv2d_wgrad_split" if flags & 4 else "conv2d_wgrad_mfma"
    KernelTimer.stop(ev, group, fl)
    if ev is not None:
        # x and dy read once, dw (+ db) written once (+ read when accumulating)
        byts = 4.0 * (x.numel() + dy.numel() + dw.numel() * (2 if accumulate_into is not None else 1)
                      + (Cout if with_bias else 0))
        KernelTimer.stop(ev, f"{group}_{bound_of(fl, byts, math_mode)}_bound", fl,
                         extra=lambda: {"bytes": byts})
    if KernelTimer.detail and ev is not None:
        KernelTimer.stop(ev, f"wgrad {N}x{H}x{W}x{Cin}->{Cout} k{KH} s{stride}", fl,
                         extra=lambda: {"bytes": byts})
    _C.check(rc, "d2mi_conv2d_wgrad")
    return (dw, db) if with_bias else dw


_WGRAD_PROBLEM_DT = np.dtype([(n, np.uint64) for n in ("x", "dy", "dw", "dbias")] + [
    (n, np.int32) for n in ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad_beg",
                            "pad_end")])
WGRAD_GROUP_MAX = 64
_wgrad_group_tables = {}


def _wgrad_problems(shapes, ptrs=None):
    """The host array of d2mi_conv2d_wgrad_group: shapes [(N, H, W, Cin, Cout, k,
    stride, (pb, pe))], ptrs [(x, dy, dw, dbias)] device addresses (None: zeros)."""
    tab = np.zeros(len(shapes), dtype=_WGRAD_PROBLEM_DT)
    for i, (N, H, W, Cin, Cout, k, stride, (pb, pe)) in enumerate(shapes):
        tab[i] = (ptrs[i] if ptrs else (0, 0, 0, 0)) + (N, H, W, Cin, Cout, k, k, stride, pb, pe)
    return tab


def conv2d_wgrad_group(problems, math_mode=None, out=None):
    """conv2d_wgrad of many problems -- [(x, dy, kernel_size, stride, (pb, pe),
    with_bias)] -> [(dw, db-or-None)] -- in one launch per kernel family and
    one reduce per family (d2mi_conv2d_wgrad_group).  Tuning "wgrad_group" 1
    (default): every problem keeps its own plan's pixel splits -- the bits of
    conv2d_wgrad; 2: one chunks-per-split per family (few slabs, long walks,
    sums in another order).  A group of one is conv2d_wgrad itself.  out: the dw tensors to
    write (contiguous f32 HWIO, 4-byte aligned at least: gradient-bucket views)."""
    math_mode = math_mode or CONV_MATH
    if math_mode not in ("f32", "split"):
        raise ValueError(f"conv math must be 'f32' or 'split', got {math_mode!r}")
    if not problems:
        return []
    outs = []
    for at in range(0, len(problems), WGRAD_GROUP_MAX):
        outs += _wgrad_group(problems[at:at + WGRAD_GROUP_MAX], math_mode,
                             None if out is None else list(out[at:at + WGRAD_GROUP_MAX]))
    return outs


def _wgrad_group(problems, math_mode, dws=None):
    n = len(problems)
    if n == 1 and dws is None:
        x, dy, k, stride, pad, with_bias = problems[0]
        r = conv2d_wgrad(x, dy, k, stride, pad, with_bias=with_bias, math_mode=math_mode)
        return [r if with_bias else (r, None)]
    xs = [_f32c(p[0]) for p in problems]
    dys = [_f32c(p[1]) for p in problems]
    _C.require_device(*xs, *dys)
    dev = xs[0].device
    shapes = []
    for x, dy, p in zip(xs, dys, problems):
        N, H, W, Cin = x.shape
        shapes.append((N, H, W, Cin, dy.shape[-1], int(p[2]), int(p[3]),
                       (int(p[4][0]), int(p[4][1]))))
    sizes = [s[5] * s[5] * s[3] * s[4] for s in shapes]
    couts = [s[4] if p[5] else 0 for s, p in zip(shapes, problems)]
    if dws is None:  # one allocation for the gradients (every size is a multiple of 4 floats)
        flat = torch.empty(sum(sizes) + sum(couts), dtype=torch.float32, device=dev)
        parts = flat.split(sizes + couts)
        dws = [parts[i].view(s[5], s[5], s[3], s[4]) for i, s in enumerate(shapes)]
        dbs = [parts[n + i] if couts[i] else None for i in range(n)]
    else:
        for dw, s in zip(dws, shapes):
            if (tuple(dw.shape) != (s[5], s[5], s[3], s[4]) or dw.dtype != torch.float32
                    or not dw.is_contiguous() or dw.device != dev):
                raise ValueError("conv2d_wgrad_group: out must be contiguous f32 HWIO tensors")
        dbs = [torch.empty((c,), dtype=torch.float32, device=dev) if c else None for c in couts]
    flags = 4 if math_mode == "split" else 0
    tab = _wgrad_problems(shapes, [(x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                                    0 if db is None else db.data_ptr())
                                   for x, dy, dw, db in zip(xs, dys, dws, dbs)])
    lib = _C.lib()
    # (asked every call: the group's plan moves with the wgrad_* tuning knobs)
    # (a group without slabs still needs a workspace to be planned as a group)
    wsb = max(lib.d2mi_conv2d_wgrad_group_workspace_size(tab.ctypes.data, n, flags), 256)
    ws = _C.scratch(wsb, dev)
    tkey = (n, dev)
    table = _wgrad_group_tables.get(tkey)
    if table is None:
        table = _wgrad_group_tables[tkey] = _HostTable(
            lib.d2mi_conv2d_wgrad_group_table_size(n), dev, "wgrad group")
    host = np.empty(table.dev.numel(), dtype=np.uint8)
    rc = lib.d2mi_conv2d_wgrad_group_table(tab.ctypes.data, n, flags, _C.ptr(ws), wsb,
                                           host.ctypes.data, host.size)
    _C.check(rc, "d2mi_conv2d_wgrad_group_table")
    dev_tab = table.upload(host)
    ev = KernelTimer.start()
    rc = lib.d2mi_conv2d_wgrad_group(tab.ctypes.data, n, flags, _C.ptr(dev_tab), host.size,
                                     _C.ptr(ws), wsb, _C.stream_of(dev))
    fl = sum(2.0 * dy.numel() * s[5] * s[5] * s[3] for dy, s in zip(dys, shapes))
    group = "conv2d_wgrad_split" if flags & 4 else "conv2d_wgrad_mfma"
    KernelTimer.stop(ev, group, fl)
    if ev is not None:
        byts = 4.0 * (sum(x.numel() + dy.numel() for x, dy in zip(xs, dys)) + sum(sizes)
                      + sum(couts))
        KernelTimer.stop(ev, f"{group}_{bound_of(fl, byts, math_mode)}_bound", fl,
                         extra=lambda: {"bytes": byts})
        if KernelTimer.detail:
            KernelTimer.stop(ev, f"wgrad_group[{n}] " + " ".join(sorted(
                {f"{s[3]}->{s[4]}k{s[5]}s{s[6]}" for s in shapes})), fl,
                extra=lambda: {"bytes": byts})
    _C.check(rc, "d2mi_conv2d_wgrad_group")
    return list(zip(dws, dbs))


# ------------------------------------------------------------- plan queries
# The launch plans of the three conv families as dicts (d2mi_conv2d_plan and
# its kin, include/d2mi.h: the planner the launchers run; no GPU needed).
# operands: the OP_* facts about a launch's pointers; workspace_bytes None =
# the shape's own *_workspace_size.
OP_TOPDOWN, OP_RESIDUAL, OP_GATE, OP_ALIGNED, OP_BIAS_ALIGNED, OP_WORKSPACE, OP_WS_ALIGNED = (
    1, 2, 4, 8, 16, 32, 64)
OP_ALL_ALIGNED = OP_ALIGNED | OP_BIAS_ALIGNED | OP_WS_ALIGNED
CONV_FAMILIES = ("tiled128x128", "tiled128x64", "tiled128x32", "ws256x128", "stream1x1")
WGRAD_KERNELS = ("f32", "split", "split_occ3", "ws", "ws_inc")
_LAUNCH_FIELDS = ("tile0", "tiles", "splits", "kt_per_split", "m_base", "m_end", "reduce",
                  "reduce_grid")
CONV_PLAN_FIELDS = (("family", "occ", "split3", "lds_epi", "M", "BM", "BN", "nM", "nN", "nk")
                    + tuple("main_" + f for f in _LAUNCH_FIELDS)
                    + tuple("tail_" + f for f in _LAUNCH_FIELDS)
                    + ("stream_kmax", "stream_tn", "stream_form", "stream_nslices", "stream_grid"))
LEVELS_PLAN_FIELDS = ("family", "occ", "split3", "lds_epi", "BM", "BN", "nN", "nk", "tiles",
                      "splits", "kt_per_split", "reduce_grid", "nlev")
WGRAD_PLAN_FIELDS = ("kernel", "TM", "TN", "BM", "BN", "nCi", "nCo", "tiles", "nchunks", "splits",
                     "chunks_per_split", "part", "reduce", "reduce_grid")


def _plan_query(fn, name, args, flags, operands, workspace_bytes, n):
    out = (_C.ctypes.c_int32 * n)()
    rc = fn(*args, int(flags), int(operands), int(workspace_bytes), out, n)
    _C.check(min(rc, 0), name)
    v = list(out)
    return v[:-2], v[-2] | (v[-1] << 31)


def conv_plan(N, H, W, Cin, Cout, k, stride=1, pad=(0, 0), flags=4,
              operands=OP_ALL_ALIGNED | OP_WORKSPACE, workspace_bytes=None):
    """The plan of conv2d_nhwc for a shape (flags: d2mi_conv2d_nhwc_ex's, 4 = split math)."""
    args = (N, H, W, Cin, Cout, k, k, int(stride), int(pad[0]), int(pad[1]))
    lib = _C.lib()
    if workspace_bytes is None:
        workspace_bytes = lib.d2mi_conv2d_workspace_size(*args)
    v, wsb = _plan_query(lib.d2mi_conv2d_plan, "d2mi_conv2d_plan", args, flags, operands,
                         workspace_bytes, len(CONV_PLAN_FIELDS) + 2)
    return dict(zip(CONV_PLAN_FIELDS, v), workspace_bytes=wsb)


def conv_levels_plan(dims, Cin, Cout, k, stride=1, pad=(0, 0), flags=4,
                     operands=OP_ALL_ALIGNED | OP_WORKSPACE, workspace_bytes=None):
    """The plan of conv2d_nhwc_levels; dims: (N, H, W) per level."""
    dm = _C.host_array(_C.ctypes.c_int32, [int(d) for lv in dims for d in lv])
    args = (dm, len(dims), Cin, Cout, k, k, int(stride), int(pad[0]), int(pad[1]))
    lib = _C.lib()
    if workspace_bytes is None:
        workspace_bytes = lib.d2mi_conv2d_levels_workspace_size(*args)
    v, wsb = _plan_query(lib.d2mi_conv2d_levels_plan, "d2mi_conv2d_levels_plan", args, flags,
                         operands, workspace_bytes, len(LEVELS_PLAN_FIELDS) + 16)
    n = len(LEVELS_PLAN_FIELDS)
    return dict(zip(LEVELS_PLAN_FIELDS, v), tile0=v[n:n + 7], moff=v[n + 7:n + 14],
                workspace_bytes=wsb)


def wgrad_plan(N, H, W, Cin, Cout, k, stride=1, pad=(0, 0), flags=4,
               operands=OP_ALL_ALIGNED | OP_WORKSPACE, workspace_bytes=None):
    """The plan of conv2d_wgrad (flags: d2mi_conv2d_wgrad_ex's, 4 = split math, 8 = accumulate)."""
    args = (N, H, W, Cin, Cout, k, k, int(stride), int(pad[0]), int(pad[1]))
    lib = _C.lib()
    if workspace_bytes is None:
        workspace_bytes = lib.d2mi_conv2d_wgrad_workspace_size(*args)
    v, wsb = _plan_query(lib.d2mi_conv2d_wgrad_plan, "d2mi_conv2d_wgrad_plan", args, flags,
                         operands, workspace_bytes, len(WGRAD_PLAN_FIELDS) + 2)
    return dict(zip(WGRAD_PLAN_FIELDS, v), workspace_bytes=wsb)


WGRAD_FAMILIES = ("ws", "ws_inc", "split2x2", "split2x1", "split1x2", "split1x1", "split2x2_occ3")
WGRAD_GROUP_FAMILY_FIELDS = ("problems", "workgroups", "chunks_per_split", "reduce_problems",
                             "reduce_grid")
WGRAD_GROUP_PROBLEM_FIELDS = ("family", "kernel", "tiles", "nchunks", "splits", "chunks_per_split",
                              "wg0")


def wgrad_group_plan(shapes, flags=4, operands=OP_WORKSPACE | OP_WS_ALIGNED, workspace_bytes=None):
    """The plan of conv2d_wgrad_group (no GPU needed); shapes: [(N, H, W, Cin,
    Cout, k, stride, (pb, pe))].  {"grouped", "families": {name: {...}},
    "problems": [{..., "slab_offset" (bytes), "slab_bytes"}], "workspace_bytes"}."""
    tab = _wgrad_problems(shapes)
    n = len(shapes)
    lib = _C.lib()
    if workspace_bytes is None:
        workspace_bytes = lib.d2mi_conv2d_wgrad_group_workspace_size(tab.ctypes.data, n, flags)
    nf, npf = len(WGRAD_FAMILIES), len(WGRAD_GROUP_PROBLEM_FIELDS)
    m = 2 + 6 * nf + (npf + 2) * n + 2
    out = (_C.ctypes.c_int32 * m)()
    rc = lib.d2mi_conv2d_wgrad_group_plan(tab.ctypes.data, n, int(flags), int(operands),
                                          int(workspace_bytes), out, m)
    _C.check(min(rc, 0), "d2mi_conv2d_wgrad_group_plan")
    v = list(out)
    fams = {name: dict(zip(WGRAD_GROUP_FAMILY_FIELDS, v[2 + 6 * f:8 + 6 * f]))
            for f, name in enumerate(WGRAD_FAMILIES)}
    probs = []
    for i, s in enumerate(shapes):
        pv = v[2 + 6 * nf + (npf + 2) * i:][:npf + 2]
        d = dict(zip(WGRAD_GROUP_PROBLEM_FIELDS, pv))
        d["slab_offset"] = pv[npf] | (pv[npf + 1] << 31)
        d["slab_bytes"] = (d["splits"] * (s[5] * s[5] * s[3] * s[4] + s[4]) * 4
                           if v[0] and d["splits"] > 1 else 0)
        probs.append(d)
    return {"grouped": v[0], "families": fams, "problems": probs,
            "workspace_bytes": v[-2] | (v[-1] << 31)}


def stem_conv_weights(w):
    """HWIO [7, 7, 3, Cout=64] -> the [3][64][160] bf16 planes d2mi_stem_conv
    takes (K = (kh * 7 + kw) * 3 + c, zero-padded to 160)."""
    if tuple(w.shape) != (7, 7, 3, 64):
        raise ValueError(f"stem conv weights must be [7, 7, 3, 64], got {tuple(w.shape)}")
    wt = torch.zeros((64, 160), dtype=torch.float32, device=w.device)
    wt[:, :147] = _f32c(w).reshape(147, 64).t()
    return split_bf16x3(wt.contiguous())


def stem_conv(x, w3):
    """d2mi_stem_conv: the 7x7 / stride-2 stem conv (Cin 3 -> 64, pad 3) on
    the split-bf16 MFMA; x [N, H, W, 3] NHWC, w3 from stem_conv_weights.
    Raw sums (the folded shift is stem_pool's); no gradient."""
    x = _f32c(x)
    _C.require_device(x, w3)
    N, H, W, C = x.shape
    if C != 3:
        raise ValueError(f"stem conv takes 3 input channels, got {C}")
    y = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), dtype=torch.float32,
                    device=x.device)
    rc = _C.lib().d2mi_stem_conv(_C.ptr(x), _C.ptr(w3), N, H, W, _C.ptr(y),
                                 _C.stream_of(x.device))
    _C.check(rc, "d2mi_stem_conv")
    return y


def preprocess_images(x, mean, std, flip, size_divisibility=0):
    """d2mi_preprocess_images: (x - mean) / std, the BGR channel flip and the
    zero pad to size_divisibility in one pass (rcnn.py:146-157 +
    image_list.py:89-100); x [N, H, W, 3] NHWC f32 -> [N, Hp, Wp, 3]."""
    x = _f32c(x)
    mean, std = _f32c(mean), _f32c(std)
    _C.require_device(x, mean, std)
    N, H, W, C = x.shape
    if C != 3 or mean.numel() != 3 or std.numel() != 3:
        raise ValueError(f"preprocess takes 3 channels and 3 means / stds, got {tuple(x.shape)}")
    s = int(size_divisibility)
    Hp, Wp = (H + (-H) % s, W + (-W) % s) if s > 0 else (H, W)
    out = torch.empty((N, Hp, Wp, 3), dtype=torch.float32, device=x.device)
    rc = _C.lib().d2mi_preprocess_images(_C.ptr(x), _C.ptr(mean), _C.ptr(std), N, H, W, Hp, Wp,
                                         int(bool(flip)), _C.ptr(out), _C.stream_of(x.device))
    _C.check(rc, "d2mi_preprocess_images")
    return out


def stem_pool(y, shift=None):
    """relu(y + shift) -> zero pad 1 -> 3x3 / 2 VALID max pool, NHWC
    (d2mi_stem_pool): the ResNet stem tail in one pass (no gradient)."""
    y = _f32c(y)
    shift = _f32c(shift) if shift is not None else None
    _C.require_device(y)
    N, H, W, C = y.shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32,
                      device=y.device)
    rc = _C.lib().d2mi_stem_pool(_C.ptr(y), _C.ptr(shift), N, H, W, C, _C.ptr(out),
                                 _C.stream_of(y.device))
    _C.check(rc, "d2mi_stem_pool")
    return out


def upsample2x_grad(gy):
    """Adjoint of the FPN top-down nearest 2x upsample (d2mi_upsample2x_grad):
    gy [N, OH, OW, C] -> [N, ceil(OH/2), ceil(OW/2), C]."""
    gy = _f32c(gy)
    _C.require_device(gy)
    N, OH, OW, C = gy.shape
    out = torch.empty((N, (OH + 1) // 2, (OW + 1) // 2, C), dtype=torch.float32, device=gy.device)
    rc = _C.lib().d2mi_upsample2x_grad(_C.ptr(gy), N, OH, OW, C, _C.ptr(out),
                                       _C.stream_of(gy.device))
    _C.check(rc, "d2mi_upsample2x_grad")
    return out


def stride_scatter(g, out_shape, stride, add=None, add2=None, gate=None):
    """Input gradient of a 1x1 stride-s conv from its GEMM on the strided grid
    (d2mi_stride_scatter_ex): zeros off the grid, + add, + add2 (nullable, in
    that order), then zeroed where gate <= 0 (gate nullable: the ReLU backward
    of the ReLU output ``gate``)."""
    g = _f32c(g)
    add = _f32c(add) if add is not None else None
    add2 = _f32c(add2) if add2 is not None else None
    gate = _f32c(gate) if gate is not None else None
    _C.require_device(g)
    N, H, W, C = out_shape
    if g.shape != (N, (H - 1) // stride + 1, (W - 1) // stride + 1, C):
        raise ValueError(f"stride_scatter: {tuple(g.shape)} is not the stride-{stride} grid of "
                         f"{tuple(out_shape)}")
    for t in (add, add2, gate):
        if t is not None and tuple(t.shape) != tuple(out_shape):
            raise ValueError(f"stride_scatter: operand {tuple(t.shape)} != {tuple(out_shape)}")
    out = torch.empty(tuple(out_shape), dtype=torch.float32, device=g.device)
    rc = _C.lib().d2mi_stride_scatter_ex(_C.ptr(g), _C.ptr(add), _C.ptr(add2), _C.ptr(gate), N, H,
                                         W, C, int(stride), _C.ptr(out), _C.stream_of(g.device))
    _C.check(rc, "d2mi_stride_scatter_ex")
    return out


def wgrad_skinny(x, g, with_bias=True, accumulate_into=None):
    """1x1-conv weight (+ bias) gradient for Cout <= 80 over all pixels (one
    streaming pass over x per 16 output columns: one for the 3-anchor RPN head's
    16, five for the 15-anchor head's 76):
    x [..., Cin], g [..., Cout] -> (gw [1, 1, Cin, Cout] HWIO, gb [Cout] or None).
    accumulate_into: a (gw, gb) pair of an earlier call to add this one into
    (old + new, in place; returned)."""
    x, g = _f32c(x), _f32c(g)
    _C.require_device(x, g)
    Cin, Cout = x.shape[-1], g.shape[-1]
    P = x.numel() // Cin
    if g.numel() != P * Cout:
        raise ValueError(f"wgrad_skinny: {tuple(x.shape)} vs {tuple(g.shape)}")
    if accumulate_into is not None:
        gw, gb = accumulate_into
        if (tuple(gw.shape) != (1, 1, Cin, Cout) or not gw.is_contiguous()
                or (gb is None) == with_bias):
            raise ValueError("wgrad_skinny: accumulate_into does not match this gradient")
    else:
        gw = torch.empty((1, 1, Cin, Cout), dtype=torch.float32, device=x.device)
        gb = torch.empty((Cout,), dtype=torch.float32, device=x.device) if with_bias else None
    wsb = _C.lib().d2mi_wgrad_skinny_workspace_size(P, Cin, Cout)
    ws = _C.workspace(wsb, x.device)
    ev = KernelTimer.start()
    rc = _C.lib().d2mi_wgrad_skinny_ex(_C.ptr(x), _C.ptr(g), P, Cin, Cout, _C.ptr(gw), _C.ptr(gb),
                                       int(accumulate_into is not None), _C.ptr(ws), wsb,
                                       _C.stream_of(x.device))
    # algorithmic bytes: x and g read once
    KernelTimer.stop(ev, "wgrad_skinny", 4 * P * (Cin + Cout))
    _C.check(rc, "d2mi_wgrad_skinny")
    return gw, gb


def wgrad_skinny_levels(xs, gs, with_bias=True):
    """wgrad_skinny of several calls sharing one weight, summed in list order
    (d2mi_wgrad_skinny_levels: one partial launch + one reduce; bit-identical
    to the calls one by one with accumulate_into after the first).  xs[l]
    [..., Cin] 16-B aligned with Cin % 4 == 0, gs[l] [..., Cout], Cout <= 80."""
    xs = [_f32c(x) for x in xs]
    gs = [_f32c(g) for g in gs]
    _C.require_device(*xs, *gs)
    Cin, Cout = xs[0].shape[-1], gs[0].shape[-1]
    Ps = [x.numel() // Cin for x in xs]
    for x, g, P in zip(xs, gs, Ps):
        if x.shape[-1] != Cin or g.numel() != P * Cout:
            raise ValueError(f"wgrad_skinny_levels: {tuple(x.shape)} vs {tuple(g.shape)}")
    dev = xs[0].device
    gw = torch.empty((1, 1, Cin, Cout), dtype=torch.float32, device=dev)
    gb = torch.empty((Cout,), dtype=torch.float32, device=dev) if with_bias else None
    Pa = _C.host_array(_C.ctypes.c_int32, Ps)
    lib = _C.lib()
    wsb = lib.d2mi_wgrad_skinny_levels_workspace_size(Pa, len(xs), Cin, Cout)
    ws = _C.scratch(wsb, dev)
    ev = KernelTimer.start()
    rc = lib.d2mi_wgrad_skinny_levels(_C.host_array(_C.c_void_p, [x.data_ptr() for x in xs]),
                                      _C.host_array(_C.c_void_p, [g.data_ptr() for g in gs]), Pa,
                                      len(xs), Cin, Cout, _C.ptr(gw), _C.ptr(gb), 0, _C.ptr(ws),
                                      wsb, _C.stream_of(dev))
    KernelTimer.stop(ev, "wgrad_skinny", 4 * sum(Ps) * (Cin + Cout))
    _C.check(rc, "d2mi_wgrad_skinny_levels")
    return gw, gb


def skinny_levels_ok(x):
    """Whether a level's input can join wgrad_skinny_levels."""
    return x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 4 == 0 \
        and x.data_ptr() % 16 == 0


def column_sum(x):
    """Sum over every leading dim of x [..., C] -> [C] (fixed order)."""
    x = _f32c(x)
    _C.require_device(x)
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty((C,), dtype=torch.float32, device=x.device)
    wsb = _C.lib().d2mi_column_sum_workspace_size(rows, C)
    ws = _C.workspace(wsb, x.device)
    rc = _C.lib().d2mi_column_sum(_C.ptr(x), rows, C, _C.ptr(out), _C.ptr(ws), wsb,
                                  _C.stream_of(x.device))
    _C.check(rc, "d2mi_column_sum")
    return out
