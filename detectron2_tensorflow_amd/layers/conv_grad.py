"""The MFMA conv as an autograd op, ``conv_mfma``, and the routing of its
backward: dgrad on the same MFMA kernel (flipped kernel); wgrad on the MFMA
wgrad kernel or hipBLASLt / MIOpen, whichever measured faster for the shape
(see _wgrad); stride-2 KxK dgrad and Cout % 4 != 0 use torch.nn.grad.
"""
import contextlib

import torch
import torch.nn.functional as F

from . import handoff, ops


def _dgrad(gy, w, x_shape, stride, pb, pe, relu_gate=None, add=None, add2=None, census=None):
    """Input gradient (+ add, then the relu_gate mask, when given).  census: an
    ops.RowCensus of gy (a declared handoff.RowBound) for the stride-1 MFMA
    path, which then computes only the rows near a non-zero gy row.  Stride 1:
    a forward conv of gy with the spatially flipped kernel — whose HWIO layout IS the packed [KH, KW, out', in'] layout
    of the transposed conv, flipped by the kernel's tap indexing (kFlipTaps) —
    on the MFMA kernel, padded (KH-1-pb, KH-1-pe).
    1x1 stride s: the MFMA GEMM gy . W^T on the strided grid, scattered into
    zeros.  Anything else: torch.nn.grad (MIOpen)."""
    KH, KW, Cin, Cout = w.shape
    gy = gy.contiguous()
    if add2 is not None:  # (dgrad + add) + add2, gated: the strided 1x1 scatter only
        if not (KH == 1 and KW == 1 and pb == 0 and pe == 0 and stride > 1 and Cin % 4 == 0
                and Cout % 4 == 0):
            gx = _dgrad(gy, w, x_shape, stride, pb, pe, add=add).add_(add2)
            return gx if relu_gate is None else torch.ops.aten.threshold_backward(gx, relu_gate, 0.0)
        g = ops.conv2d_nhwc(gy, w.detach().contiguous(), None, 1, (0, 0))
        return ops.stride_scatter(g, x_shape, stride, add, add2, relu_gate)
    if KH == KW and Cout % 4 == 0:
        if stride == 1 and max(pb, pe) <= KH - 1:
            # the flip is an index flip inside the kernel (no flipped copy)
            return ops.conv2d_nhwc(gy, w.detach().contiguous(), None, 1,
                                   (KH - 1 - pb, KH - 1 - pe), flip_taps=KH > 1,
                                   residual=add, relu_gate=relu_gate, census=census)
        if KH == 1 and pb == 0 and pe == 0:
            g = ops.conv2d_nhwc(gy, w.detach().contiguous(), None, 1, (0, 0))
            if Cin % 4 == 0:  # zero holes + scatter (+ add) (+ gate) in one pass
                return ops.stride_scatter(g, x_shape, stride, add, gate=relu_gate)
            gx = torch.zeros(x_shape, dtype=gy.dtype, device=gy.device)
            gx[:, ::stride, ::stride] = g
            gx = gx if add is None else gx.add_(add)
            return gx if relu_gate is None else torch.ops.aten.threshold_backward(gx, relu_gate, 0.0)
    if relu_gate is not None:
        raise ValueError("relu_gate is fused into the stride-1 MFMA dgrad / the 1x1 scatter only")
    xin_shape = (x_shape[0], x_shape[3], x_shape[1] + pb + pe, x_shape[2] + pb + pe)
    gx = torch.nn.grad.conv2d_input(xin_shape, w.permute(3, 2, 0, 1), gy.permute(0, 3, 1, 2),
                                    stride, 0)
    gx = gx[:, :, pb:gx.shape[2] - pe, pb:gx.shape[3] - pe].permute(0, 2, 3, 1)
    return gx if add is None else gx + add


_WGRAD_1X1_MIN_P = 8192


def _wgrad(x, gy, w_shape, stride, pb, pe, want_bias=False, accumulate_into=None, census=None):
    """(weight gradient HWIO, bias gradient or None).

    census: an ops.RowCensus of gy's pixel rows (a declared handoff.RowBound),
    or None: the MFMA wgrad of a KxK conv then walks only the 32-pixel chunks
    that hold a non-zero row (bit-identical); every other path ignores it.

    accumulate_into: (gw, gb) of earlier calls of the same shared weight
    (gb None without a bias): this call's gradient is added into them --
    inside the MFMA wgrad's reduce pass where it runs, else by an in-place
    add -- and the accumulators are returned (gb None when this path made
    no bias gradient: the caller adds its column sum).

    Routed by measurement (tools/bench_kernels.py --only wgrad, MI355X):
    with split products (the default, ops.conv.CONV_MATH) every KxK and every 1x1
    over >= 8k output pixels runs on the MFMA wgrad kernel (bias gradient
    fused; FPN p2 3x3 154 TF/s vs MIOpen's 122, mask-head 3x3 147 vs 110);
    smaller 1x1 -> X^T . dY as one hipBLASLt GEMM.  With f32 products the
    KxK go to MIOpen's igemm wrw, which beats the f32 MFMA kernel there."""
    KH, KW, Cin, Cout = w_shape
    acc_w, acc_b = accumulate_into if accumulate_into is not None else (None, None)

    def added(gw):  # a path without the fused accumulate
        return (gw if acc_w is None else acc_w.add_(gw)), None

    route = _mfma_wgrad_route(x, gy, w_shape, stride, pb, pe)
    if route is not None:
        k, pads = route
        if want_bias and (acc_w is None or acc_b is not None):
            acc = (acc_w, acc_b) if acc_w is not None else None
            return ops.conv2d_wgrad(x, gy, k, stride, pads, with_bias=True, accumulate_into=acc,
                                    census=census)
        return ops.conv2d_wgrad(x, gy, k, stride, pads, accumulate_into=acc_w, census=census), None
    if KH == 1 and KW == 1 and pb == 0 and pe == 0:
        xs = x if stride == 1 else x[:, ::stride, ::stride]
        xs = xs.reshape(-1, Cin)
        return added(torch.mm(xs.t(), gy.reshape(-1, Cout)).reshape(1, 1, Cin, Cout))
    xin = F.pad(x, (0, 0, pb, pe, pb, pe)) if (pb or pe) else x
    gw = torch.nn.grad.conv2d_weight(xin.permute(0, 3, 1, 2), (Cout, Cin, KH, KW),
                                     gy.permute(0, 3, 1, 2), stride, 0)
    return added(gw.permute(2, 3, 1, 0))


def _mfma_wgrad_route(x, gy, w_shape, stride, pb, pe):
    """(kernel size, pads) of the ops.conv2d_wgrad call _wgrad makes for this
    shape, or None where it routes to hipBLASLt / MIOpen."""
    KH, KW, Cin, Cout = w_shape
    eligible = Cin % 4 == 0 and Cout % 4 == 0
    if KH == 1 and KW == 1 and pb == 0 and pe == 0:
        P = gy.numel() // Cout
        # tools/exp_wgrad_1x1.py: MFMA from 8400 pixels (res4: 54 vs 64-79 us
        # on hipBLASLt), and the strided 1024->2048 at 2100; hipBLASLt below
        if eligible and (P >= _WGRAD_1X1_MIN_P or (stride > 1 and Cin * Cout >= 2 ** 21)):
            return 1, (0, 0)
        return None
    if (ops.conv.CONV_MATH == "split" and eligible and KH == KW
            and 6 * max(x.numel(), gy.numel()) < 2 ** 31):
        return KH, (pb, pe)
    return None


# A side stream while the graphed training step captures its backward
# (engine/graphed.py, under wgrad_on): every MFMA conv's weight gradient is
# issued there, beside its data gradient, so the replayed graph runs the two
# concurrently (a replayed graph runs forked branches in parallel,
# tools/graph_parallel_probe.py).  None in eager steps: a per-layer stream
# fork costs host time there (r2 measured +3.7 %), and a replay pays none.
_wgrad_stream = None


@contextlib.contextmanager
def wgrad_on(stream):
    """Every conv_mfma backward inside issues its weight gradient on ``stream``."""
    global _wgrad_stream
    _wgrad_stream = stream
    try:
        yield
    finally:
        _wgrad_stream = None


def _gate_eligible(w_shape, stride, pb, pe):
    KH, KW, _, Cout = w_shape
    return KH == KW and Cout % 4 == 0 and stride == 1 and max(pb, pe) <= KH - 1


# ---- the steps of _ConvMFMAFn.backward, in the order it takes them
def _relu_masked(ctx, gy, y):
    """gy under the output ReLU's mask, unless its sole consumer applied it."""
    if ctx.out_tag is not None and ctx.out_tag.masked:
        return gy
    # relu is the last op whenever an add is fused (relu_after)
    return torch.ops.aten.threshold_backward(gy, y, 0.0)


def _topdown_grad(ctx, gy):
    """The gradient of the fused + up2(topdown): gy summed over 2x2 blocks."""
    if gy.shape[-1] % 4 == 0:
        gtd = ops.upsample2x_grad(gy)
    else:
        N, OH, OW, C = gy.shape
        g = F.pad(gy, (0, 0, 0, OW % 2, 0, OH % 2))
        gtd = g.reshape(N, (OH + 1) // 2, 2, (OW + 1) // 2, 2, C).sum((2, 4))
    links = ctx.links
    if links is not None and links.td_pair is not None and ctx.needs_input_grad[7]:
        # the merged map's other reader is its output conv: first of the
        # two leaves its gradient, the second adds it (the output conv in
        # its dgrad epilogue) -- autograd's sum of the two, no add launch
        gtd = links.td_pair.meet_topdown(gtd)
    return gtd


def _residual_grad(ctx, gy):
    """gy itself: to autograd, or to the conv reading the residual (res_grad_to)."""
    links = ctx.links
    if ctx.needs_input_grad[8] and links is not None and links.res_grad_to is not None:
        links.res_grad_to.put(gy)  # taken by the conv reading it
        return None
    return gy if ctx.needs_input_grad[8] else None


def _row_census(links):
    """gy's row census where a row bound was declared (handoff.RowBound; None: dense)."""
    rows = links.rows if links is not None else None
    return rows[0].take(rows[1]) if rows is not None else None


def input_grad(links, gate_ok, dgrad):
    """The input gradient of one conv call.  ``links`` (a handoff.Links or
    None) says what rides on the one data-gradient launch, dgrad(gate, add,
    add2) -> gx, and what becomes of its result (Links.plan); gate_ok: that
    launch can apply the input's ReLU mask (_gate_eligible)."""
    if links is None:
        return dgrad(False, None, None)
    plan = links.plan(gate_ok)
    return plan.finish(dgrad(plan.gate, plan.add, plan.add2))


def _defer_weight_grad(ctx, x, gy, w, stride, pb, pe, want_b, census):
    """Leave this call's weight (and bias) gradient to the backward of the
    batched fold whose output the weight is (handoff.WgradJoin): True when
    deposited -- the MFMA route of _wgrad, no census, accumulator or side
    stream, tuning "wgrad_group" on."""
    entry = ctx.fold_entry
    if (entry is None or not ctx.needs_input_grad[1] or census is not None
            or _wgrad_stream is not None or not gy.is_cuda
            or (ctx.links is not None and ctx.links.wacc is not None)
            or ops.get_tuning("wgrad_group") <= 0):
        return False
    route = _mfma_wgrad_route(x, gy, w.shape, stride, pb, pe)
    if route is None:
        return False
    join, index = entry
    join.deposit((index, x, gy, route[0], stride, route[1], want_b))
    return True


def _weight_grad(ctx, x, gy, w, stride, pb, pe, want_b, census, side=None):
    """(weight, bias) gradient, None where not needed.  side: issued on that
    stream (wgrad_on) BEFORE the data gradient, so that the two run
    concurrently; _join_weight_grad follows the data gradient."""
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(gy.device))
        if census is not None:  # (made on this stream, read on the side one)
            census.ws.record_stream(side)
        with torch.cuda.stream(side):
            return _weight_grad(ctx, x, gy, w, stride, pb, pe, want_b, census)

    def step(buf):  # (buf: the sums of a shared weight's earlier calls, or None)
        gw = gb = None
        if ctx.needs_input_grad[1]:
            gw, gb = _wgrad(x, gy, w.shape, stride, pb, pe, want_b, accumulate_into=buf,
                            census=census)
        if want_b and gb is None:
            cs = ops.column_sum(gy)
            gb = cs if buf is None or buf[1] is None else buf[1].add_(cs)
        return gw, gb

    # a weight shared by several calls of one forward (a handoff.LevelAccumulator:
    # the RPN head's 3x3 over the FPN levels): the reduce pass adds each call's
    # gradient in (old + new, autograd's order); only the last returns the sums
    wacc = ctx.links.wacc if ctx.links is not None else None
    if ctx.needs_input_grad[1] and wacc is not None:
        return wacc.accumulate(step) or (None, None)
    return step(None)


def _join_weight_grad(side, gw, gb):
    main = torch.cuda.current_stream(side.device)
    main.wait_stream(side)
    for t in (gw, gb):  # (made on the side stream, used on this one)
        if t is not None:
            t.record_stream(main)


class _ConvMFMAFn(torch.autograd.Function):
    """The MFMA conv with its fused epilogue (bias, ReLU, top-down / residual
    add).  ``links`` (a handoff.Links or None) holds this call's ends of the
    gradient hand-offs of the training graph -- the sole-consumer ReLU gate,
    the residual link, the pair, the join, the level accumulator: see
    layers/handoff.py.  The backward asks it what to do with the input
    gradient (input_grad) and makes one _dgrad call from the answer."""

    @staticmethod
    def forward(ctx, x, w_hwio, bias, w_packed, stride, pads, relu, topdown=None, residual=None,
                relu_after=False, links=None):
        has_add = topdown is not None or residual is not None
        if relu and has_add and not relu_after:
            raise ValueError("relu(conv) + add is not differentiable here; use relu_after_add")
        y = ops.conv2d_nhwc(x, w_packed, bias, stride, pads, relu, topdown, residual,
                            relu_after_add=relu_after)
        ctx.save_for_backward(x, w_hwio, y if relu else None)
        ctx.conf = (stride, pads, relu, bias is not None, topdown is not None, residual is not None)
        ctx.links = links
        # the weight is a batched fold's own output (no view, pad or cast in
        # between): its gradient may wait for that fold's backward
        ctx.fold_entry = handoff.tagged(w_hwio, handoff.FOLD_ENTRY)
        if links is not None:
            links.bind(x, topdown, residual is not None)
        ctx.out_tag = None
        if relu:  # (forward runs with grad mode off: tag unconditionally)
            ctx.out_tag = handoff.ReluTag()
            handoff.tag(y, handoff.RELU, ctx.out_tag)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        stride, (pb, pe), relu, has_bias, has_td, has_res = ctx.conf
        links = ctx.links
        if relu:
            gy = _relu_masked(ctx, gy, y)
        gtd = _topdown_grad(ctx, gy) if has_td else None
        gres = _residual_grad(ctx, gy) if has_res else None
        census = _row_census(links)
        wg = (ctx, x, gy, w, stride, pb, pe, has_bias and ctx.needs_input_grad[2], census)
        side = _wgrad_stream
        forked = side is not None and ctx.needs_input_grad[1] and gy.is_cuda
        deferred = _defer_weight_grad(*wg)
        if deferred:
            gw = gb = None
        elif forked:
            gw, gb = _weight_grad(*wg, side)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = input_grad(links, links is not None and _gate_eligible(w.shape, stride, pb, pe),
                            lambda gate, add, add2: _dgrad(
                                gy, w, x.shape, stride, pb, pe, relu_gate=x if gate else None,
                                add=add, add2=add2, census=census))
        if forked and not deferred:
            _join_weight_grad(side, gw, gb)
        elif not deferred:
            gw, gb = _weight_grad(*wg)
        return gx, gw, gb, None, None, None, None, gtd, gres, None, None


def conv_mfma(x, w_hwio, bias, w_packed, stride, pads, relu, topdown=None, residual=None,
              relu_after=False, links=None):
    """_ConvMFMAFn.apply with keywords (Function.apply takes none)."""
    return _ConvMFMAFn.apply(x, w_hwio, bias, w_packed, stride, pads, relu, topdown, residual,
                             relu_after, links)


