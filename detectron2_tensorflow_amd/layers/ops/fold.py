"""FrozenBatchNorm folded into the conv weights, one layer or the whole
network at once (csrc/frozen_bn.hip), and the host tables of the batched
fold."""
import numpy as np
import torch

from ... import _C
from ...utils import capture
from .. import handoff
from ._common import _f32c, _HostTable
from .conv import conv2d_wgrad_group


class _FoldFrozenBNFn(torch.autograd.Function):
    """(w_eff, b_eff, packed) = conv weights with a frozen BatchNorm folded in
    (d2mi_fold_frozen_bn); packed is the MFMA layout of w_eff (no gradient)."""

    @staticmethod
    def forward(ctx, w, bias, gamma, beta, mean, var, eps, want_packed):
        _C.require_device(w, mean, var)
        KH, KW, Cin, Cout = w.shape
        w = _f32c(w)
        w_eff = torch.empty_like(w)
        packed = (torch.empty((KH, KW, Cout, Cin), dtype=torch.float32, device=w.device)
                  if want_packed else None)
        b_eff = torch.empty((Cout,), dtype=torch.float32, device=w.device)
        rc = _C.lib().d2mi_fold_frozen_bn(_C.ptr(w), _C.ptr(bias), _C.ptr(gamma), _C.ptr(beta),
                                          _C.ptr(mean), _C.ptr(var), float(eps), KH, KW, Cin,
                                          Cout, _C.ptr(w_eff), _C.ptr(packed), _C.ptr(b_eff),
                                          _C.stream_of(w.device))
        _C.check(rc, "d2mi_fold_frozen_bn")
        ctx.save_for_backward(w, bias, gamma, mean, var)
        # packed never gets a gradient: no zero tensor materialised for it
        ctx.set_materialize_grads(False)
        ctx.eps = float(eps)
        ctx.has = (bias is not None, gamma is not None, beta is not None)
        if packed is not None:
            ctx.mark_non_differentiable(packed)
        return w_eff, b_eff, packed

    @staticmethod
    def backward(ctx, gw_eff, gb_eff, _gpacked):
        w, bias, gamma, mean, var = ctx.saved_tensors
        KH, KW, Cin, Cout = w.shape
        has_bias, has_gamma, has_beta = ctx.has
        need = ctx.needs_input_grad
        dev = w.device
        if gw_eff is None:
            gw_eff = torch.zeros_like(w)
        gw_eff = _f32c(gw_eff)
        gb_eff = _f32c(gb_eff) if gb_eff is not None else None
        mk = lambda cond, shape: torch.empty(shape, dtype=torch.float32, device=dev) if cond else None
        gw = mk(need[0], w.shape)
        gbias = mk(has_bias and need[1], (Cout,))
        ggamma = mk(has_gamma and need[2], (Cout,))
        gbeta = mk(has_beta and need[3], (Cout,))
        wsb = _C.lib().d2mi_fold_frozen_bn_bwd_workspace_size(Cout)
        ws = _C.workspace(wsb, dev)
        rc = _C.lib().d2mi_fold_frozen_bn_bwd(
            _C.ptr(gw_eff), _C.ptr(gb_eff), _C.ptr(w), _C.ptr(bias), _C.ptr(gamma), _C.ptr(mean),
            _C.ptr(var), ctx.eps, KH, KW, Cin, Cout, _C.ptr(gw), _C.ptr(gbias), _C.ptr(ggamma),
            _C.ptr(gbeta), _C.ptr(ws), wsb, _C.stream_of(dev))
        _C.check(rc, "d2mi_fold_frozen_bn_bwd")
        return gw, gbias, ggamma, gbeta, None, None, None, None


def fold_frozen_bn(w_hwio, bias, gamma, beta, mean, var, eps, want_packed=False):
    """Conv weights (HWIO) with a frozen BatchNorm folded in: returns
    (w_eff, b_eff, packed-or-None), differentiable w.r.t. w, bias, gamma, beta."""
    return _FoldFrozenBNFn.apply(w_hwio, bias, gamma, beta, mean, var, float(eps),
                                 bool(want_packed))


_FOLD_DT = np.dtype([(n, np.uint64) for n in (
    "w", "bias", "gamma", "beta", "mean", "var", "w_eff", "w_packed", "b_eff", "gw_eff", "gb_eff",
    "gw", "gbias", "ggamma", "gbeta")] + [("eps", np.float32)] + [(n, np.int32) for n in (
        "taps", "Cin", "Cout", "fwd_begin", "bwd_begin", "co_begin", "pad")] + [
    ("partial_offset", np.int64)])


_fold_tables = {}


def _fold_table(kind, n, device):
    key = (kind, n, device)
    t = _fold_tables.get(key)
    if t is None:
        sz, chunks = _C.ctypes.c_int(), _C.ctypes.c_int()
        _C.lib().d2mi_fold_many_sizes(_C.ctypes.byref(sz), _C.ctypes.byref(chunks))
        if sz.value != _FOLD_DT.itemsize:
            raise RuntimeError("d2mi_fold_entry layout mismatch")
        t = _fold_tables[key] = (_HostTable(n * _FOLD_DT.itemsize, device, f"fold {kind}"),
                                 chunks.value)
    return t


def _addr(t):
    return 0 if t is None else t.data_ptr()


def _sole_owner(t):
    """True when no tensor but ``t`` itself uses t's storage (no live view)."""
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata) <= 2


class _FoldPlan:
    """The forward fold of one set of layers, kept across training steps: the
    parameters are updated in place (same addresses every step), so the
    entry table and the three flat output buffers are reused -- one launch
    over a table already on the device, no host table rebuild or upload --
    whenever none of last step's output views is still alive (the previous
    step's graph is gone)."""

    def __init__(self, flats, tab, fwd, shapes, dev):
        self.flats, self.tab, self.fwd, self.shapes = flats, tab, fwd, shapes
        self.dev_tab = torch.empty(tab.nbytes, dtype=torch.uint8, device=dev)
        self.dev_tab.copy_(torch.from_numpy(tab.view(np.uint8)))

    def reusable(self):
        return all(_sole_owner(f) for f in self.flats)

    def views(self):
        sizes, couts, psz, shapes = self.shapes
        w_effs = self.flats[0].split(sizes)
        b_effs = self.flats[1].split(couts)
        packs = self.flats[2].split(psz)
        outs = []
        for i, (KH, KW, Cin, Cout) in enumerate(shapes):
            outs += [w_effs[i].view(KH, KW, Cin, Cout), b_effs[i],
                     packs[i].view(KH, KW, Cout, Cin) if psz[i] else None]
        return outs


_fold_plans = {}


class _FoldManyFn(torch.autograd.Function):
    """Every BN-conv of the network folded at once: d2mi_fold_frozen_bn_many
    (one launch) forward, d2mi_fold_frozen_bn_bwd_many (two launches)
    backward.  inputs: per entry (w, bias, gamma, beta, mean, var); outputs:
    per entry (w_eff, b_eff, packed-or-None).  Repeated folds of the same
    parameters run from a _FoldPlan.

    Every w_eff carries (a handoff.WgradJoin, its entry index) as its
    FOLD_ENTRY tag: a conv whose weight is that very tensor may leave its
    weight gradient to this node's backward (layers/conv_grad.py), which
    computes every deposited one in one grouped launch per kernel family
    (ops.conv2d_wgrad_group) before the fold adjoint."""

    @staticmethod
    def forward(ctx, spec, *ts):
        n = len(spec)
        dev = ts[0].device
        ctx.join = handoff.WgradJoin()
        key = (spec, dev, tuple(_addr(t) for t in ts), tuple(ts[6 * i].shape for i in range(n)))
        plan = None if capture.capturing() else _fold_plans.get(key)
        if plan is not None and plan.reusable():
            outs = plan.views()
            for i in range(n):
                handoff.tag(outs[3 * i], handoff.FOLD_ENTRY, (ctx.join, i))
                if outs[3 * i + 2] is not None:
                    ctx.mark_non_differentiable(outs[3 * i + 2])
            rc = _C.lib().d2mi_fold_frozen_bn_many(_C.ptr(plan.dev_tab), n, plan.fwd,
                                                   _C.stream_of(dev))
            _C.check(rc, "d2mi_fold_frozen_bn_many")
            ctx.save_for_backward(*ts)
            ctx.tab, ctx.sizes = plan.tab, plan.bwd_sizes
            ctx.set_materialize_grads(False)
            return tuple(outs)
        rows, outs = [], []
        fwd = bwd = cob = part = 0
        table, chunks = _fold_table("fwd", n, dev)
        ws_ = [ts[6 * i] for i in range(n)]
        for w in ws_:
            if not (w.is_contiguous() and w.dtype == torch.float32 and w.device == dev):
                raise ValueError("fold_frozen_bn_many: contiguous f32 weights on one device")
        # the outputs are views of three flat buffers (3 allocations, not 3n)
        sizes = [w.numel() for w in ws_]
        couts = [w.shape[3] for w in ws_]
        flats = (torch.empty(sum(sizes), dtype=torch.float32, device=dev),
                 torch.empty(sum(couts), dtype=torch.float32, device=dev),
                 torch.empty(max(sum(sz if sp[1] else 0 for sz, sp in zip(sizes, spec)), 1),
                             dtype=torch.float32, device=dev))
        w_effs = flats[0].split(sizes)
        b_effs = flats[1].split(couts)
        psz = [sz if sp[1] else 0 for sz, sp in zip(sizes, spec)]
        packs = flats[2].split(psz)
        for i, (eps, want_packed) in enumerate(spec):
            w, bias, gamma, beta, mean, var = ts[6 * i:6 * i + 6]
            KH, KW, Cin, Cout = w.shape
            w_eff = w_effs[i].view(KH, KW, Cin, Cout)
            b_eff = b_effs[i]
            packed = packs[i].view(KH, KW, Cout, Cin) if want_packed else None
            nco, taps = -(-Cout // 64), KH * KW
            rows.append((_addr(w), _addr(bias), _addr(gamma), _addr(beta),
                         _addr(mean), _addr(var), _addr(w_eff), _addr(packed), _addr(b_eff),
                         0, 0, 0, 0, 0, 0, eps, taps, Cin, Cout, fwd, bwd, cob, 0, part))
            fwd += nco * -(-Cin // 64) * taps
            bwd += nco * chunks
            cob += Cout
            part += chunks * Cout
            outs += [w_eff, b_eff, packed]
            handoff.tag(w_eff, handoff.FOLD_ENTRY, (ctx.join, i))
            if packed is not None:
                ctx.mark_non_differentiable(packed)
        tab = np.array(rows, dtype=_FOLD_DT)
        rc = _C.lib().d2mi_fold_frozen_bn_many(_C.ptr(table.upload(tab)), n, fwd,
                                               _C.stream_of(dev))
        _C.check(rc, "d2mi_fold_frozen_bn_many")
        if not capture.capturing():
            if len(_fold_plans) > 4:  # (each holds its outputs: ~0.2 GB for R50)
                _fold_plans.clear()
            plan = _FoldPlan(flats, tab.copy(), fwd,
                             (sizes, couts, psz, [tuple(w.shape) for w in ws_]), dev)
            plan.bwd_sizes = (bwd, cob, part)
            _fold_plans[key] = plan
        ctx.save_for_backward(*ts)
        ctx.tab, ctx.sizes = tab, (bwd, cob, part)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ts = ctx.saved_tensors
        tab = ctx.tab
        n = len(tab)
        need = ctx.needs_input_grad[1:]
        dev = ts[0].device
        bwd, cob, part = ctx.sizes
        ret = [None]
        keep = []
        cols = [[0] * n for _ in range(6)]  # gw_eff gb_eff gw gbias ggamma gbeta
        # the weight gradients the convs left to this backward: one grouped call
        late = {}
        items = ctx.join.take_all()
        if items:
            for (i, *_), g in zip(items, conv2d_wgrad_group([it[1:] for it in items])):
                late.setdefault(i, []).append(g)
        del items
        for i in range(n):
            w, bias, gamma, beta = ts[6 * i:6 * i + 4]
            gw_eff, gb_eff = grads[3 * i], grads[3 * i + 1]
            for dw, db in late.get(i, ()):
                gw_eff = dw if gw_eff is None else gw_eff + dw
                if db is not None:
                    gb_eff = db if gb_eff is None else gb_eff + db
            if gw_eff is not None:
                gw_eff = _f32c(gw_eff)
            if gb_eff is not None:
                gb_eff = _f32c(gb_eff)
            keep += [gw_eff, gb_eff]
            k = 6 * i
            gw = torch.empty_like(w) if need[k] else None
            gbias = torch.empty_like(bias) if need[k + 1] and bias is not None else None
            ggamma = torch.empty_like(gamma) if need[k + 2] and gamma is not None else None
            gbeta = torch.empty_like(beta) if need[k + 3] and beta is not None else None
            for c, t in enumerate((gw_eff, gb_eff, gw, gbias, ggamma, gbeta)):
                if t is not None:
                    cols[c][i] = t.data_ptr()
            ret += [gw, gbias, ggamma, gbeta, None, None]
        for c, name in enumerate(("gw_eff", "gb_eff", "gw", "gbias", "ggamma", "gbeta")):
            tab[name] = cols[c]
        table, _ = _fold_table("bwd", n, dev)
        ws = _C.scratch(part * 4, dev)
        rc = _C.lib().d2mi_fold_frozen_bn_bwd_many(_C.ptr(table.upload(tab)), n, bwd, cob,
                                                   _C.ptr(ws), _C.stream_of(dev))
        _C.check(rc, "d2mi_fold_frozen_bn_bwd_many")
        del keep
        return tuple(ret)


def fold_frozen_bn_many(entries):
    """entries: [(w_hwio, bias, gamma, beta, mean, var, eps, want_packed)] ->
    [(w_eff, b_eff, packed-or-None)], the batched fold_frozen_bn (bit-identical
    results, differentiable w.r.t. each w, bias, gamma, beta)."""
    if not entries:
        return []
    spec = tuple((float(e[6]), bool(e[7])) for e in entries)
    ts = []
    for e in entries:
        _C.require_device(e[0], e[4], e[5])
        ts += [_f32c(e[0])] + [None if t is None else _f32c(t) for t in e[1:4]] + [
            _f32c(e[4]), _f32c(e[5])]
    outs = _FoldManyFn.apply(spec, *ts)
    return [tuple(outs[3 * i:3 * i + 3]) for i in range(len(entries))]
