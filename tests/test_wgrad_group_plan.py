"""The grouped weight-gradient plan (csrc/conv_plan.h: plan_wgrad_group, read
through d2mi_conv2d_wgrad_group_plan without a GPU) and the autograd contract
of the deferral that feeds it (handoff.WgradJoin), on the CPU."""
import contextlib
import random

import pytest
import torch

from detectron2_tensorflow_amd.layers import handoff, ops

# The MFMA-routed weight gradients of the trainable Mask R-CNN R50-FPN backbone
# (res3..res5) at the bench geometry, 2 x 800 x 1344: (N, H, W, Cin, Cout, k,
# stride, pads) and how many convs have the shape (profiles/r6_train_conv_shapes.txt;
# the res5 1x1s and the 1024->512 shortcut run on hipBLASLt).
BACKBONE = [
    ((2, 200, 336, 256, 128, 1, 2, (0, 0)), 1), ((2, 200, 336, 256, 512, 1, 2, (0, 0)), 1),
    ((2, 100, 168, 128, 128, 3, 1, (1, 1)), 4), ((2, 100, 168, 128, 512, 1, 1, (0, 0)), 4),
    ((2, 100, 168, 512, 128, 1, 1, (0, 0)), 3), ((2, 100, 168, 512, 256, 1, 2, (0, 0)), 1),
    ((2, 100, 168, 512, 1024, 1, 2, (0, 0)), 1), ((2, 50, 84, 256, 256, 3, 1, (1, 1)), 6),
    ((2, 50, 84, 256, 1024, 1, 1, (0, 0)), 6), ((2, 50, 84, 1024, 256, 1, 1, (0, 0)), 5),
    ((2, 50, 84, 1024, 2048, 1, 2, (0, 0)), 1), ((2, 25, 42, 512, 512, 3, 1, (1, 1)), 3)]


@contextlib.contextmanager
def mode(value):
    """tuning "wgrad_group": 1 = every problem keeps its own plan's splits (the
    default), 2 = one chunks-per-split per family."""
    old = ops.get_tuning("wgrad_group")
    ops.set_tuning("wgrad_group", value)
    try:
        yield
    finally:
        ops.set_tuning("wgrad_group", old)


def backbone_group():
    return [s for s, k in BACKBONE for _ in range(k)]


def random_group(rng):
    shapes = []
    for _ in range(rng.randint(2, 20)):
        k = rng.choice((1, 1, 3))
        stride = rng.choice((1, 1, 2)) if k == 1 else 1
        shapes.append((rng.randint(1, 3), rng.randint(5, 120), rng.randint(5, 120),
                       4 * rng.randint(1, 160), 4 * rng.randint(1, 160), k, stride,
                       (k // 2, k // 2)))
    return shapes


def groups():
    rng = random.Random(7)
    return [[s for s, _ in BACKBONE], backbone_group()] + [random_group(rng) for _ in range(12)]


def wsize(s):
    return s[5] * s[5] * s[3] * s[4]


def own_plan(s, **kw):
    return ops.wgrad_plan(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], **kw)


def check_layout(shapes, g, common=True):
    assert g["grouped"] == 1
    by_family = {}
    for s, p in zip(shapes, g["problems"]):
        own = own_plan(s)
        # its own tile geometry and kernel; every chunk in exactly one split
        assert (p["kernel"], p["tiles"], p["nchunks"]) == (own["kernel"], own["tiles"], own["nchunks"])
        assert (p["splits"] - 1) * p["chunks_per_split"] < p["nchunks"] <= \
            p["splits"] * p["chunks_per_split"]
        assert p["family"] >= 0
        if common:
            assert p["chunks_per_split"] == \
                g["families"][ops.WGRAD_FAMILIES[p["family"]]]["chunks_per_split"]
        else:  # the splits of its own plan: the single launch's sums
            assert (p["splits"], p["chunks_per_split"]) == (own["splits"], own["chunks_per_split"])
        by_family.setdefault(p["family"], []).append(p)
    # workgroup ranges: disjoint and dense per family
    for f, ps in by_family.items():
        fam = g["families"][ops.WGRAD_FAMILIES[f]]
        at = 0
        for p in sorted(ps, key=lambda p: p["wg0"]):
            assert p["wg0"] == at
            at += p["tiles"] * p["splits"]
        assert at == fam["workgroups"] and len(ps) == fam["problems"]
        assert sum(p["splits"] > 1 for p in ps) == fam["reduce_problems"]
    assert sum(f["problems"] for f in g["families"].values()) == len(shapes)
    # slabs: where there is more than one split, disjoint, 16-B aligned, inside the workspace
    slabs = sorted((p["slab_offset"], p["slab_bytes"]) for p in g["problems"] if p["splits"] > 1)
    end = 0
    for off, nbytes in slabs:
        assert off >= end and off % 16 == 0 and nbytes > 0
        end = off + nbytes
    assert end <= g["workspace_bytes"]
    assert all(p["slab_bytes"] == 0 for p in g["problems"] if p["splits"] == 1)


@pytest.mark.parametrize("gi", range(14))
def test_group_plan_covers_every_chunk_once_in_dense_disjoint_ranges(gi):
    shapes = groups()[gi]
    with mode(2):
        check_layout(shapes, ops.wgrad_group_plan(shapes))
    with mode(1):
        check_layout(shapes, ops.wgrad_group_plan(shapes), common=False)


@pytest.mark.parametrize("gi", range(14))
def test_group_plan_does_not_depend_on_problem_order(gi):
    shapes = groups()[gi]
    perm = list(range(len(shapes)))
    random.Random(gi).shuffle(perm)
    with mode(2):
        g = ops.wgrad_group_plan(shapes)
        h = ops.wgrad_group_plan([shapes[i] for i in perm])
    check_layout([shapes[i] for i in perm], h)
    assert h["families"] == g["families"] and h["workspace_bytes"] == g["workspace_bytes"]
    key = lambda p: tuple(sorted(p.items()))  # noqa: E731
    for s in set(shapes):  # equal shapes may trade places among themselves
        a = sorted(key(g["problems"][i]) for i, t in enumerate(shapes) if t == s)
        b = sorted(key(h["problems"][j]) for j, i in enumerate(perm) if shapes[i] == s)
        assert a == b, s


@pytest.mark.parametrize("gi", (0, 1, 5))
def test_short_or_missing_workspace_gives_the_ungrouped_plans(gi):
    shapes = groups()[gi]
    with mode(2):
        need = ops.wgrad_group_plan(shapes)["workspace_bytes"]
    assert need > 0
    fields = ("kernel", "tiles", "nchunks", "splits", "chunks_per_split")
    for operands, nbytes in ((ops.OP_WORKSPACE | ops.OP_WS_ALIGNED, need - 1), (0, 0),
                             (ops.OP_WORKSPACE, need)):  # short, missing, not 16-B aligned
        with mode(2):
            g = ops.wgrad_group_plan(shapes, operands=operands, workspace_bytes=nbytes)
        assert g["grouped"] == 0 and all(f["problems"] == 0 for f in g["families"].values())
        for s, p in zip(shapes, g["problems"]):
            own = own_plan(s, operands=operands | ops.OP_ALIGNED, workspace_bytes=nbytes)
            assert p["family"] == -1 and [p[f] for f in fields] == [own[f] for f in fields], s


def test_group_of_one_is_the_single_plan_field_by_field():
    for s, _ in BACKBONE + [((1, 9, 11, 256, 128, 3, 1, (1, 1)), 1), ((1, 8, 8, 68, 36, 1, 2, (0, 0)), 1)]:
        own = own_plan(s)
        g = ops.wgrad_group_plan([s], workspace_bytes=own["workspace_bytes"])
        assert g["grouped"] == 0 and g["workspace_bytes"] == own["workspace_bytes"]
        p = g["problems"][0]
        for f in ("kernel", "tiles", "nchunks", "splits", "chunks_per_split"):
            assert p[f] == own[f], (s, f)
        # and its workspace query asks for what the single launch does
        assert ops.wgrad_group_plan([s])["workspace_bytes"] == own["workspace_bytes"]


def test_bench_backbone_group_walks_long_and_writes_few_slabs():
    shapes = backbone_group()
    with mode(2):
        g = ops.wgrad_group_plan(shapes)
    check_layout(shapes, g)
    used = [f for f in g["families"].values() if f["problems"]]
    assert len(used) <= 5 and all(f["chunks_per_split"] >= 64 for f in used), g["families"]
    alone = 0
    for s in shapes:
        own = own_plan(s)
        alone += own["splits"] * (wsize(s) + s[4]) * 4 if own["part"] else 0
    grouped = sum(p["slab_bytes"] for p in g["problems"])
    assert 800e6 < alone < 880e6          # (838 MB of partial slabs per step today)
    assert 4 * grouped <= alone, (grouped, alone)
    assert max(p["splits"] for p in g["problems"]) <= 16


def test_default_mode_keeps_every_problems_own_splits():
    """tuning "wgrad_group" = 1, the default: shared launches, and per problem
    the splits of its own plan -- the sums, and so the bits, of its single launch."""
    assert ops.get_tuning("wgrad_group") == 1
    shapes = backbone_group()
    g = ops.wgrad_group_plan(shapes)
    check_layout(shapes, g, common=False)
    used = {k: f for k, f in g["families"].items() if f["problems"]}
    assert sorted(used) == ["split2x2", "ws", "ws_inc"]
    assert [used[k]["problems"] for k in sorted(used)] == [24, 3, 9]


def test_workspace_query_is_capped_and_a_larger_group_runs_as_single_launches():
    """Under the default every problem's slabs are live at once: the query asks
    for at most 1 GiB, and a group that needs more gets the per-problem plans."""
    s = (2, 50, 84, 256, 256, 3, 1, (1, 1))
    own = own_plan(s)
    per = own["splits"] * (wsize(s) + s[4]) * 4
    assert per > 30e6
    few, many = [s] * 30, [s] * 40
    g = ops.wgrad_group_plan(few)
    assert g["grouped"] == 1 and g["workspace_bytes"] == 30 * per < 2 ** 30
    assert 40 * per > 2 ** 30
    g = ops.wgrad_group_plan(many)
    assert g["grouped"] == 0 and g["workspace_bytes"] == own["workspace_bytes"]
    assert all(p["family"] == -1 and p["splits"] == own["splits"] for p in g["problems"])


# ---- the autograd contract of the deferral, with torch standing in for the kernels
class _Fold(torch.autograd.Function):
    """Two outputs per weight, as _FoldManyFn: (2 * w, 3 * b)."""

    @staticmethod
    def forward(ctx, join, *ts):
        ctx.join = join
        ctx.n = len(ts) // 2
        ctx.set_materialize_grads(False)
        outs = []
        for i in range(ctx.n):
            w_eff, b_eff = 2 * ts[2 * i], 3 * ts[2 * i + 1]
            handoff.tag(w_eff, handoff.FOLD_ENTRY, (join, i))
            outs += [w_eff, b_eff]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        _Fold.calls.append([g is None for g in grads])
        late = {}
        for i, x, gy in ctx.join.take_all():  # the stub: the deferred gradients in torch
            late[i] = (x.t() @ gy, gy.sum(0))
        ret = [None]
        for i in range(ctx.n):
            gw, gb = grads[2 * i], grads[2 * i + 1]
            if i in late:
                assert gw is None and gb is None
                gw, gb = late[i]
            ret += [None if gw is None else 2 * gw, None if gb is None else 3 * gb]
        return tuple(ret)


class _Linear(torch.autograd.Function):
    """x @ w + b whose backward defers the weight and bias gradients."""

    @staticmethod
    def forward(ctx, x, w, b, defer):
        ctx.save_for_backward(x, w)
        ctx.entry = handoff.tagged(w, handoff.FOLD_ENTRY) if defer else None
        return x @ w + b

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        if ctx.entry is not None:
            join, i = ctx.entry
            join.deposit((i, x, gy))
            return gy @ w.t(), None, None, None
        return gy @ w.t(), x.t() @ gy, gy.sum(0), None


def _net(defer):
    torch.manual_seed(3)
    ws = [torch.randn(5, 5, dtype=torch.float64, requires_grad=True) for _ in range(3)]
    bs = [torch.randn(5, dtype=torch.float64, requires_grad=True) for _ in range(3)]
    join = handoff.WgradJoin()
    outs = _Fold.apply(join, *[t for pair in zip(ws, bs) for t in pair])
    x = torch.randn(4, 5, dtype=torch.float64)
    for i in range(3):
        x = _Linear.apply(x, outs[2 * i], outs[2 * i + 1], defer).tanh()
    return ws + bs, x, join, outs


def test_consumers_returning_none_still_get_their_parameters_filled_by_the_join():
    _Fold.calls = []
    params, y, join, _ = _net(defer=True)
    events = []
    handoff.OBSERVER = lambda label, event: events.append(event)
    try:
        y.sum().backward(retain_graph=True)
    finally:
        handoff.OBSERVER = None
    # the fold's backward ran once, after every consumer, with no incoming gradient at all
    assert _Fold.calls == [[True] * 6] and events == ["deposit"] * 3 + ["take"] and join.empty
    got = [p.grad.clone() for p in params]
    ref_params, ref_y, _, _ = _net(defer=False)
    ref_y.sum().backward()
    for g, p in zip(got, ref_params):
        assert torch.equal(g, p.grad)
    # a second backward over the retained graph deposits and joins again
    for p in params:
        p.grad = None
    y.sum().backward()
    assert len(_Fold.calls) == 3 and join.empty
    for p, q in zip(params, ref_params):
        assert torch.equal(p.grad, q.grad)


def test_backward_that_skips_the_join_raises_and_leaves_no_deposit():
    _Fold.calls = []
    params, y, join, outs = _net(defer=True)
    # gradients w.r.t. the folded tensors only: the fold's own backward is not reached
    with pytest.raises(handoff.HandoffError):
        torch.autograd.grad(y.sum(), [outs[1]], retain_graph=True)
    assert join.empty and _Fold.calls == []
    y.sum().backward()  # and a whole backward afterwards starts clean
    assert join.empty and all(p.grad is not None for p in params)
