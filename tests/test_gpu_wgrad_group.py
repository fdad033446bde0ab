"""Grouped weight gradients on the GPU (ops.conv2d_wgrad_group,
d2mi_conv2d_wgrad_group): every kernel family's grouped launch and reduce
against float64, and the deferral of a folded ResNet stage's weight gradients
to the fold's backward (layers/conv_grad.py, layers/ops/fold.py).

Bars, as tests/test_gpu_conv_arms.py's weight gradients: small-integer operands
are exact in any summation order (torch.equal to float64); randn operands at
rtol 1e-4, atol 2e-5 max|want| for dw and atol 1e-3 for db."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu


def ops():
    from detectron2_tensorflow_amd.layers import ops as o
    return o


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda", 0)


@contextlib.contextmanager
def knobs(**kv):
    o = ops()
    old = {k: o.get_tuning(k) for k in kv}
    try:
        for k, v in kv.items():
            o.set_tuning(k, v)
        yield
    finally:
        for k, v in old.items():
            o.set_tuning(k, v)


# several pixel splits even at these sizes: one chunk per split allowed, and a
# slot target small enough that a family's summed tiles can take more than one
# round (the plan then weighs rounds against chunks per split); wgrad_group 2:
# one chunks-per-split per family, so the splits are not those of the single
# launches (OWN: the default, every problem with its own plan's splits)
SPLITS = dict(wgrad_minch=1, wgrad_slots=64, wgrad_group=2)
OWN = dict(wgrad_minch=1, wgrad_slots=64, wgrad_group=1)

# (N, H, W, Cin, Cout, k, stride); with_bias on the odd-numbered ones
PROBLEMS = [
    (1, 9, 11, 256, 128, 3, 1),  # ws_inc: 99 pixels, a ragged last chunk
    (2, 6, 7, 256, 256, 3, 1),   # ws_inc: an image boundary inside a chunk, 2 co tiles
    (1, 5, 3, 256, 128, 3, 1),   # ws: OW < 4, the non-incremental cursor
    (1, 7, 9, 64, 64, 1, 1),     # split 1x1
    (2, 5, 6, 128, 192, 3, 1),   # split 2x2: a partial co tile
    (1, 8, 8, 68, 36, 1, 2),     # split 2x1, stride 2: partial tiles both ways
]
FAMILY = ["ws_inc", "ws_inc", "ws", "split1x1", "split2x2", "split2x1"]
GROUPS = {
    "alone0": [0], "alone1": [1], "alone2": [2], "alone3": [3], "alone4": [4], "alone5": [5],
    "ws_inc": [0, 1], "ws": [2, 2], "split": [3, 4, 5], "all": [0, 1, 2, 3, 4, 5],
    # repeated shapes; the one-chunk 5x3 map gets one split, the others several
    "seven": [0, 2, 4, 0, 5, 2, 1],
}

_data = {}


def data(i, kind):
    """Operands and float64 reference of PROBLEMS[i], made once and shared."""
    if (i, kind) not in _data:
        N, H, W, Cin, Cout, k, s = PROBLEMS[i]
        p = (k - 1) // 2
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        g = torch.Generator().manual_seed(100 + 2 * i + (kind == "int"))
        if kind == "int":
            x = torch.randint(-4, 5, (N, H, W, Cin), generator=g).float()
            dy = torch.randint(-4, 5, (N, OH, OW, Cout), generator=g).float()
        else:
            x = torch.randn(N, H, W, Cin, generator=g)
            dy = torch.randn(N, OH, OW, Cout, generator=g)
        dw = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Cout, Cin, k, k),
                                         dy.double().permute(0, 3, 1, 2), s, p).permute(2, 3, 1, 0)
        _data[(i, kind)] = (x, dy, dw.contiguous(), dy.double().sum((0, 1, 2)))
    return _data[(i, kind)]


def problem(i, kind, dev):
    N, H, W, Cin, Cout, k, s = PROBLEMS[i]
    x, dy, _, _ = data(i, kind)
    p = (k - 1) // 2
    return (x.to(dev), dy.to(dev), k, s, (p, p), i % 2 == 1)


def shape_of(i):
    N, H, W, Cin, Cout, k, s = PROBLEMS[i]
    p = (k - 1) // 2
    return (N, H, W, Cin, Cout, k, s, (p, p))


def run(idx, kind, dev, **kw):
    return ops().conv2d_wgrad_group([problem(i, kind, dev) for i in idx], **kw)


def test_the_problems_cover_the_families_and_split():
    """What the cases claim about the plan, asked of the planner."""
    o = ops()
    with knobs(**SPLITS):
        for i, fam in enumerate(FAMILY):
            g = o.wgrad_group_plan([shape_of(i), shape_of(i)])
            assert g["grouped"] == 1 and o.WGRAD_FAMILIES[g["problems"][0]["family"]] == fam, i
        g = o.wgrad_group_plan([shape_of(i) for i in GROUPS["seven"]])
        splits = [p["splits"] for p in g["problems"]]
        assert min(splits) == 1 and max(splits) > 1 and sum(s > 1 for s in splits) >= 3, splits
        # (the second 2x6x7 map of three chunks: one split beside two of the 9x11's)
        assert g["problems"][6]["nchunks"] == 3 and splits[6] == 1 and splits[0] == 2
        g = o.wgrad_group_plan([shape_of(i) for i in GROUPS["all"]])
        assert all(p["splits"] > 1 for p in g["problems"] if p["nchunks"] > 1)
        assert [p["nchunks"] for p in g["problems"]] == [4, 3, 1, 2, 2, 1]


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_is_exact_on_integers_and_repeatable(dev, name):
    idx = GROUPS[name]
    with knobs(**SPLITS):
        got = run(idx, "int", dev)
        again = run(idx, "int", dev)
    for i, (dw, db), (dw2, db2) in zip(idx, got, again):
        _, _, want_w, want_b = data(i, "int")
        assert torch.equal(dw.cpu().double(), want_w), (name, i)
        assert torch.equal(dw, dw2)
        assert (db is None) == (i % 2 == 0)
        if db is not None:
            assert torch.equal(db.cpu().double(), want_b) and torch.equal(db, db2), (name, i)


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_random_data_at_the_wgrad_bars(dev, name):
    idx = GROUPS[name]
    with knobs(**SPLITS):
        got = run(idx, "rand", dev)
        again = run(idx, "rand", dev)
    for i, (dw, db), (dw2, db2) in zip(idx, got, again):
        _, _, want_w, want_b = data(i, "rand")
        scale = float(want_w.abs().max())
        torch.testing.assert_close(dw.cpu().double(), want_w, rtol=1e-4, atol=2e-5 * scale,
                                   msg=lambda m: f"{name} problem {i}: {m}")
        assert torch.equal(dw, dw2)
        if db is not None:
            torch.testing.assert_close(db.cpu().double(), want_b, rtol=1e-4, atol=1e-3)
            assert torch.equal(db, db2)


@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_group_of_one_is_the_single_launch(dev, i):
    for kv in (SPLITS, {}):
        with knobs(**kv):
            (dw, db), = run([i], "rand", dev)
            x, dy, k, s, pad, wb = problem(i, "rand", dev)
            one = ops().conv2d_wgrad(x, dy, k, s, pad, with_bias=wb)
            # and through the C entry itself (caller's dw): a group of one runs the single plan
            out = torch.empty_like(dw)
            (dw3, db3), = run([i], "rand", dev, out=[out])
        dw1, db1 = one if wb else (one, None)
        assert torch.equal(dw, dw1) and torch.equal(dw3, dw1) and dw3.data_ptr() == out.data_ptr()
        assert (db is None and db1 is None) or (torch.equal(db, db1) and torch.equal(db3, db1))


@pytest.mark.parametrize("name", [n for n in GROUPS if len(GROUPS[n]) > 1])
def test_default_mode_gives_the_bits_of_the_single_launches(dev, name):
    """tuning "wgrad_group" = 1: shared launches and reduces, each problem's own
    splits -- torch.equal to conv2d_wgrad, on random data, split or not."""
    idx = GROUPS[name]
    for kv in (OWN, dict(wgrad_group=1)):
        with knobs(**kv):
            plan = ops().wgrad_group_plan([shape_of(i) for i in idx])
            assert plan["grouped"] == 1
            got = run(idx, "rand", dev)
            for i, (dw, db) in zip(idx, got):
                x, dy, k, s, pad, wb = problem(i, "rand", dev)
                one = ops().conv2d_wgrad(x, dy, k, s, pad, with_bias=wb)
                dw1, db1 = one if wb else (one, None)
                assert torch.equal(dw, dw1), (name, i)
                assert (db is None and db1 is None) or torch.equal(db, db1), (name, i)
        if kv is OWN:
            assert max(p["splits"] for p in plan["problems"]) > 1 or name == "ws"


def test_permuting_the_problems_leaves_every_gradient_bit_equal(dev):
    idx = GROUPS["seven"]
    perm = [3, 6, 0, 5, 2, 1, 4]
    with knobs(**SPLITS):
        got = run(idx, "rand", dev)
        moved = run([idx[j] for j in perm], "rand", dev)
    for pos, j in enumerate(perm):
        assert torch.equal(moved[pos][0], got[j][0]), (pos, j)
        if got[j][1] is not None:
            assert torch.equal(moved[pos][1], got[j][1]), (pos, j)


def test_unaligned_dw_gets_the_aligned_run_bit_for_bit(dev):
    """dw as views at a 4-byte offset (a gradient bucket): the reduce's scalar
    stores carry the sums of its float4 form; nothing is written outside."""
    idx = GROUPS["all"]
    sizes = [k * k * Cin * Cout for (_, _, _, Cin, Cout, k, _) in (PROBLEMS[i] for i in idx)]
    with knobs(**SPLITS):
        got = run(idx, "rand", dev)
        buf = torch.full((sum(sizes) + len(idx) + 1,), 7.5, device=dev)
        views, at = [], 1
        for i, n in zip(idx, sizes):
            _, _, _, Cin, Cout, k, _ = PROBLEMS[i]
            views.append(buf[at:at + n].view(k, k, Cin, Cout))
            at += n + 1  # (one guard float between the views)
        assert sum(v.data_ptr() % 16 != 0 for v in views) >= 4
        un = run(idx, "rand", dev, out=views)
    keep = torch.ones_like(buf, dtype=torch.bool)
    at = 1
    for (dw, db), (dwu, dbu), v, n in zip(got, un, views, sizes):
        assert dwu.data_ptr() == v.data_ptr() and torch.equal(dwu, dw)
        assert (db is None) or torch.equal(dbu, db)
        keep[at:at + n] = False
        at += n + 1
    assert bool((buf[keep] == 7.5).all())


# ---- model level: one folded ResNet stage, deferred against per-conv
def _stage(dev):
    from detectron2_tensorflow_amd.layers.conv_weights import FoldGroup
    from detectron2_tensorflow_amd.modeling.backbone.resnet import (BottleneckBlock, Stage,
                                                                   resnet_arg_scope)
    torch.manual_seed(11)
    with resnet_arg_scope(False, "FrozenBN"):
        stage = Stage(BottleneckBlock, dict(in_channels=64, out_channels=256,
                                            bottleneck_channels=64), 2, 1, scope="res2")
    stage = stage.to(dev).train()
    g = torch.Generator().manual_seed(12)
    for m in stage.modules():
        bn = getattr(m, "normalizer_fn", None)
        if bn is not None and hasattr(bn, "moving_variance"):
            with torch.no_grad():
                bn.moving_mean.copy_(torch.randn(bn.moving_mean.shape, generator=g) * 0.1)
                bn.moving_variance.copy_(torch.rand(bn.moving_variance.shape, generator=g) + 0.5)
    group = FoldGroup.attach(stage)
    assert group is not None and len(group.layers) == 7
    return stage


def _backward(stage, x, dy):
    for p in stage.parameters():
        p.grad = None
    y = stage(x)
    y.backward(dy)
    return {n: p.grad.clone() for n, p in stage.named_parameters() if p.grad is not None}


def test_folded_stage_defers_its_weight_gradients_to_one_grouped_call(dev, monkeypatch):
    from detectron2_tensorflow_amd.layers import handoff
    o = ops()
    stage = _stage(dev)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 24, 32, 64, generator=g).to(dev)
    dy = torch.randn(2, 24, 32, 256, generator=g).to(dev)
    singles = []
    real = o.conv.conv2d_wgrad
    monkeypatch.setattr(o.conv, "conv2d_wgrad", lambda *a, **k: (singles.append(a[2]), real(*a, **k))[1])
    monkeypatch.setattr(o, "conv2d_wgrad", o.conv.conv2d_wgrad)
    from detectron2_tensorflow_amd.layers.ops import fold
    grouped = []  # problems of each grouped call the fold's backward makes
    real_group = fold.conv2d_wgrad_group
    monkeypatch.setattr(fold, "conv2d_wgrad_group",
                        lambda ps, **k: (grouped.append(len(ps)), real_group(ps, **k))[1])
    events = []
    grads = {}
    for arm in (1, 0, 1, 2):
        with knobs(wgrad_group=arm):
            del singles[:], events[:], grouped[:]
            handoff.OBSERVER = lambda label, ev: events.append((label, ev))
            try:
                grads.setdefault(arm, []).append(_backward(stage, x, dy))
            finally:
                handoff.OBSERVER = None
            late = [e for e in events if e[0] == "deferred weight gradients"]
            if arm:
                # the two 3x3s (768 pixels: the 1x1s run on hipBLASLt) wait for the
                # fold's backward: one grouped call of both, no MFMA wgrad of their own
                assert grouped == [2] and singles == [], (grouped, singles)
                assert late == [("deferred weight gradients", "deposit")] * 2 + [
                    ("deferred weight gradients", "take")]
            else:
                assert grouped == [] and singles == [3, 3] and late == []
    on, on2 = grads[1]
    off, = grads[0]
    common, = grads[2]
    assert on.keys() == off.keys() == common.keys() and len(on) >= 7
    for n in on:
        # the default keeps every problem's own splits: the per-conv arm's bits
        assert torch.equal(on[n], on2[n]) and torch.equal(on[n], off[n]), n
        scale = float(off[n].abs().max())
        atol = 1e-3 if on[n].dim() == 1 else 2e-5 * scale
        torch.testing.assert_close(common[n], off[n], rtol=1e-4, atol=atol,
                                   msg=lambda m: f"{n}: {m}")
