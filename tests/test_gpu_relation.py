"""The fused relation attention on the GPU (ops.relation_attention,
csrc/relation.hip) against the float64 restatement of the reference
(tests/relation_reference.py), forward and backward, with the tolerance taken
from the float32 tensor formulation's own distance from float64; determinism,
the module with the toggle on and off, the whole model, and graph capture.

Shapes: the issue's (1,1) (1,2) (2,63) (2,65) (1,130), plus one below / above
every tile width of the kernels -- 64 columns per tile (63 / 65), 4 rows per
forward workgroup (2 / 5), 2 rows per row-pass workgroup (1 / 3), 8 rows per
column-pass chunk (5 / 9), and past 256 rows the chunk grows (257: 9 rows)."""
import functools
import os

import numpy as np
import pytest
import torch

import relation_reference as rref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
FASTER = os.path.join(ROOT, "configs", "COCO-Detection", "faster_rcnn_R_50_FPN_1x.yaml")
OVERRIDE = ["MODEL.ROI_HEADS.NAME", "RelationRoiHeads", "MODEL.ROI_BOX_HEAD.NAME", "RelationBoxHead"]
F64 = torch.float64

SHAPES = [(1, 1), (1, 2), (2, 63), (2, 65), (1, 130), (1, 3), (1, 5), (1, 9)]
SIZES = [(16, 4, 64, 64), (4, 4, 16, 8), (16, 4, 64, 128)]  # (G, dk, dv, E)
CASES = [(s, z) for z in SIZES for s in SHAPES] + [((1, 257), SIZES[0])]
PATTERNS = ("all", "scattered", "one_empty", "one_single")


def _valid(pattern, N, R, g):
    if pattern == "all":
        return torch.ones(N, R, dtype=torch.bool)
    v = torch.rand(N, R, generator=g) < 0.6
    if pattern == "scattered":
        v[:, 0] = True
        return v
    v[N - 1] = False  # the last image: no valid slot / a single one
    if pattern == "one_single":
        v[N - 1, R // 2] = True
    return v


def _inputs(N, R, G, dk, dv, E, pattern, seed, backward):
    """float32 inputs on the host: boxes inside an 800 x 1333 image, every
    fifth an exact duplicate of its predecessor and every seventh a 1-pixel
    box (y2 = y1, x2 = x1).  Forward: Wg ~ N(0, 0.3), bg ~ N(0, 0.5) (both
    clamp sides and the ReLU edge).  Backward: |Wg| <= 0.005, bg = +-1."""
    g = torch.Generator().manual_seed(seed)
    y1 = torch.rand(N, R, generator=g) * 700
    x1 = torch.rand(N, R, generator=g) * 1200
    boxes = torch.stack([y1, x1, y1 + torch.rand(N, R, generator=g) * 99 + 1,
                         x1 + torch.rand(N, R, generator=g) * 132 + 1], -1)
    idx = torch.arange(R)
    one = idx % 7 == 3
    boxes[:, one, 2:] = boxes[:, one, :2]
    dup = (idx % 5 == 4) & (idx > 0)
    boxes[:, dup] = boxes[:, torch.nonzero(dup)[:, 0] - 1]
    valid = _valid(pattern, N, R, g)
    q = torch.randn(N, R, G * dk, generator=g)
    k = torch.randn(N, R, G * dk, generator=g)
    v = torch.randn(N, R, dv, generator=g)
    if backward:
        wg = (torch.rand(E, G, generator=g) * 2 - 1) * 0.005
        bg = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0)
    else:
        wg = torch.randn(E, G, generator=g) * 0.3
        bg = torch.randn(G, generator=g) * 0.5
    d_out = torch.randn(N, R, G * dv, generator=g)
    return boxes, valid, q, k, v, wg, bg, d_out


def _grads(fn, boxes, valid, q, k, v, wg, bg, G, d_out):
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v, wg, bg)]
    out = fn(boxes, valid, *leaves, G)
    return out.detach(), torch.autograd.grad(out, leaves, d_out.to(out.dtype))


@functools.lru_cache(maxsize=None)
def _case(N, R, G, dk, dv, E, pattern, backward):
    """One case's inputs on the GPU with the float64 restatement's output (and
    gradients) and the float32 tensor formulation's: computed once, shared by
    the tests, never modified."""
    from detectron2_tensorflow_amd.modeling.roi_heads import relation_dense
    dev = torch.device("cuda:0")
    seed = N * 1000 + R + 17 * E + PATTERNS.index(pattern)
    t32 = [t.to(dev) for t in _inputs(N, R, G, dk, dv, E, pattern, seed, backward)]
    boxes, valid, q, k, v, wg, bg, d_out = t32
    t64 = [t.to(F64) if t.is_floating_point() else t for t in t32]
    if not backward:
        with torch.no_grad():
            ref = rref.relation(*t64[:7], G)
            dense = relation_dense(boxes, valid, q, k, v, wg, bg, G)
        return t32, ref, dense, None, None
    ref, ref_g = _grads(rref.relation, *t64[:7], G, t64[7])
    dense, dense_g = _grads(relation_dense, boxes, valid, q, k, v, wg, bg, G, d_out)
    return t32, ref, dense, ref_g, dense_g


def _check(name, got, ref, dense, worst):
    """max |got - ref64| <= 4 e_ref + 1e-6 max |ref64|, e_ref the float32
    tensor formulation's own distance from the float64 restatement."""
    e_ref = float((dense.to(F64) - ref).abs().max())
    e_hip = float((got.to(F64) - ref).abs().max())
    bound = 4 * e_ref + 1e-6 * float(ref.abs().max())
    worst.append((name, e_ref, e_hip, bound))
    return e_hip <= bound


@pytest.mark.parametrize("shape,size", CASES)
def test_forward_matches_the_float64_restatement(dev, shape, size):
    from detectron2_tensorflow_amd.layers import ops
    (N, R), (G, dk, dv, E) = shape, size
    log, bad = [], []
    for pattern in PATTERNS:
        (boxes, valid, q, k, v, wg, bg, _), ref, dense, _, _ = _case(N, R, G, dk, dv, E, pattern,
                                                                    False)
        got = ops.relation_attention(boxes, valid, q, k, v, wg, bg, G)
        assert got.shape == (N, R, G * dv) and torch.isfinite(got).all()
        assert (got[~valid] == 0).all(), pattern
        if not _check(pattern, got, ref, dense, log):
            bad.append(pattern)
    print("forward", shape, size, [(n, f"{a:.3e}", f"{b:.3e}", f"{c:.3e}") for n, a, b, c in log])
    assert not bad, (bad, log)


@pytest.mark.parametrize("shape,size", CASES)
def test_backward_matches_float64_autograd_of_the_restatement(dev, shape, size):
    """dq, dk, dv, dWg, dbg (and out) within 4 e_ref + 1e-6 max|ref| of float64
    autograd of the restatement, per tensor and validity pattern.  (Measured
    on the MI355X, worst kernel error / bound: out 0.55, dq 0.43, dk 0.43,
    dv 0.53, dWg 0.26, dbg 0.65.)"""
    from detectron2_tensorflow_amd.layers import ops
    (N, R), (G, dk, dv, E) = shape, size
    log, bad = [], []
    for pattern in PATTERNS:
        t32, ref, dense, ref_g, dense_g = _case(N, R, G, dk, dv, E, pattern, True)
        boxes, valid, q, k, v, wg, bg, d_out = t32
        # every pre-activation is far from the gradient's discontinuities at
        # gw = 0 and gw = 1e-6: |sum_c emb_c Wg[c, g]| <= E * 0.005 <= 0.64,
        # so even groups have gw in [0.36, 1.64] and odd groups are clamped
        assert float(wg.abs().max()) <= 0.005 and E * 0.005 <= 0.64
        assert (bg[0::2] == 1).all() and (bg[1::2] == -1).all()
        out, got_g = _grads(ops.relation_attention, boxes, valid, q, k, v, wg, bg, G, d_out)
        if not _check(pattern + "/out", out, ref, dense, log):
            bad.append(pattern + "/out")
        for name, g_hip, g_ref, g_dense in zip(("dq", "dk", "dv", "dWg", "dbg"), got_g, ref_g,
                                               dense_g):
            assert torch.isfinite(g_hip).all(), (pattern, name)
            if not _check(f"{pattern}/{name}", g_hip, g_ref, g_dense, log):
                bad.append(f"{pattern}/{name}")
        d_q, d_k, d_v, d_wg, d_bg = got_g
        for name, t in (("dq", d_q), ("dk", d_k), ("dv", d_v)):
            assert (t[~valid] == 0).all(), (pattern, name)
        assert (d_wg[:, 1::2] == 0).all() and (d_bg[1::2] == 0).all(), pattern
        if R > 1 and valid.any():  # (a single column: P = 1 and every gradient but dv is 0)
            assert float(d_wg[:, 0::2].abs().max()) > 0 and float(d_bg[0::2].abs().max()) > 0
    print("backward", shape, size, [(n, f"{a:.3e}", f"{b:.3e}", f"{c:.3e}") for n, a, b, c in log])
    assert not bad, (bad, [r for r in log if r[0] in bad])


def test_two_runs_are_bit_identical(dev):
    from detectron2_tensorflow_amd.layers import ops
    (boxes, valid, q, k, v, wg, bg, d_out), *_ = _case(2, 65, 16, 4, 64, 64, "scattered", True)
    runs = [_grads(ops.relation_attention, boxes, valid, q, k, v, wg, bg, 16, d_out)
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


def test_module_fused_and_dense_paths_agree(dev, monkeypatch):
    """ObjectRelationModule with FUSED_RELATION on (the kernels) and off (the
    tensor formulation): outputs and parameter gradients within the tolerance
    rule, the reference being the module run in float64."""
    import copy
    from detectron2_tensorflow_amd.layers.ops import relation
    from detectron2_tensorflow_amd.modeling import ObjectRelationModule
    torch.manual_seed(0)
    m = ObjectRelationModule(input_size=256, embedding_dim=64, key_dim=64, num_groups=16,
                             scope="r1").to(dev)
    with torch.no_grad():  # (the backward test's condition on the geometry conv)
        m.geometry.weights.uniform_(-0.005, 0.005)
        m.geometry.bias.copy_(torch.where(torch.arange(16) % 2 == 0, 1.0, -1.0))
    m64 = copy.deepcopy(m).double().cpu()  # (the float64 module: on the host)
    boxes, valid, *_ = _inputs(2, 65, 16, 4, 16, 64, "scattered", 5, True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(130, 256, generator=g)
    gy = torch.randn(130, 256, generator=g)

    def run(mod, fused, dt, where):
        monkeypatch.setattr(relation, "FUSED_RELATION", fused)
        xi = x.to(where, dt).requires_grad_(True)
        assert mod.fused(xi) == fused
        y = mod(xi, boxes.to(where, dt), valid.to(where))
        grads = torch.autograd.grad(y, [xi] + list(mod.parameters()), gy.to(where, dt))
        return [t.detach().to(dev) for t in [y] + list(grads)]

    fused = run(m, True, torch.float32, dev)
    dense = run(m, False, torch.float32, dev)
    ref = run(m64, False, F64, torch.device("cpu"))
    names = ["y", "dx"] + [n for n, _ in m.named_parameters()]
    log = []
    bad = [n for n, a, d, r in zip(names, fused, dense, ref) if not _check(n, a, r, d, log)]
    print("module", [(n, f"{a:.3e}", f"{b:.3e}", f"{c:.3e}") for n, a, b, c in log])
    assert not bad, (bad, log)
    assert all(float(t.abs().max()) > 0 for t in fused)


def _model(dev, training):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(FASTER)
    cfg.merge_from_list(OVERRIDE)
    if training:
        cfg.SOLVER.WARMUP_ITERS = 3
    finalize(cfg, training, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    return cfg, (model.train() if training else model.eval())


def test_relation_model_inference(dev, monkeypatch):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers.ops import relation
    from detectron2_tensorflow_amd.modeling import RelationRoiHeads
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_images
    monkeypatch.setattr(relation, "FUSED_RELATION", True)  # (the kernels, whatever the default)
    _, model = _model(dev, False)
    assert isinstance(model.roi_heads, RelationRoiHeads)
    with torch.no_grad():
        inst = model.inference(synthetic_images(2, 128, 160, 0, dev))["instances"]
    assert inst["boxes"].shape == (2, 100, 4) and inst["scores"].shape == (2, 100)
    for k in ("boxes", "scores"):
        assert torch.isfinite(inst[k]).all(), k
    assert {"boxes", "scores", "is_valid"} <= set(inst)
    _C.raise_on_errors(dev)


def test_relation_model_training_step(dev, monkeypatch):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.layers.ops import relation
    monkeypatch.setattr(relation, "FUSED_RELATION", True)  # (the kernels, whatever the default)
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg, model = _model(dev, True)
    batch = synthetic_train_batch(2, 128, 160, 0, dev, sqrt_area=(16.0, 128.0))
    calibrate_rcnn_scores(model, batch)
    grads = {}
    hooks = [p.register_hook(lambda g, n=n: grads.__setitem__(n, float(g.abs().max())))
             for n, p in model.roi_heads.box_head.relations.named_parameters()]
    assert len(hooks) == 16
    losses = Trainer(cfg, model).step(batch)
    _C.raise_on_errors(dev)
    for h in hooks:
        h.remove()
    print({k: round(float(v), 4) for k, v in losses.items()}, grads)
    for k in ("loss_cls", "loss_box_reg"):
        assert np.isfinite(float(losses[k])), losses
    assert len(grads) == 16 and all(np.isfinite(v) and v > 0.0 for v in grads.values()), grads
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_forward_and_backward_capture_into_a_graph(dev):
    """The op makes no host synchronisation: forward + backward captured on one
    stream (no parallel branches) replay to the eager result bit for bit."""
    from detectron2_tensorflow_amd.layers import ops
    (boxes, valid, q, k, v, wg, bg, d_out), *_ = _case(2, 65, 16, 4, 64, 64, "scattered", True)
    eager_out, eager_g = _grads(ops.relation_attention, boxes, valid, q, k, v, wg, bg, 16, d_out)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v, wg, bg)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up on the capture stream: scratch allocated)
        out = ops.relation_attention(boxes, valid, *leaves, 16)
        torch.autograd.grad(out, leaves, d_out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = ops.relation_attention(boxes, valid, *leaves, 16)
        grads = torch.autograd.grad(out, leaves, d_out)
    for _ in range(2):
        out.zero_()
        for t in grads:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_out)
        for a, b in zip(grads, eager_g):
            assert torch.equal(a, b)
