"""The Relation Network heads without a GPU: the hand-made cases that pin the
padded-column and clamp rules, the embedding's channel order, the tensor
formulation against the float64 restatement (tests/relation_reference.py),
the config keys and the model's structure and variable names, the host-side
argument checks of the C entries, and the module's CPU path."""
import ctypes
import math
import os

import pytest
import torch

import relation_reference as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
FASTER = "COCO-Detection/faster_rcnn_R_50_FPN_1x.yaml"
OVERRIDE = ["MODEL.ROI_HEADS.NAME", "RelationRoiHeads", "MODEL.ROI_BOX_HEAD.NAME", "RelationBoxHead"]
F64 = torch.float64


def _build(override):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", FASTER))
    if override:
        cfg.merge_from_list(OVERRIDE)
    finalize(cfg, False, 1, CATS)
    torch.manual_seed(0)
    return cfg, build_model(cfg)


@pytest.mark.parametrize("bias", [1.0, -1.0])
def test_hand_made_case_padded_columns_and_clamp(bias):
    """Identical boxes, Wg = 0, q = 0: gw = relu(bias), so the log term is 0
    (bias 1) or log 1e-6 (bias -1, the clamp) for every column alike, every
    logit is equal and P is uniform over all 4 columns -- the invalid one
    takes its quarter of the mass and contributes a zero value."""
    from detectron2_tensorflow_amd.modeling.roi_heads import relation_dense
    G, dk, dv, E = 4, 2, 4, 8
    boxes = torch.tensor([[[10., 20., 50., 80.]] * 3 + [[3., 4., 90., 100.]]], dtype=F64)
    valid = torch.tensor([[True, True, True, False]])
    g = torch.Generator().manual_seed(0)
    q = torch.zeros(1, 4, G * dk, dtype=F64)
    k = torch.randn(1, 4, G * dk, generator=g, dtype=F64)
    v = torch.randn(1, 4, dv, generator=g, dtype=F64)  # (slot 3's row must not be read)
    wg, bg = torch.zeros(E, G, dtype=F64), torch.full((G,), bias, dtype=F64)
    want_row = ((v[0, 0] + v[0, 1] + v[0, 2]) / 4).repeat(G)  # / 4, not / 3
    for fn in (relation_dense, rref.relation):
        out = fn(boxes, valid, q, k, v, wg, bg, G)
        assert out.shape == (1, 4, G * dv)
        for i in range(3):
            # (0.25 v is exact; the three-term sum may round in another order)
            torch.testing.assert_close(out[0, i], want_row, rtol=0, atol=1e-14)
        assert (out[0, 3] == 0).all()


@pytest.mark.parametrize("E", [64, 8])
def test_embedding_channel_order(E):
    """Channel t (E/4) + s (E/8) + f is sin (s = 0) / cos (s = 1) of
    100 p_t / 1000^(8 f / E): the concat on the last axis, then the reshape."""
    from detectron2_tensorflow_amd.modeling.roi_heads.relation_module import geometry_embeddings
    boxes = torch.tensor([[[10., 20., 50., 80.], [5., 100., 45., 130.], [30., 10., 200., 40.]]],
                         dtype=F64)
    got = geometry_embeddings(boxes, E)
    want = rref.geometry_embeddings(boxes, E)
    assert got.shape == want.shape == (1, 3, 3, E)
    h = boxes[0, :, 2] - boxes[0, :, 0] + 1
    w = boxes[0, :, 3] - boxes[0, :, 1] + 1
    cy = 0.5 * (boxes[0, :, 0] + boxes[0, :, 2])
    cx = 0.5 * (boxes[0, :, 1] + boxes[0, :, 3])
    for i in range(3):
        for j in range(3):
            p = [math.log(max(float((cy[i] - cy[j]) / h[i]), 1e-5)),
                 math.log(max(float((cx[i] - cx[j]) / w[i]), 1e-5)),
                 math.log(float(h[i] / h[j])), math.log(float(w[i] / w[j]))]
            for c in range(E):
                t, s, f = c // (E // 4), (c % (E // 4)) // (E // 8), c % (E // 8)
                arg = 100.0 * p[t] / 1000.0 ** (8.0 * f / E)
                lit = math.cos(arg) if s else math.sin(arg)
                assert abs(float(want[0, i, j, c]) - lit) < 1e-9, (i, j, c)
                assert abs(float(got[0, i, j, c]) - float(want[0, i, j, c])) < 1e-12, (i, j, c)
    # (slot 0 is above and left of slot 2: both offsets negative, clamped)
    assert float(want[0, 0, 2, 0]) == pytest.approx(math.sin(100.0 * math.log(1e-5)), abs=1e-9)


def random_case(N, R, G, dk, dv, E, seed, dtype=F64, valid=None):
    g = torch.Generator().manual_seed(seed)
    y1 = torch.rand(N, R, generator=g, dtype=F64) * 700
    x1 = torch.rand(N, R, generator=g, dtype=F64) * 1200
    boxes = torch.stack([y1, x1, y1 + torch.rand(N, R, generator=g, dtype=F64) * 99,
                         x1 + torch.rand(N, R, generator=g, dtype=F64) * 132], -1)
    if valid is None:
        valid = torch.rand(N, R, generator=g) < 0.7
    q = torch.randn(N, R, G * dk, generator=g, dtype=F64)
    k = torch.randn(N, R, G * dk, generator=g, dtype=F64)
    v = torch.randn(N, R, dv, generator=g, dtype=F64)
    wg = torch.randn(E, G, generator=g, dtype=F64) * 0.3
    bg = torch.randn(G, generator=g, dtype=F64) * 0.5
    return [t.to(dtype) for t in (boxes,)] + [valid] + [t.to(dtype) for t in (q, k, v, wg, bg)]


def test_dense_formulation_equals_the_restatement():
    from detectron2_tensorflow_amd.modeling.roi_heads import relation_dense
    boxes, valid, q, k, v, wg, bg = random_case(2, 9, 4, 4, 8, 16, seed=1)
    valid[1, :] = torch.tensor([False, True] + [False] * 7)
    assert valid[0].any() and not valid[0].all()
    got = relation_dense(boxes, valid, q, k, v, wg, bg, 4)
    want = rref.relation(boxes, valid, q, k, v, wg, bg, 4)
    assert got.dtype == F64 and float(want.abs().max()) > 0.1
    assert float((got - want).abs().max()) <= 1e-12
    assert (got[~valid] == 0).all()


def test_config_defaults():
    from detectron2_tensorflow_amd.config import get_cfg
    r = get_cfg().MODEL.ROI_BOX_RELATION_HEAD
    assert (r.NUM_GROUPS, r.KEY_DIM, r.GEOMETRY_EMBEDDING_DIM) == (16, 64, 64)
    assert (r.DUPLICATE_REMOVAL_IOU, r.RANK_EMBEDDING_DIM, r.NMS_NUM_GROUP) == (0.5, 128, 16)


def test_override_builds_the_relation_heads_with_the_reference_names():
    from detectron2_tensorflow_amd.modeling import (ObjectRelationModule, RelationBoxHead,
                                                    RelationRoiHeads, StandardROIHeads)
    _, model = _build(True)
    rh = model.roi_heads
    assert type(rh) is RelationRoiHeads and type(rh.box_head) is RelationBoxHead
    assert len(rh.box_head.relations) == 2
    assert all(isinstance(m, ObjectRelationModule) for m in rh.box_head.relations)
    names = {n: tuple(t.shape) for n, t in model.reference_variables(include_scope=False)}
    shapes = {"geometry": ((1, 1, 64, 16), (16,)), "query": ((1024, 64), (64,)),
              "key": ((1024, 64), (64,)), "value": ((1024, 64), (64,))}
    rel = {}
    for r in ("r1", "r2"):
        for layer, (ws, bs) in shapes.items():
            rel[f"roi_heads/box_head/{r}/{layer}/weights"] = ws
            rel[f"roi_heads/box_head/{r}/{layer}/bias"] = bs
    for n, s in rel.items():
        assert names[n] == s, n
    # without the override: StandardROIHeads, and the same names minus the relation modules'
    _, plain = _build(False)
    assert type(plain.roi_heads) is StandardROIHeads
    plain_names = {n: tuple(t.shape) for n, t in plain.reference_variables(include_scope=False)}
    assert plain_names == {n: s for n, s in names.items() if n not in rel}
    assert not [n for n in plain_names if "/r1/" in n or "/r2/" in n]
    assert "roi_heads/box_head/fc2/weights" in plain_names


def test_relation_entries_refuse_bad_arguments_without_gpu():
    """Argument validation happens on the host before any launch; the message
    names the argument."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    a = ctypes.c_void_p(4096)  # aligned, never dereferenced: refused first

    def fwd(G=16, dk=4, dv=64, E=64):
        return lib.d2mi_relation_fwd(a, a, a, a, a, a, a, 2, 65, G, dk, dv, E, a, a, None)

    def bwd(G=16, dk=4, dv=64, E=64, ws=a, n=1 << 40):
        return lib.d2mi_relation_bwd(a, a, a, a, a, a, a, a, a, a, 2, 65, G, dk, dv, E, a, a, a, a,
                                     a, ws, n, None)

    for call in (fwd, bwd):
        for kw, word in (({"E": 12}, "E = 12"), ({"dk": 16}, "dk = 16"), ({"dv": 6}, "dv = 6"),
                         ({"G": 17}, "G = 17"), ({"E": 136}, "E = 136"), ({"dv": 68}, "dv = 68")):
            rc = call(**kw)
            assert rc < 0 and word in _C.last_error(), (kw, _C.last_error())
    size = lib.d2mi_relation_workspace_size(2, 65, 16, 4, 64, 64)
    assert size > 1
    rc = bwd(n=size - 1)
    msg = _C.last_error()
    assert rc < 0 and "too small" in msg and f"{size - 1} < {size}" in msg, msg


def test_envelope_predicate_matches_the_host_checks():
    from detectron2_tensorflow_amd.layers import ops
    assert ops.relation_supported(16, 4, 64, 64) and ops.relation_supported(4, 8, 16, 128)
    for bad in ((17, 4, 64, 64), (16, 16, 64, 64), (16, 4, 6, 64), (16, 4, 128, 64),
                (16, 4, 64, 12), (16, 4, 64, 136)):
        assert not ops.relation_supported(*bad), bad
    # the toggle has one owner and is not an attribute of the package
    from detectron2_tensorflow_amd.layers.ops import relation
    assert relation.FUSED_RELATION in (True, False) and not hasattr(ops, "FUSED_RELATION")


def test_module_cpu_path_backpropagates_to_all_eight_parameters():
    from detectron2_tensorflow_amd.modeling import ObjectRelationModule
    from detectron2_tensorflow_amd.modeling.roi_heads import relation_dense
    torch.manual_seed(0)
    m = ObjectRelationModule(input_size=32, embedding_dim=16, key_dim=8, num_groups=4, scope="r1")
    names = [n for n, _ in m.reference_variables()]
    assert names == [f"r1/{layer}/{leaf}" for layer in ("geometry", "query", "key", "value")
                     for leaf in ("weights", "bias")]
    with torch.no_grad():
        m.geometry.bias.fill_(0.5)
    boxes, valid, *_ = random_case(2, 5, 4, 2, 8, 16, seed=2, dtype=torch.float32)
    valid[0, 0] = True
    x = torch.randn(10, 32, requires_grad=True)
    assert not m.fused(x)
    y = m(x, boxes, valid)
    assert y.shape == x.shape
    # the module is features + relation_dense(...) of its own projections
    q, k, v = (lin(x).reshape(2, 5, -1) for lin in (m.query, m.key, m.value))
    want = x + relation_dense(boxes, valid, q, k, v, m.geometry.weights.reshape(16, 4),
                              m.geometry.bias, 4).reshape(10, 32)
    assert torch.equal(y, want)
    assert torch.equal(y[~valid.reshape(-1)], x[~valid.reshape(-1)])  # invalid rows unchanged
    y.square().sum().backward()
    params = dict(m.named_parameters())
    assert len(params) == 8
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    assert torch.isfinite(x.grad).all()
