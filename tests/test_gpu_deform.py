"""GPU tests of deformable convolution: the HIP sampler
(d2mi_deform_sample_fwd / _bwd) against the restatement of the reference
(tests/deform_reference.py) -- the forward bit for bit, the gradients against
float64 autograd at the project's float bound (max abs error <= 1e-4 * max
|reference|) -- layers.DeformConv2D against Conv2D and the restatement, and
the dconv Mask R-CNN config end to end (inference, an eager training step,
the graphed step against the eager one).

Measured on the MI355X (max abs error / max |reference|; the bound is 1e-4):
see DESIGN.md "Deformable convolution"."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
DCONV = os.path.join(ROOT, "configs", "Misc", "mask_rcnn_R_50_FPN_1x_dconv_c3-c5.yaml")
BOUND = 1e-4

#         N  H   W   C    G  k  stride rate padding
SHAPES = [(2, 7, 9, 8, 2, 3, 1, 1, "SAME"),
          (1, 8, 11, 16, 1, 3, 2, 1, "SAME"),
          (1, 9, 9, 8, 1, 3, 1, 2, "SAME"),
          (1, 6, 7, 8, 1, 3, 1, 1, "VALID"),
          (1, 13, 17, 128, 1, 3, 1, 1, "SAME")]
IDS = ["g2", "stride2", "rate2", "valid", "c128"]

_CASES = {}


def _case(shape):
    """Inputs and the restatement's results of one shape, computed once:
    offsets normal(0, 2), so a good share of the samples clip."""
    if shape in _CASES:
        return _CASES[shape]
    N, H, W, C, G, k, stride, rate, padding = shape
    rng = np.random.default_rng(len(_CASES) + 1)
    pads = ref.pads_of(k, rate, padding)
    OH, OW = ref.out_size(H, k, stride, rate, pads), ref.out_size(W, k, stride, rate, pads)
    x = torch.from_numpy(rng.normal(size=(N, H, W, C)).astype(np.float32))
    off = torch.from_numpy(rng.normal(0, 2, size=(N, OH, OW, 2 * G * k * k)).astype(np.float32))
    gcols = torch.from_numpy(rng.normal(size=(N, OH, OW, k * k * C)).astype(np.float32))
    cols32 = ref.deform_cols(x, off, k, stride, rate, padding, G, torch.float32)
    xd = x.double().requires_grad_(True)
    od = off.double().requires_grad_(True)
    cols64 = ref.deform_cols(xd, od, k, stride, rate, padding, G, torch.float64)
    gx, goff = torch.autograd.grad(cols64, (xd, od), gcols.double())
    _CASES[shape] = dict(x=x, off=off, gcols=gcols, cols=cols32, gx=gx, goff=goff, pads=pads)
    return _CASES[shape]


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_bit_exact(dev, shape):
    from detectron2_tensorflow_amd.layers import ops
    c = _case(shape)
    N, H, W, C, G, k, stride, rate, padding = shape
    cols = ops.deform_sample(c["x"].to(dev), c["off"].to(dev), k, stride, rate, c["pads"], G)
    assert torch.equal(cols.cpu(), c["cols"])
    # an offset map padded to a multiple of 4 channels is read through its row stride
    offp = torch.cat([c["off"], torch.full(c["off"].shape[:3] + (2,), 7.0)], 3).to(dev)
    assert torch.equal(ops.deform_sample(c["x"].to(dev), offp, k, stride, rate, c["pads"], G).cpu(),
                       c["cols"])


def test_forward_zero_offsets_is_im2col(dev):
    from detectron2_tensorflow_amd.layers import ops
    x = _case(SHAPES[0])["x"]
    for stride, rate in ((1, 1), (2, 1), (1, 2)):
        want = ref.im2col(x, 3, stride, rate, "SAME")
        off = torch.zeros(want.shape[:3] + (36,), device=dev)
        got = ops.deform_sample(x.to(dev), off, 3, stride, rate, ref.same_pads(3, rate), 2)
        assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_matches_float64_autograd_and_is_deterministic(dev, shape):
    from detectron2_tensorflow_amd.layers import ops
    c = _case(shape)
    N, H, W, C, G, k, stride, rate, padding = shape
    args = (c["x"].to(dev), c["off"].to(dev), c["gcols"].to(dev), k, stride, rate, c["pads"], G)
    gx, goff = ops.deform_sample_bwd(*args)
    gx2, goff2 = ops.deform_sample_bwd(*args)
    ex, eo = _rel(gx, c["gx"]), _rel(goff, c["goff"])
    print(f"deform bwd {IDS[SHAPES.index(shape)]}: gx err {ex:.3e} goffsets err {eo:.3e} "
          f"(x max|ref|)")
    assert ex <= BOUND and eo <= BOUND
    assert torch.equal(gx, gx2) and torch.equal(goff, goff2)
    # through autograd, with a padded offset map: the pad channels get 0
    x = args[0].clone().requires_grad_(True)
    offp = torch.cat([args[1], torch.zeros_like(args[1][..., :2])], 3).requires_grad_(True)
    ops.deform_sample(x, offp, k, stride, rate, c["pads"], G).backward(args[2])
    assert torch.equal(x.grad, gx)
    assert torch.equal(offp.grad[..., :-2], goff) and float(offp.grad[..., -2:].abs().max()) == 0.0


def test_backward_collision_case(dev):
    """Every tap of every output lands in one interior pixel neighbourhood
    (y = 5.3, x = 7.6): 8,640 contributions on 4 pixels -- the long-list
    split of the sum pass (and the merge path of the key sort)."""
    from detectron2_tensorflow_amd.layers import ops
    N, H, W, C, k = 1, 12, 20, 8, 3
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.normal(size=(N, H, W, C)).astype(np.float32))
    gcols = torch.from_numpy(rng.normal(size=(N, H, W, 9 * C)).astype(np.float32))
    by, bx = ref.base_positions(H, W, k, 1, 1)
    off = torch.stack([5.3 - by.float(), 7.6 - bx.float()], -1).reshape(1, H, W, 18)
    xd, od = x.double().requires_grad_(True), off.double().requires_grad_(True)
    cols64 = ref.deform_cols(xd, od, k, 1, 1, "SAME", 1, torch.float64)
    wx, wo = torch.autograd.grad(cols64, (xd, od), gcols.double())
    assert int((wx.abs().sum(-1) > 0).sum()) == 4
    args = (x.to(dev), off.to(dev), gcols.to(dev), k, 1, 1, (1, 1), 1)
    cols = ops.deform_sample(*args[:2], k, 1, 1, (1, 1), 1)
    assert torch.equal(cols.cpu(), ref.deform_cols(x, off, k, 1, 1, "SAME", 1))
    gx, goff = ops.deform_sample_bwd(*args)
    gx2, goff2 = ops.deform_sample_bwd(*args)
    ex, eo = _rel(gx, wx), _rel(goff, wo)
    print(f"deform bwd collision: gx err {ex:.3e} goffsets err {eo:.3e} (x max|ref|)")
    assert ex <= BOUND and eo <= BOUND
    assert torch.equal(gx, gx2) and torch.equal(goff, goff2)
    assert int((gx.abs().sum(-1) > 0).sum()) == 4


def _layers(dev, cin, cout, **kw):
    from detectron2_tensorflow_amd.layers import Conv2D, DeformConv2D
    torch.manual_seed(3)
    d = DeformConv2D(cin, cout, 3, **kw).to(dev)
    c = Conv2D(cin, cout, 3, impl="mfma", **kw).to(dev)
    with torch.no_grad():
        d.bias.normal_()
        c.weights.copy_(d.weights)
        c.bias.copy_(d.bias)
    return d, c


def test_fresh_layer_equals_conv2d(dev):
    """Zero-initialised offsets: a plain 3x3 conv (SAME: every tap on the
    last padded row / column reads the zero ring either way)."""
    d, c = _layers(dev, 128, 128, activation="relu")
    x = torch.randn(2, 13, 17, 128, device=dev)
    with torch.no_grad():
        got, want = d(x), c(x)
    assert got.shape == want.shape == (2, 13, 17, 128)
    assert getattr(got, "_d2mi_relu_info", None) is not None  # the fused ReLU's tag
    err = float((got - want).abs().max() / want.abs().max())
    print(f"DeformConv2D vs Conv2D: {err:.3e} x max")
    assert err <= BOUND


OFFSET_BIAS = [0.37, -0.37, 1.6, -2.25, 0.81, 1.27, -1.6, 0.37, 2.25, -0.81, -0.37, 1.6, 0.63,
               -1.27, -2.25, 0.37, 1.6, -0.63]


@pytest.mark.parametrize("stride,padding", [(1, "SAME"), (2, "SAME"), (1, "VALID")])
def test_layer_matches_restatement_with_gradients(dev, stride, padding):
    """offset_weights = 0 and a fixed fractional offset_bias: the positions sit
    away from the integers, so no floor can flip between f32 and float64."""
    from detectron2_tensorflow_amd.layers import DeformConv2D
    torch.manual_seed(5)
    cin, cout = 16, 24
    layer = DeformConv2D(cin, cout, 3, stride=stride, padding=padding).to(dev)
    with torch.no_grad():
        layer.bias.normal_()
        layer.offset_bias.copy_(torch.tensor(OFFSET_BIAS))
    x = torch.randn(2, 10, 13, cin, device=dev, requires_grad=True)
    out = layer(x)
    gout = torch.randn_like(out)
    out.backward(gout)
    names = ("weights", "bias", "offset_weights", "offset_bias")
    P = {n: getattr(layer, n).detach().cpu().double().requires_grad_(True) for n in names}
    xd = x.detach().cpu().double().requires_grad_(True)
    want = ref.deform_conv(xd, P["weights"], P["bias"], P["offset_weights"], P["offset_bias"], 3,
                           stride, 1, padding, 1, torch.float64)
    grads = torch.autograd.grad(want, [xd] + [P[n] for n in names], gout.cpu().double())
    errs = {"out": _rel(out.detach(), want.detach()), "x": _rel(x.grad, grads[0])}
    for n, g in zip(names, grads[1:]):
        errs[n] = _rel(getattr(layer, n).grad, g)
    print(f"DeformConv2D s{stride} {padding} vs float64 restatement (x max):",
          {k: f"{v:.3e}" for k, v in errs.items()})
    assert all(v <= BOUND for v in errs.values()), errs


def test_layer_forward_with_learned_offsets(dev):
    """Random offset_weights under SAME padding (the map is continuous in the
    offsets there: a floor that flips between f32 and float64 moves nothing)."""
    from detectron2_tensorflow_amd.layers import DeformConv2D
    torch.manual_seed(6)
    layer = DeformConv2D(16, 24, 3, deform_num_groups=2).to(dev)
    with torch.no_grad():
        layer.offset_weights.normal_(0, 0.1)
        layer.offset_bias.normal_()
        layer.bias.normal_()
        x = torch.randn(2, 10, 13, 16, device=dev)
        out = layer(x)
        want = ref.deform_conv(x.cpu(), layer.weights.cpu(), layer.bias.cpu(),
                               layer.offset_weights.cpu(), layer.offset_bias.cpu(), 3, 1, 1, "SAME",
                               2, torch.float64)
    err = _rel(out, want)
    print(f"DeformConv2D learned offsets vs float64 restatement: {err:.3e} x max")
    assert err <= BOUND


# ------------------------------------------------------------- whole model
def _model(dev, training):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(DCONV)
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    if training:
        cfg.SOLVER.WARMUP_ITERS = 3
    finalize(cfg, training, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    return cfg, (model.train() if training else model.eval())


def _perturb_offsets(model):
    """Non-zero offsets (a fresh layer's are 0: every sample would sit on the
    integer grid)."""
    from detectron2_tensorflow_amd.layers import DeformConv2D
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, DeformConv2D):
                m.offset_bias.copy_(torch.randn(m.offset_bias.shape, generator=g))
                m.offset_weights.copy_(torch.randn(m.offset_weights.shape, generator=g) * 1e-3)


def test_dconv_model_inference(dev):
    from detectron2_tensorflow_amd import _C
    cfg, model = _model(dev, False)
    _perturb_offsets(model)
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.uniform(0, 255, size=(1, 256, 320, 3)).astype(np.float32)).to(dev)
    with torch.no_grad():
        out = model.inference({"image": img, "image_shape": torch.tensor([[256, 320]], device=dev)})
    inst = out["instances"]
    assert inst["boxes"].shape == (1, 100, 4) and inst["masks"].shape == (1, 100, 28, 28)
    assert torch.isfinite(inst["boxes"]).all() and torch.isfinite(inst["masks"]).all()
    _C.raise_on_errors(dev)


def test_dconv_model_training_step(dev):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.layers import DeformConv2D
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg, model = _model(dev, True)
    _perturb_offsets(model)
    batch = synthetic_train_batch(2, 256, 320, 0, dev)
    calibrate_rcnn_scores(model, batch)
    grads = {}
    hooks = [m.offset_weights.register_hook(
        lambda g, n=n: grads.__setitem__(n, float(g.abs().max())))
        for n, m in model.named_modules() if isinstance(m, DeformConv2D)]
    losses = Trainer(cfg, model).step(batch)
    _C.raise_on_errors(dev)
    for h in hooks:
        h.remove()
    assert all(np.isfinite(float(v)) for v in losses.values()), losses
    assert len(grads) == 13 and all(np.isfinite(v) and v > 0.0 for v in grads.values()), grads
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_dconv_graphed_step_one_replay_matches_eager_step(dev, monkeypatch):
    """tests/test_gpu_graphed.py::test_graphed_step_one_replay_matches_eager_step
    with the dconv config: losses, weights and momentum bit-identical, and no
    capture holds a memset node."""
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.engine.graphed import GraphedTrainer
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    cfg, m_eager = _model(dev, True)
    _, m_graph = _model(dev, True)
    _perturb_offsets(m_eager)
    batch = synthetic_train_batch(2, 256, 320, 11, dev)
    calibrate_rcnn_scores(m_eager, batch)
    m_graph.load_state_dict(m_eager.state_dict())
    eager = Trainer(cfg, m_eager)
    graphed = GraphedTrainer(cfg, m_graph, warmup=1)
    for i in range(2):  # 0: the graphed trainer's eager warm-up; 1: capture + ONE replay
        torch.manual_seed(100 + i)
        le = eager.step(batch)
        torch.manual_seed(100 + i)
        lg = graphed.step(batch)
        torch.cuda.synchronize()
        assert set(le) == set(lg)
        for k in le:
            assert torch.equal(le[k].reshape(()), lg[k].reshape(())), (i, k, le[k], lg[k])
        for (n, pe), pg in zip(m_eager.named_parameters(), m_graph.parameters()):
            assert torch.equal(pe, pg), (i, n)
        for ae, ag in zip(eager.optimizer.accum, graphed.optimizer.accum):
            assert torch.equal(ae, ag), i
    assert graphed.replays == 1
    assert graphed.census and all(c.get("memset", 0) == 0 and c.get("kernel", 0) > 100
                                  for c in graphed.census.values()), graphed.census
    _C.raise_on_errors(dev)
