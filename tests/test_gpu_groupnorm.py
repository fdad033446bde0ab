"""GroupNorm training on the GPU (d2mi_group_norm_train_fwd / _bwd): the HIP
arm of ops.group_norm_train against the float64 restatement
(tests/gn_reference.py), against the inference kernel's bits and against the
torch arm, through Conv2D, and in one Trainer step of SOLOv2."""
import pytest
import torch

import gn_reference as ref
from test_groupnorm_cpu import check_against_float64, inputs, run_op

pytestmark = pytest.mark.gpu
PASSES = ["gn_train_fwd", "gn_train_bwd"]

# shape [N, H, W, C], G: the smallest at which each mechanism can go wrong
SHAPES = [
    ((1, 1, 1, 8), 2),        # one pixel: the variance of 4 channels; no NaN in either group
    ((2, 5, 7, 8), 2),        # one quad per group, an odd H*W, two ragged forward chunks
    ((3, 9, 11, 24), 2),      # C/4 = 6 does not divide 256: idle threads, 3 quads per group
    ((1, 67, 61, 64), 16),    # the most forward chunks, ragged last chunks in both directions
    ((70, 7, 7, 256), 32),    # many images, a tiny H*W: the dgamma / dbeta sum over N
    ((300, 7, 7, 64), 16),    # more images than runs in that sum: ten images per run, a ragged last
    ((2, 3, 5, 2048), 32),    # C/4 > 256: the quad loop
]


def _recorded(fn):
    """fn() with the launch records on: (result, the recorded gn_* launch names)."""
    from detectron2_tensorflow_amd.layers.ops import KernelTimer
    saved = (KernelTimer.enabled, KernelTimer.detail, KernelTimer.records)
    KernelTimer.reset()
    try:
        out = fn()
        names = [r[0] for r in KernelTimer.records if r[0].startswith("gn_")]
    finally:
        KernelTimer.enabled, KernelTimer.detail, KernelTimer.records = saved
    return out, names


@pytest.fixture
def toggle():
    """Sets ops.norm.FUSED_GN_TRAIN for one test and puts the old value back."""
    from detectron2_tensorflow_amd.layers.ops import norm
    old = norm.FUSED_GN_TRAIN

    def set_(value):
        norm.FUSED_GN_TRAIN = value
    yield set_
    norm.FUSED_GN_TRAIN = old


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,G", SHAPES)
def test_hip_arm_vs_float64_deterministic_and_inference_bits(dev, toggle, shape, G, relu):
    from detectron2_tensorflow_amd.layers import ops
    toggle(True)
    t = inputs(shape, 21)
    got, names = _recorded(lambda: run_op(t, G, dev, relu))
    assert names == PASSES
    check_against_float64(got, t, G, relu)
    again = run_op(t, G, dev, relu)
    for k, v in got.items():
        assert torch.equal(v, again[k]), k
    if shape[-1] <= 1024:  # the inference kernel's own bits
        with torch.no_grad():
            y = ops.group_norm(t["x"].to(dev), G, t["gamma"].to(dev), t["beta"].to(dev), 1e-5, relu)
        assert torch.equal(got["y"], y)


@pytest.mark.parametrize("relu", [False, True])
def test_toggle_selects_the_arm_and_the_arms_agree(dev, toggle, relu):
    """FUSED_GN_TRAIN is read where the arm is chosen: the records hold the two
    launches with it on and none with it off; the arms agree within the bar,
    every element compared.  y is compared as it comes.  With the ReLU an
    element whose z is within rounding of zero takes either side in two float32
    evaluations, and dx there differs by the whole dy * gamma * r: so the torch
    arm's gradients are taken under the mask the HIP arm used (its GroupNorm
    without the ReLU, fed dy where the HIP arm's y > 0; the gradient is linear
    in that), and the two masks may differ only where float64's z is within
    the bar of zero."""
    t = inputs((1, 67, 61, 64), 22)
    toggle(True)
    hip, names = _recorded(lambda: run_op(t, 16, dev, relu))
    assert names == PASSES
    toggle(False)
    tor, names = _recorded(lambda: run_op(t, 16, dev, relu))
    assert names == []
    assert all(v.is_cuda for v in tor.values())
    ref.close(hip["y"], tor["y"], "y")
    if relu:
        flips = int(((hip["y"] > 0) != (tor["y"] > 0)).sum())
        z = ref.forward(t["x"], 16, t["gamma"], t["beta"], 1e-5)["z"]
        assert flips <= int((z.abs() <= ref.BAR * float(z.abs().max())).sum())
        masked = dict(t, dy=t["dy"] * (hip["y"] > 0).cpu())
        tor, names = _recorded(lambda: run_op(masked, 16, dev, False))
        assert names == []
    for k in ("dx", "dgamma", "dbeta"):
        ref.close(hip[k], tor[k], k)


@pytest.mark.parametrize("shape,G", [((3, 9, 11, 24), 2), ((70, 7, 7, 256), 32)])
def test_needs_input_grad_selects_the_outputs(dev, toggle, shape, G):
    """A frozen affine gives dx only, a leaf input dgamma / dbeta only: the
    other results are None and the present ones have the full call's bits."""
    toggle(True)
    t = inputs(shape, 23)
    full = run_op(t, G, dev, True)
    frozen, names = _recorded(lambda: run_op(t, G, dev, True, grads=(True, False, False)))
    assert names == PASSES
    assert frozen["dgamma"] is None and frozen["dbeta"] is None
    assert torch.equal(frozen["dx"], full["dx"])
    leaf = run_op(t, G, dev, True, grads=(False, True, True))
    assert leaf["dx"] is None
    assert torch.equal(leaf["dgamma"], full["dgamma"]) and torch.equal(leaf["dbeta"], full["dbeta"])
    half = run_op(t, G, dev, True, grads=(False, True, False))
    assert half["dx"] is None and half["dbeta"] is None
    assert torch.equal(half["dgamma"], full["dgamma"])


def test_refused_size_takes_the_torch_arm_and_no_images_launch_nothing(dev, toggle):
    toggle(True)
    t = inputs((3, 4, 5, 6), 24)  # C / G = 2
    got, names = _recorded(lambda: run_op(t, 3, dev, True))
    assert names == []
    check_against_float64(got, t, 3, True)
    t = inputs((0, 5, 7, 8), 25)
    got, names = _recorded(lambda: run_op(t, 2, dev, True))
    assert names == []
    assert got["y"].shape == (0, 5, 7, 8) and got["dx"].shape == (0, 5, 7, 8)
    for k in ("dgamma", "dbeta"):
        assert got[k].shape == (8,) and not got[k].any(), k


def test_group_norm_through_conv2d(dev, toggle):
    """Conv2D with a GroupNorm and a ReLU: one gn_train_fwd takes both (the
    output equals conv -> float64 GroupNorm -> ReLU with no further pass), and
    the conv's weight gradient is that of the torch arm."""
    from detectron2_tensorflow_amd.layers import Conv2D, GroupNorm
    torch.manual_seed(5)
    conv = Conv2D(64, 64, 3, use_bias=False, activation="relu", normalizer=GroupNorm,
                  normalizer_params={"num_groups": 16}).to(dev)
    t = inputs((2, 12, 10, 64), 26)
    with torch.no_grad():
        conv.normalizer_fn.gamma.copy_(t["gamma"]); conv.normalizer_fn.beta.copy_(t["beta"])
    x, dy = t["x"].to(dev), t["dy"].to(dev)

    def run():
        conv.zero_grad(set_to_none=True)
        y = conv(x)
        y.backward(dy)
        return y.detach(), conv.weights.grad.clone(), conv.normalizer_fn.gamma.grad.clone()

    toggle(True)
    (y, dw, dg), names = _recorded(run)
    assert names == PASSES
    with torch.no_grad():
        raw = conv(x, raw=True)
    want = ref.forward(raw, 16, t["gamma"], t["beta"], 1e-5, relu=True)["y"]
    ref.close(y, want, "y")
    assert float(y.min()) == 0.0 and float(dw.abs().max()) > 0
    toggle(False)
    (y0, dw0, dg0), names = _recorded(run)
    assert names == []
    ref.close(y, y0, "y vs torch arm")
    ref.close(dw, dw0, "weight gradient")
    ref.close(dg, dg0, "gamma gradient")


def test_solo_trainer_step(dev, toggle):
    """One eager Trainer step of solo_v2_R_50_FPN at 256x320 on the HIP arm:
    finite losses, within the bar of the torch arm's step from the same
    weights and batch."""
    from test_solo import _cfg
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg = _cfg()
    models = []
    for _ in range(2):  # the same weights twice
        torch.manual_seed(0)
        models.append(build_model(cfg).to(dev).train())
    model, twin = models
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), twin.parameters()))
    batch = synthetic_train_batch(2, 256, 320, 5, dev, num_classes=80, sqrt_area=(24.0, 200.0),
                                  full_mask_hw=(256, 320))
    toggle(True)
    losses, names = _recorded(lambda: Trainer(cfg, model).step(batch))
    assert "gn_train_fwd" in names and "gn_train_bwd" in names
    toggle(False)
    base, names = _recorded(lambda: Trainer(cfg, twin).step(batch))
    assert names == []
    _C.raise_on_errors(dev)
    assert set(losses) == set(base)
    for k, v in losses.items():
        v, b = float(v), float(base[k])
        print(k, v, b)
        assert v == v and abs(v) != float("inf"), (k, v)
        assert abs(v - b) <= ref.BAR * abs(b), (k, v, b)


@pytest.mark.parametrize("fused", [True, False])
def test_mask_rcnn_gn_trainer_step_on_either_arm(dev, toggle, fused):
    """One eager Trainer step of Misc/mask_rcnn_R_50_FPN_3x_gn at 256x320: its
    FPN levels come out of a GroupNorm and are read by the RPN head and the
    ROI poolers, whose per-level gradient hand-off (handoff.Pair, tagged on the
    tensor object) has to close on the HIP arm (contiguous outputs) and to be
    left to autograd on the torch arm (permuted views, which the pooler
    copies): the step ends without a HandoffError, with finite losses."""
    import os
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(root, "configs/Misc/mask_rcnn_R_50_FPN_3x_gn.yaml"))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    finalize(cfg, training=True, world_size=1,
             category_map={"num_thing_classes": 80, "num_stuff_classes": 53,
                           "stuff_ignore_value": 0})
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 0, dev)
    calibrate_rcnn_scores(model, batch)
    toggle(fused)
    losses, names = _recorded(lambda: Trainer(cfg, model).step(batch))
    _C.raise_on_errors(dev)
    assert ("gn_train_bwd" in names) == fused and ("gn_train_fwd" in names) == fused
    for k, v in losses.items():
        assert torch.isfinite(torch.as_tensor(v)).all(), (k, v)
