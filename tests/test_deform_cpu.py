"""CPU tests of the deformable-conv feature: the public surface
(layers.DeformConv2D / ModulatedDeformConv2D, the dconv configs building,
checkpoint names), the host-side argument checks of the two new ABI calls, and
the known-answer tests of the restatement the GPU tests compare against
(tests/deform_reference.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}


def _build(rel):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", rel))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    finalize(cfg, training=False, world_size=1, category_map=CATS)
    return cfg, build_model(cfg)


def test_layers_are_exported():
    from detectron2_tensorflow_amd import layers
    assert "DeformConv2D" in layers.__all__ and "ModulatedDeformConv2D" in layers.__all__
    assert layers.DeformConv2D.__arg_scope_enabled__


def test_parameter_names_and_shapes():
    from detectron2_tensorflow_amd.layers import DeformConv2D
    m = DeformConv2D(16, 24, 3, deform_num_groups=2, scope="conv2")
    got = {k: tuple(v.shape) for k, v in m.reference_variables()}
    assert got == {"conv2/weights": (3, 3, 16, 24), "conv2/bias": (24,),
                   "conv2/offset_weights": (3, 3, 16, 36), "conv2/offset_bias": (36,)}
    for t in (m.offset_weights, m.offset_bias, m.bias):  # zero-initialised (:311, :355, :364)
        assert float(t.detach().abs().max()) == 0.0
    assert all(p.requires_grad for p in m.parameters())
    frozen = DeformConv2D(16, 24, 3, use_bias=False, trainable=False, scope="c")
    assert sorted(k for k, _ in frozen.reference_variables()) == [
        "c/offset_bias", "c/offset_weights", "c/weights"]
    assert not any(p.requires_grad for p in frozen.parameters())
    # arg-scope aware
    from detectron2_tensorflow_amd.utils.arg_scope import arg_scope
    with arg_scope([DeformConv2D], use_bias=False):
        assert DeformConv2D(8, 8, 3).bias is None


def test_unsupported_variants_raise():
    from detectron2_tensorflow_amd.layers import DeformConv2D, ModulatedDeformConv2D
    with pytest.raises(NotImplementedError, match="cannot be constructed or called"):
        ModulatedDeformConv2D(8, 8, 3)
    with pytest.raises(NotImplementedError, match="grouped deformable"):
        DeformConv2D(8, 8, 3, num_groups=2)
    with pytest.raises(ValueError, match="deform_num_groups"):
        DeformConv2D(6, 8, 3, deform_num_groups=4)
    # no CPU fall-back
    with pytest.raises(ValueError, match="GPU"):
        DeformConv2D(8, 8, 3)(torch.zeros(1, 5, 5, 8))


def test_dconv_config_builds_with_reference_variable_names():
    from detectron2_tensorflow_amd.checkpoint.loader import load_reference_weights
    from detectron2_tensorflow_amd.layers import DeformConv2D
    cfg, model = _build("Misc/mask_rcnn_R_50_FPN_1x_dconv_c3-c5.yaml")
    _, plain = _build("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_1x.yaml")
    got = {k: tuple(v.shape) for k, v in model.reference_variables(include_scope=False)}
    want = {k: tuple(v.shape) for k, v in plain.reference_variables(include_scope=False)}
    for stage, blocks, b in (("res3", 4, 128), ("res4", 6, 256), ("res5", 3, 512)):
        for i in range(1, blocks + 1):
            want[f"backbone/{stage}/block_{i}/conv2/offset_weights"] = (3, 3, b, 18)
            want[f"backbone/{stage}/block_{i}/conv2/offset_bias"] = (18,)
    assert got == want
    assert sum(isinstance(m, DeformConv2D) for m in model.modules()) == 13
    rng = np.random.default_rng(0)
    tensors = {k: rng.normal(size=s).astype(np.float32) for k, s in want.items()}
    assert load_reference_weights(model, tensors, strict=True) == ([], [])
    name = "backbone/res4/block_3/conv2/offset_weights"
    assert np.array_equal(dict(model.reference_variables(include_scope=False))[name].detach().numpy(),
                          tensors[name])


def test_dconv_3x_config_builds_and_modulated_raises():
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    _build("Misc/mask_rcnn_R_50_FPN_3x_dconv_c3-c5.yaml")
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "Misc",
                                     "mask_rcnn_R_50_FPN_1x_dconv_c3-c5.yaml"))
    cfg.MODEL.RESNETS.DEFORM_MODULATED = True
    finalize(cfg, training=False, world_size=1, category_map=CATS)
    with pytest.raises(NotImplementedError, match="cannot be constructed or called"):
        build_model(cfg)


def test_host_side_argument_errors_raise_without_gpu():
    """Argument validation happens on the host before any launch."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    # N H W C G k stride rate pb pe off_stride
    rc = lib.d2mi_deform_sample_fwd(None, None, 1, 8, 8, 6, 1, 3, 1, 1, 1, 1, 18, None, None)
    assert rc < 0 and "multiple of 4" in _C.last_error()
    rc = lib.d2mi_deform_sample_fwd(None, None, 1, 8, 8, 8, 1, 2, 1, 1, 1, 1, 8, None, None)
    assert rc < 0 and "kernel size 2" in _C.last_error()
    rc = lib.d2mi_deform_sample_bwd(None, None, None, 1, 8, 8, 12, 2, 3, 1, 1, 1, 1, 36, 36, None,
                                    None, None, 0, None)
    assert rc < 0 and "multiple of 4" in _C.last_error()
    rc = lib.d2mi_deform_sample_bwd(None, None, None, 1, 8, 8, 8, 1, 2, 1, 1, 1, 1, 8, 8, None,
                                    None, None, 0, None)
    assert rc < 0 and "kernel size 2" in _C.last_error()
    rc = lib.d2mi_deform_sample_fwd(None, None, 1, 8, 8, 8, 3, 3, 1, 1, 1, 1, 54, None, None)
    assert rc < 0 and "divisible" in _C.last_error()
    rc = lib.d2mi_deform_sample_fwd(None, None, 1, 8, 8, 8, 1, 3, 0, 1, 1, 1, 18, None, None)
    assert rc < 0 and "stride and rate" in _C.last_error()
    rc = lib.d2mi_deform_sample_fwd(None, None, 1 << 12, 1 << 10, 1 << 10, 8, 1, 3, 1, 1, 1, 1, 18,
                                    None, None)
    assert rc < 0 and "32-bit" in _C.last_error()
    assert lib.d2mi_deform_sample_bwd_workspace_size(1, 8, 8, 8, 1, 2, 1, 1, 1, 1) == 0
    assert lib.d2mi_deform_sample_bwd_workspace_size(1, 8, 8, 8, 1, 3, 1, 1, 1, 1) > 0


# ---------------------------------------------- the restatement's own KATs
def _x(shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=shape).astype(np.float32))


@pytest.mark.parametrize("stride,rate,groups", [(1, 1, 1), (2, 1, 2), (1, 2, 1)])
def test_restatement_zero_offsets_is_im2col(stride, rate, groups):
    x = _x((2, 7, 9, 8))
    want = ref.im2col(x, 3, stride, rate, "SAME")
    off = torch.zeros(want.shape[:3] + (2 * groups * 9,))
    assert torch.equal(ref.deform_cols(x, off, 3, stride, rate, "SAME", groups), want)
    assert torch.equal(ref.deform_cols(x, off, 3, stride, rate, "SAME", groups, torch.float64),
                       want.double())


def test_restatement_integer_offsets_is_shifted_im2col():
    # stride 3 VALID on 11x11: base taps reach 8, the shifted ones 9 < Hp - 1 = 10
    x = _x((1, 11, 11, 8), 1)
    want = ref.im2col(x, 3, 3, 1, "VALID", shift=(1, 1))
    off = torch.ones(want.shape[:3] + (18,))
    assert torch.equal(ref.deform_cols(x, off, 3, 3, 1, "VALID"), want)
    # per-group shifts: group 0 by (1, 0), group 1 by (0, 1)
    off = torch.zeros(want.shape[:3] + (2, 9, 2))
    off[..., 0, :, 0] = 1.0
    off[..., 1, :, 1] = 1.0
    got = ref.deform_cols(x, off.reshape(want.shape[:3] + (36,)), 3, 3, 1, "VALID", groups=2)
    a = ref.im2col(x, 3, 3, 1, "VALID", shift=(1, 0)).reshape(1, 3, 3, 9, 8)
    b = ref.im2col(x, 3, 3, 1, "VALID", shift=(0, 1)).reshape(1, 3, 3, 9, 8)
    assert torch.equal(got.reshape(1, 3, 3, 9, 8), torch.cat([a[..., :4], b[..., 4:]], -1))


def test_restatement_last_row_is_zero_under_valid():
    """y == Hp - 1 exactly: y0 == y1 == Hp - 1 and all four weights are 0
    (convolutional.py:76-79, :101-105) -- what a clipped sample gets."""
    x = _x((1, 6, 7, 8), 2).abs() + 1.0
    OH, OW = 4, 5
    off = torch.zeros(1, OH, OW, 9, 2)
    off[..., 0] = 100.0  # every tap clipped to the last row
    cols = ref.deform_cols(x, off.reshape(1, OH, OW, 18), 3, 1, 1, "VALID")
    assert float(cols.abs().max()) == 0.0
    # and with zero offsets only the taps ON the last row / column vanish
    cols = ref.deform_cols(x, torch.zeros(1, OH, OW, 18), 3, 1, 1, "VALID").reshape(1, OH, OW, 9, 8)
    plain = ref.im2col(x, 3, 1, 1, "VALID").reshape(1, OH, OW, 9, 8)
    assert torch.equal(cols[:, :OH - 1, :OW - 1], plain[:, :OH - 1, :OW - 1])
    assert float(cols[:, OH - 1, :, 6:].abs().max()) == 0.0  # kh = 2 at the last output row
    assert float(plain[:, OH - 1, :, 6:].abs().min()) > 0.0


def test_restatement_gradients_follow_the_clip_and_the_corners():
    """float64 autograd: a clipped sample passes no offset gradient, an
    interior one passes sum_c g_c * (-(x1-x)p0 - (x-x0)p1 + (x1-x)p2 + (x-x0)p3)."""
    x = _x((1, 5, 5, 4), 3).double()
    off = torch.zeros(1, 5, 5, 1, 2, dtype=torch.float64)
    off[0, 2, 2, 0] = torch.tensor([0.25, 0.5])
    off[0, 0, 0, 0] = torch.tensor([-3.0, 0.5])  # y clipped at 0
    off.requires_grad_(True)
    cols = ref.deform_cols(x, off.reshape(1, 5, 5, 2), 1, 1, 1, "VALID", 1, torch.float64)
    g = _x((1, 5, 5, 4), 4).double()
    (cols * g).sum().backward()
    p0, p1, p2, p3 = x[0, 2, 2], x[0, 2, 3], x[0, 3, 2], x[0, 3, 3]
    gy = (g[0, 2, 2] * (-0.5 * p0 - 0.5 * p1 + 0.5 * p2 + 0.5 * p3)).sum()
    gx = (g[0, 2, 2] * (-0.75 * p0 + 0.75 * p1 - 0.25 * p2 + 0.25 * p3)).sum()
    assert torch.allclose(off.grad[0, 2, 2, 0], torch.stack([gy, gx]), rtol=1e-12, atol=1e-12)
    assert float(off.grad[0, 0, 0, 0, 0]) == 0.0 and float(off.grad[0, 0, 0, 0, 1]) != 0.0
