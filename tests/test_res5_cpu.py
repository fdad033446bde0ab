"""The C4 model family without a GPU: every C4 config builds, the head carries
the converter's C4 variable names, its constructor follows the reference, the
tensor formulation of the pool / gather and its autograd equal float64, and a
CPU training forward of a narrow head matches the float64 restatement of the
reference (tests/res5_reference.py) within the README's 1e-4."""
import ctypes
import os

import numpy as np
import pytest
import torch

import res5_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
C4_CONFIGS = ["COCO-Detection/faster_rcnn_R_50_C4_1x.yaml",
              "COCO-Detection/faster_rcnn_R_50_C4_3x.yaml",
              "COCO-Detection/faster_rcnn_R_101_C4_3x.yaml",
              "COCO-InstanceSegmentation/mask_rcnn_R_50_C4_1x.yaml",
              "COCO-InstanceSegmentation/mask_rcnn_R_50_C4_3x.yaml",
              "COCO-InstanceSegmentation/mask_rcnn_R_101_C4_3x.yaml",
              "PascalVOC-Detection/faster_rcnn_R_50_C4.yaml"]
MASK_C4 = "COCO-InstanceSegmentation/mask_rcnn_R_50_C4_1x.yaml"


def _build(yaml, extra=(), cats=ref.CATS):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    path = os.path.join(ROOT, "configs", yaml)
    if yaml.startswith("PascalVOC"):
        # a detectron2 leftover the reference's own loader rejects too (it sets
        # MODEL.WEIGHTS and INPUT.*, tests/test_configs.py): its base and the
        # model keys it sets, which are all that shape the network
        with pytest.raises(KeyError):
            cfg.merge_from_file(path)
        cfg = get_cfg()
        cfg.merge_from_file(os.path.join(ROOT, "configs", "Base-RCNN-C4.yaml"))
        extra = ["MODEL.MASK_ON", False, "MODEL.RESNETS.DEPTH", 50] + list(extra)
        cats = dict(cats, num_thing_classes=20)
    else:
        cfg.merge_from_file(path)
    cfg.merge_from_list(list(extra))
    finalize(cfg, False, 1, cats)
    torch.manual_seed(0)
    return cfg, build_model(cfg)


@pytest.mark.parametrize("yaml", C4_CONFIGS)
def test_c4_configs_build(yaml):
    from detectron2_tensorflow_amd.modeling import Res5ROIHeads
    cfg, model = _build(yaml)
    rh = model.roi_heads
    assert type(rh) is Res5ROIHeads and rh.in_features == ["res4"]
    assert len(rh.res5.blocks) == 3 and rh.out_channels == 2048
    b1 = rh.res5.blocks[0]
    assert (b1.conv1.stride, b1.conv2.stride, b1.shortcut.stride) == (2, 1, 2)
    assert (b1.conv1.in_channels, b1.conv1.out_channels, b1.conv3.out_channels) == (1024, 512, 2048)
    assert rh.pooler.output_size == (14, 14) and rh.pooler.scales == [1.0 / 16]
    assert rh.half_pooler.output_size == (7, 7) and rh.elides() == rh.ELIDE_STRIDE
    assert rh.mask_on == cfg.MODEL.MASK_ON == ("mask_rcnn" in yaml)
    assert hasattr(rh, "mask_head") == rh.mask_on
    K = 20 if yaml.startswith("PascalVOC") else 80
    names = {n: tuple(t.shape) for n, t in model.reference_variables(include_scope=False)}
    assert names["roi_heads/fastrcnn/class_logits/weights"] == (2048, K + 1)
    assert names["roi_heads/fastrcnn/box_deltas/weights"] == (2048, 4 * K)
    # res5 lives in the head, not in the backbone
    assert not [n for n in names if n.startswith("backbone/res5")]


def test_model_carries_the_converter_names_of_the_c4_case():
    """Every output key of the golden file's C4 case (class-agnostic boxes,
    ROI_MASK_HEAD.NUM_CONV 4 -- the two head settings of that case that change
    the variable list) is a variable of the built mask_rcnn_R_50_C4_1x; with
    the config as shipped (NUM_CONV 0) all but the four mask_fcn convs are."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "convert_d2_golden.npz"))
    pre = "mask_rcnn_R_50_C4_agnostic|out|"
    want = [k[len(pre):] for k in z.files if k.startswith(pre)]
    assert len(want) > 250 and "roi_heads/res5/block_3/conv3/norm/moving_mean" in want
    _, model = _build(MASK_C4, ["MODEL.ROI_MASK_HEAD.NUM_CONV", 4,
                                "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True])
    names = {n: tuple(t.shape) for n, t in model.reference_variables(include_scope=False)}
    assert not [k for k in want if k not in names]
    # class-agnostic regressor with MASK_ON: the predictor shapes
    assert names["roi_heads/fastrcnn/box_deltas/weights"] == (2048, 4)
    assert names["roi_heads/fastrcnn/box_deltas/bias"] == (4,)
    assert names["roi_heads/fastrcnn/class_logits/weights"] == (2048, 81)
    assert names["roi_heads/mask_head/mask_fcn1/weights"] == (3, 3, 2048, 256)
    assert names["roi_heads/mask_head/deconv/weights"] == (2, 2, 256, 256)
    assert names["roi_heads/mask_head/predictor/weights"] == (1, 1, 256, 80)
    _, shipped = _build(MASK_C4)
    got = {n for n, _ in shipped.reference_variables(include_scope=False)}
    assert [k for k in want if k not in got] == [
        f"roi_heads/mask_head/mask_fcn{i}/{leaf}" for i in (1, 2, 3, 4)
        for leaf in ("weights", "bias")]


def test_constructor_refuses_a_deformable_res5_and_two_features():
    with pytest.raises(AssertionError, match="Deformable conv"):
        _build(MASK_C4, ["MODEL.RESNETS.DEFORM_ON_PER_STAGE", [False, False, False, True]])
    with pytest.raises(AssertionError):
        ref.narrow_head(ROOT, ["MODEL.ROI_HEADS.IN_FEATURES", ["res4", "res4"]])


def test_literal_path_settings_have_no_elision():
    for extra in (["MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2],
                  ["MODEL.RESNETS.STRIDE_IN_1X1", False],
                  ["MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7]):
        _, head = ref.narrow_head(ROOT, extra)
        assert head.half_pooler is None and not head.elides()
    _, head = ref.narrow_head(ROOT)
    assert head.half_pooler is not None
    head.ELIDE_STRIDE = False
    assert not head.elides()


def test_graphed_trainer_refuses_the_head_at_construction():
    from detectron2_tensorflow_amd.engine.graphed import GraphedTrainer
    cfg, model = _build(MASK_C4)
    with pytest.raises(NotImplementedError, match="Res5ROIHeads"):
        GraphedTrainer(cfg, model)


@pytest.mark.parametrize("R,P,C,M", [(5, 49, 16, 3), (1, 1, 4, 1), (7, 9, 12, 0), (6, 4, 8, None)])
def test_pool_gather_tensor_formulation_against_float64(R, P, C, M):
    from detectron2_tensorflow_amd.layers import ops
    g = torch.Generator().manual_seed(R * 100 + P)
    x = torch.randn(R, P, C, generator=g, dtype=F64, requires_grad=True)
    dst = None
    if M is not None:
        dst = torch.full((R,), -1, dtype=torch.int32)
        dst[torch.randperm(R, generator=g)[:M]] = torch.randperm(M, generator=g).to(torch.int32)
    pooled, y = ops.res5_pool_dense(x, dst, M or 0)
    want_p, want_y = ref.pool_gather(x.detach(), dst, M or 0)
    assert float((pooled.detach() - want_p).abs().max()) <= 1e-15
    assert (y is None) == (dst is None)
    gp = torch.randn(R, C, generator=g, dtype=F64)
    loss = (pooled * gp).sum()
    want_dx = (gp / P)[:, None, :].expand(R, P, C).clone()
    if dst is not None:
        assert torch.equal(y, want_y)
        gy = torch.randn(M, P, C, generator=g, dtype=F64)
        loss = loss + (y * gy).sum()
        for r, d in enumerate(dst.tolist()):
            if d >= 0:
                want_dx[r] += gy[d]
    loss.backward()
    assert float((x.grad - want_dx).abs().max()) <= 1e-15


def test_pool_entries_refuse_bad_arguments_without_gpu():
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers import ops
    lib = _C.load()
    a = ctypes.c_void_p(4096)  # aligned, never dereferenced: refused first
    for kw, word in (({"C": 6}, "C = 6"), ({"C": 0}, "C = 0"), ({"P": 0}, "P = 0")):
        s = dict(R=4, P=49, C=8)
        s.update(kw)
        rc = lib.d2mi_res5_pool_fwd(a, s["R"], s["P"], s["C"], a, 2, a, a, None)
        assert rc < 0 and word in _C.last_error(), (kw, _C.last_error())
        rc = lib.d2mi_res5_pool_bwd(a, a, a, s["R"], s["P"], s["C"], 2, a, None)
        assert rc < 0 and word in _C.last_error(), (kw, _C.last_error())
    rc = lib.d2mi_res5_pool_fwd(a, 4, 49, 8, None, 2, a, a, None)
    assert rc < 0 and "without dst" in _C.last_error()
    rc = lib.d2mi_res5_pool_fwd(ctypes.c_void_p(4100), 4, 49, 8, None, 0, a, None, None)
    assert rc < 0 and "16-byte aligned" in _C.last_error()
    assert lib.d2mi_res5_pool_fwd(None, 0, 49, 8, None, 0, None, None, None) == 0  # R = 0
    with pytest.raises(ValueError, match="MI355X only"):
        ops.res5_pool(torch.zeros(2, 4, 8))
    # the toggle has one owner and is not an attribute of the package
    assert ops.res5.FUSED_POOL in (True, False) and not hasattr(ops, "FUSED_POOL")


def _cpu_losses(head, feat, proposals, targets, shapes):
    head.train()
    f = feat.clone().requires_grad_(True)
    sampled, losses = head(ref.Images(shapes), {"res4": f}, proposals, targets)
    return sampled, losses, f


@pytest.mark.parametrize("elide", [True, False])
def test_cpu_training_forward_matches_the_float64_reference(elide):
    _, head = ref.narrow_head(ROOT)
    head.ELIDE_STRIDE = elide
    feat, proposals, targets, shapes = ref.make_case()
    sampled, losses, f = _cpu_losses(head, feat, proposals, targets, shapes)
    # every candidate was sampled: 12 valid rows per image, 3 of them foreground
    assert sampled["is_valid"].sum(1).tolist() == [12, 12]
    assert ((sampled["gt_classes"] < 5) & sampled["is_valid"]).sum(1).tolist() == [3, 3]
    assert head.last_mask_rows == 8  # 2 x int(16 * 0.25) slots < one bucket of 32
    f64 = feat.to(F64).requires_grad_(True)
    want, _ = ref.train_losses(head, f64, sampled, targets)
    assert set(losses) == set(want) == {"loss_cls", "loss_box_reg", "loss_mask"}
    for k in want:
        assert float(want[k]) > 1e-3, k
        assert abs(float(losses[k]) - float(want[k])) <= 1e-4, (k, float(losses[k]), float(want[k]))
    # the gradient reaches the feature map and every head parameter
    sum(losses.values()).backward()
    sum(want.values()).backward()
    assert float((f.grad.to(F64) - f64.grad).abs().max()) <= 1e-4 * max(1.0, float(f64.grad.abs().max()))
    for n, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_cpu_training_forward_with_an_image_without_foreground():
    _, head = ref.narrow_head(ROOT)
    feat, proposals, targets, shapes = ref.make_case(zero_fg_image=1)
    sampled, losses, _ = _cpu_losses(head, feat, proposals, targets, shapes)
    want, _ = ref.train_losses(head, feat.to(F64), sampled, targets)
    for k in want:
        assert abs(float(losses[k]) - float(want[k])) <= 1e-4, k
    # no foreground at all: one bucket of masked rows, a finite (zero) mask loss
    targets["is_valid"][:] = False
    sampled, losses, f = _cpu_losses(head, feat, proposals, targets, shapes)
    assert not ((sampled["gt_classes"] < 5) & sampled["is_valid"]).any()
    assert head.last_mask_rows == 8 and float(losses["loss_mask"]) == 0.0
    assert all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    assert torch.isfinite(f.grad).all()


def test_training_with_fixed_mask_rows_is_refused():
    """The mask rows are gathered fg-first from the shared res5 output; the
    fixed-row setting orders their targets by slot, so it is an error."""
    _, head = ref.narrow_head(ROOT)
    head.mask_compact_rows = False
    feat, proposals, targets, shapes = ref.make_case()
    with pytest.raises(NotImplementedError, match="compacted fg-first rows only"):
        _cpu_losses(head, feat, proposals, targets, shapes)


def test_faster_rcnn_c4_head_has_no_mask_branch():
    _, head = ref.narrow_head(ROOT, mask_on=False)
    feat, proposals, targets, shapes = ref.make_case()
    targets.pop("gt_masks")
    sampled, losses, _ = _cpu_losses(head, feat, proposals, targets, shapes)
    want, _ = ref.train_losses(head, feat.to(F64), sampled, targets)
    assert set(losses) == {"loss_cls", "loss_box_reg"}
    for k in want:
        assert abs(float(losses[k]) - float(want[k])) <= 1e-4, k
