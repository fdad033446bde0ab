"""The single-level RPN of the C4 / DC5 families with the anchors its configs
ship (5 sizes x 3 aspect ratios = 15 per cell) on the GPU: anchors and
proposals against the oracle, the 76-column skinny weight gradient against
float64, the fused head at A = 15, the pre-NMS top-k above 8,192 candidates,
and the shipped configs end to end."""
import os

import numpy as np
import pytest
import torch

import oracle
import res5_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SIZES, RATIOS = [32, 64, 128, 256, 512], [0.5, 1.0, 2.0]


def _ops():
    from detectron2_tensorflow_amd.layers import ops
    return ops


def _cell15():
    cell = oracle.generate_cell_anchors(SIZES, RATIOS)
    assert cell.shape == (15, 4)
    return cell


def assert_boxes_close(got, want):
    """|got - want| <= max(1e-4, 2 ulp of the box's largest coordinate): the bar
    of test_gpu_ops.assert_boxes_close (expf is not correctly rounded on either
    side)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    scale = np.abs(want).max(axis=-1, keepdims=True) if want.size else want
    tol = np.maximum(F32(1e-4), 2 * np.spacing(scale.astype(F32)))
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{bad.sum()} coords off: got {got[bad][:5]} want {want[bad][:5]}"


def _proposals_vs_oracle(dev, pre, post, min_size, strides, hw, cells, logits, deltas, image_hw):
    """The assertions of test_gpu_ops._rpn_proposals_vs_oracle."""
    N = logits[0].shape[0]
    props = []
    for (h, w), s, c, d in zip(hw, strides, cells, deltas):
        anc = oracle.grid_anchors(h, w, s, c)
        props.append(oracle.apply_deltas(d.reshape(-1, 4), np.tile(anc, (N, 1)), (1, 1, 1, 1))
                     .reshape(N, -1, 4))
    wb, ws, wv = oracle.find_top_rpn_proposals(props, [l.reshape(N, -1) for l in logits],
                                               image_hw, 0.7, pre, post, min_size)
    gb, gs, gv = _ops().rpn_proposals([torch.from_numpy(l).to(dev) for l in logits],
                                      [torch.from_numpy(d).to(dev) for d in deltas], strides,
                                      [torch.from_numpy(c) for c in cells],
                                      torch.from_numpy(image_hw).to(dev), pre, post, 0.7, min_size)
    np.testing.assert_array_equal(gv.cpu().numpy(), wv)
    np.testing.assert_array_equal(gs.cpu().numpy(), ws)
    # bit for bit: a -0.0 logit stays a -0.0 score
    np.testing.assert_array_equal(gs.cpu().numpy().view(np.int32), ws.astype(F32).view(np.int32))
    assert_boxes_close(gb.cpu().numpy(), wb)
    return wv


# ------------------------------------------------------------------ anchors
def test_grid_anchors_with_15_cell_anchors_match_the_oracle(dev):
    cell = _cell15()
    got = _ops().grid_anchors(5, 7, 16, torch.from_numpy(cell), dev).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.grid_anchors(5, 7, 16, cell))


def test_rpn_proposals_with_15_anchors_match_the_oracle(dev):
    rng = np.random.default_rng(41)
    N, H, W, A = 2, 6, 9, 15
    logits = [rng.normal(size=(N, H, W, A)).astype(F32)]
    deltas = [rng.normal(0, 0.3, size=(N, H, W, A * 4)).astype(F32)]
    image_hw = np.array([[96 - 7, 144], [96, 144 - 20]], np.int32)
    wv = _proposals_vs_oracle(dev, 200, 50, 0.0, [16], [(H, W)], [_cell15()], logits, deltas,
                              image_hw)
    assert wv.any()


# ---------------------------------------------------- wide weight gradient
def _xg(dev, P, Cin, Cout, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(P, Cin, device=dev, generator=g),
            torch.randn(P, Cout, device=dev, generator=g))


def _wgrad_close(gw, gb, x, g):
    """The project's bar for this quantity (the fused RPN head's test):
    rtol 1e-4, atol 1e-5 of the reference's largest entry, against float64."""
    rw = x.double().t() @ g.double()
    rb = g.double().sum(0)
    torch.testing.assert_close(gw[0, 0].double(), rw, rtol=1e-4, atol=1e-5 * rw.abs().max().item())
    torch.testing.assert_close(gb.double(), rb, rtol=1e-4, atol=1e-5 * rb.abs().max().item())


# Cin 4: one live lane; 260: a second 256-channel pass with one live lane; P 1,
# 127 / 129: a one-pixel chunk and a chunk tail; Cout 17 / 20: a second column
# block of 1 / 4 columns; 76: the 15-anchor head's five blocks, the last of 12
@pytest.mark.parametrize("Cin,Cout,P", [(4, 17, 1), (260, 20, 127), (1024, 17, 129),
                                        (260, 76, 129), (1024, 76, 300)])
def test_wide_skinny_wgrad_matches_float64(dev, Cin, Cout, P):
    x, g = _xg(dev, P, Cin, Cout, 7)
    gw, gb = _ops().wgrad_skinny(x, g)
    assert gw.shape == (1, 1, Cin, Cout) and gb.shape == (Cout,)
    _wgrad_close(gw, gb, x, g)
    gw2, gb2 = _ops().wgrad_skinny(x, g)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)  # fixed summation order


def test_wide_skinny_wgrad_unaligned_input_takes_the_scalar_kernel(dev):
    """Cin % 4 != 0: the one-channel-per-thread kernel, over column blocks too."""
    x, g = _xg(dev, 129, 270 + 1, 76, 8)
    gw, gb = _ops().wgrad_skinny(x, g)
    _wgrad_close(gw, gb, x, g)


def test_wide_skinny_wgrad_accumulates_old_plus_new(dev):
    x1, g1 = _xg(dev, 300, 260, 76, 9)
    x2, g2 = _xg(dev, 129, 260, 76, 10)
    first = _ops().wgrad_skinny(x1, g1)
    second = _ops().wgrad_skinny(x2, g2)
    want = (first[0] + second[0], first[1] + second[1])  # float32: old + new
    acc = _ops().wgrad_skinny(x2, g2, accumulate_into=(first[0].clone(), first[1].clone()))
    assert torch.equal(acc[0], want[0]) and torch.equal(acc[1], want[1])


def test_wide_skinny_wgrad_levels_equal_the_per_level_calls(dev):
    """Two levels in one launch pair: bit-identical to one call per level with
    accumulate_into after the first -- what the 16-column route guarantees."""
    lv = [_xg(dev, 300, 260, 76, 11), _xg(dev, 129, 260, 76, 12)]
    gw, gb = _ops().wgrad_skinny_levels([x for x, _ in lv], [g for _, g in lv])
    buf = None
    for x, g in lv:
        buf = _ops().wgrad_skinny(x, g, accumulate_into=buf)
    assert torch.equal(gw, buf[0]) and torch.equal(gb, buf[1])
    xs, gs = torch.cat([x for x, _ in lv]), torch.cat([g for _, g in lv])
    _wgrad_close(gw, gb, xs, gs)


@pytest.mark.parametrize("Cout", [3, 16])
def test_narrow_skinny_wgrad_is_unchanged_in_kind(dev, Cout):
    x, g = _xg(dev, 300, 260, Cout, 13)
    gw, gb = _ops().wgrad_skinny(x, g)
    gw2, gb2 = _ops().wgrad_skinny(x, g)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    _wgrad_close(gw, gb, x, g)


# ------------------------------------------------------ fused head, A = 15
def _c4_cfg(name, training, family="COCO-InstanceSegmentation"):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", family, name + ".yaml"))
    if hasattr(cfg.MODEL, "SEGMENTATION_OUTPUT"):
        cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    finalize(cfg, training, 1, ref.CATS)
    return cfg


def test_rpn_head_fused_1x1_with_15_anchors_matches_float64(dev):
    """test_rpn_head_fused_1x1_matches_separate_convs on the C4 head: 15
    anchors, a 76-wide fused 1x1 (75 + a zero pad column), one level."""
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import StandardRPNHead
    cfg = _c4_cfg("mask_rcnn_R_50_C4_1x", True)
    torch.manual_seed(0)
    C = 64
    head = StandardRPNHead(cfg, [ShapeSpec(channels=C, stride=16)]).to(dev)
    assert head.A == 15
    with torch.no_grad():  # non-trivial biases / weights
        for c in (head.objectness_logits, head.anchor_deltas):
            c.weights.normal_(0, 0.05)
            c.bias.normal_(0, 0.1)
    xs = [torch.randn(2, 6, 8, C, device=dev)]
    for x in xs:
        x.requires_grad_(True)
    _, logits, deltas = head(xs)
    assert [tuple(t.shape) for t in logits] == [(2, 6, 8, 15)]
    assert [tuple(t.shape) for t in deltas] == [(2, 6, 8, 60)]
    gl = [torch.randn_like(t) for t in logits]
    gd = [torch.randn_like(t) for t in deltas]
    torch.autograd.backward(logits + deltas, gl + gd)
    wo, bo = head.objectness_logits.weights, head.objectness_logits.bias
    wd, bd = head.anchor_deltas.weights, head.anchor_deltas.bias
    # float64 reference of the same graph
    x64 = [x.detach().double().requires_grad_(True) for x in xs]
    share = [torch.relu(torch.nn.functional.conv2d(
        x.permute(0, 3, 1, 2), head.conv.weights.detach().double().permute(3, 2, 0, 1),
        head.conv.bias.detach().double(), padding=1)).permute(0, 2, 3, 1) for x in x64]
    ref_l = [s @ wo.detach().double()[0, 0] + bo.detach().double() for s in share]
    ref_d = [s @ wd.detach().double()[0, 0] + bd.detach().double() for s in share]
    torch.autograd.backward(ref_l + ref_d, [t.double() for t in gl + gd])
    share = [s.detach() for s in share]
    gwo = sum(s.reshape(-1, C).t() @ g.double().reshape(-1, g.shape[-1]) for s, g in zip(share, gl))
    gwd = sum(s.reshape(-1, C).t() @ g.double().reshape(-1, g.shape[-1]) for s, g in zip(share, gd))
    for lg, dl, rl, rd in zip(logits, deltas, ref_l, ref_d):
        torch.testing.assert_close(lg.double(), rl.detach(), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(dl.double(), rd.detach(), rtol=1e-4, atol=1e-4)
    tol = lambda r: dict(rtol=1e-4, atol=1e-5 * r.abs().max().item())
    torch.testing.assert_close(wo.grad[0, 0].double(), gwo, **tol(gwo))
    torch.testing.assert_close(wd.grad[0, 0].double(), gwd, **tol(gwd))
    gbo = sum(g.double().reshape(-1, g.shape[-1]).sum(0) for g in gl)
    gbd = sum(g.double().reshape(-1, g.shape[-1]).sum(0) for g in gd)
    torch.testing.assert_close(bo.grad.double(), gbo, **tol(gbo))
    torch.testing.assert_close(bd.grad.double(), gbd, **tol(gbd))
    for x, r in zip(xs, x64):
        torch.testing.assert_close(x.grad.double(), r.grad, **tol(r.grad))


# ------------------------------------------------------------ wide top-k
WIDE_HW, WIDE_A = (24, 24), 15   # 8,640 anchors: above the radix select's 8,192


@pytest.fixture(scope="module")
def wide_inputs():
    rng = np.random.default_rng(43)
    N, (H, W), A = 2, WIDE_HW, WIDE_A
    logits = rng.normal(size=(N, H, W, A)).astype(F32)
    deltas = rng.normal(0, 0.3, size=(N, H, W, A * 4)).astype(F32)
    image_hw = np.array([[384 - 17, 384], [384, 384 - 40]], np.int32)
    return logits, deltas, image_hw


def _wide_logits(kind, logits):
    logits = logits.copy()
    if kind == "tied":
        # 64 distinct values: ties cross the k boundary and the sort's 8,192-key tiles
        logits = np.clip(np.round(logits * 8) / 8, -4.0, 3.875).astype(F32)
        assert len(np.unique(logits)) <= 64
    if kind == "nonfinite":
        flat = logits[1].reshape(-1)
        pick = np.random.default_rng(44).permutation(flat.size)[:103]
        flat[pick[:100]] = -np.inf
        flat[pick[100:]] = np.nan
    return logits


@pytest.mark.parametrize("kind,pre", [("normal", 12000), ("tied", 12000), ("normal", 8500),
                                      ("tied", 8500), ("nonfinite", 12000),
                                      ("nonfinite", 8500)])
def test_rpn_proposals_above_8192_candidates_match_the_oracle(dev, wide_inputs, kind, pre):
    """k = min(pre, 8640) > 8192: the sort route.  Kept boxes and validity
    exact, scores bit-equal (the bar of test_rpn_proposals_baseline_geometry);
    pre = 8500 < 8640 makes a true selection above the cap; NaN / -inf are never
    selected."""
    base, deltas, image_hw = wide_inputs
    logits = _wide_logits(kind, base)
    assert min(pre, logits[0].size) > 8192
    wv = _proposals_vs_oracle(dev, pre, 300, 0.0, [16], [WIDE_HW], [_cell15()], [logits],
                              [deltas], image_hw)
    assert wv.sum() > 300  # both images contribute


# ------------------------------------------------------------ end to end
def _build(cfg, dev, train):
    from detectron2_tensorflow_amd.modeling import build_model
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    model = model.train() if train else model.eval()
    ag = model.proposal_generator.anchor_generator
    assert list(ag.num_cell_anchors) == [15]  # the shipped anchors, not an override
    return model


@pytest.mark.parametrize("family,name,keys", [
    ("COCO-InstanceSegmentation", "mask_rcnn_R_50_C4_1x",
     {"loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc", "total_loss"}),
    ("COCO-Detection", "faster_rcnn_R_50_DC5_1x",
     {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "total_loss"})])
def test_shipped_single_level_configs_train_a_step_and_infer(dev, family, name, keys):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg = _c4_cfg(name, True, family)
    model = _build(cfg, dev, True)
    batch = synthetic_train_batch(2, 192, 256, 0, dev)
    w = model.proposal_generator.rpn_head.anchor_deltas.weights
    assert w.shape[-1] == 60
    before = w.detach().clone()
    losses = {k: float(v.detach()) for k, v in Trainer(cfg, model).step(batch).items()}
    _C.raise_on_errors(dev)
    print(losses)
    assert set(losses) == keys
    assert all(np.isfinite(v) and v >= 0 for v in losses.values())
    assert not torch.equal(w.detach(), before)
    model.eval()
    with torch.no_grad():
        out = model.inference({"image": batch["image"], "image_shape": batch["image_shape"]})
    inst = out["instances"]
    D = cfg.TEST.DETECTIONS_PER_IMAGE
    assert inst["boxes"].shape == (2, D, 4) and torch.isfinite(inst["boxes"]).all()
    if "loss_mask" in keys:
        assert inst["masks"].shape == (2, D, 14, 14) and torch.isfinite(inst["masks"]).all()
    _C.raise_on_errors(dev)


def test_shipped_c4_proposal_network_infers(dev):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg = _c4_cfg("rpn_R_50_C4_1x", False, "COCO-Detection")
    model = _build(cfg, dev, False)
    batch = synthetic_train_batch(2, 192, 256, 0, dev)
    with torch.no_grad():
        out = model({"image": batch["image"], "image_shape": batch["image_shape"]})
    _C.raise_on_errors(dev)
    props = out["proposals"]
    post = cfg.MODEL.RPN.POST_NMS_TOPK_TEST
    assert props["boxes"].shape == (2, post, 4) and torch.isfinite(props["boxes"]).all()
    assert props["is_valid"].shape == (2, post) and props["is_valid"].any()
