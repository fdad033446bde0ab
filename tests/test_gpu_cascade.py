"""GPU tests of Cascade R-CNN: the fused stage hand-over (d2mi_cascade_refine)
against the composition of the existing device ops and against the
restatement built from the oracle (tests/cascade_reference.py), the
stage-averaged Fast R-CNN inference (d2mi_fast_rcnn_inference_stages) against
the single-stage pipeline and the oracle, CascadeROIHeads against a loop of
public pieces and the oracle's losses, and the two cascade configs as whole
models (inference, an eager step, a graph-replayed step)."""
import os
import types

import numpy as np
import pytest
import torch

import cascade_reference as cref
import oracle
import training as otrain
from test_gpu_ops import assert_boxes_close

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
CASCADE = os.path.join(ROOT, "configs", "Misc", "cascade_mask_rcnn_R_50_FPN_3x.yaml")
PANOPTIC_CASCADE = os.path.join(ROOT, "configs", "Misc",
                                "panoptic_fpn_R_101_dconv_cascade_gn_3x.yaml")
W1 = (10.0, 10.0, 5.0, 5.0)
INF = float("inf")


def _ops():
    from detectron2_tensorflow_amd.layers import ops
    return ops


# ---------------------------------------------------------------- the cases
def _random_case(seed, N, S, G):
    """Boxes scattered around the GT (so every label occurs), some invalid
    slots, invalid / crowd / difficult GT, int32 classes."""
    rng = np.random.default_rng(seed)
    image_hw = np.stack([rng.integers(180, 260, N), rng.integers(200, 300, N)], 1).astype(np.int32)
    c = rng.uniform([20, 20], [200, 240], size=(N, G, 2))
    hw = rng.uniform(16, 120, size=(N, G, 2))
    gt_boxes = np.concatenate([c - hw / 2, c + hw / 2], -1).astype(F32)
    pick = rng.integers(0, G, size=(N, S))
    boxes = gt_boxes[np.arange(N)[:, None], pick] + rng.normal(0, 12, size=(N, S, 4))
    boxes[..., 2:] = np.maximum(boxes[..., 2:], boxes[..., :2] + 1)
    far = rng.random((N, S)) < 0.1  # decoded far outside the image
    boxes[far] += 1000
    deltas = (rng.normal(size=(N * S, 4)) * [1.5, 1.5, 1.0, 1.0]).astype(F32)
    gt = {"gt_boxes": gt_boxes, "is_valid": rng.random((N, G)) < 0.8,
          "gt_classes": rng.integers(0, 80, (N, G)).astype(np.int32),
          "gt_is_crowd": rng.random((N, G)) < 0.15, "gt_difficult": rng.random((N, G)) < 0.15}
    return deltas, boxes.astype(F32), rng.random((N, S)) < 0.9, image_hw, gt


CASES = {"hand_made_2x70x5": cref.hand_made_case,
         "1x512x256": lambda: _random_case(1, 1, 512, 256),
         "3x257x1": lambda: _random_case(2, 3, 257, 1)}
_CACHE = {}


def _case(name):
    """The case's numpy arrays: made once, shared by the tests, never modified."""
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def _fused(dev, case, thr, training=True, masks=True):
    deltas, boxes, valid, image_hw, gt = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = {}
    if training:
        kw = dict(gt_boxes=t(gt["gt_boxes"]), gt_valid=t(gt["is_valid"]),
                  gt_classes=t(gt["gt_classes"]), iou_thr=thr, num_classes=80)
        if masks:
            kw.update(gt_crowd=t(gt["gt_is_crowd"]), gt_difficult=t(gt["gt_difficult"]))
    return _ops().cascade_refine(t(deltas), t(boxes), t(valid), t(image_hw), W1, **kw)


def _composed(dev, case, thr, training=True, masks=True):
    """The same outputs from the existing device ops: ops.apply_deltas, a
    clamp, ops.match_boxes_masks, gathers."""
    ops = _ops()
    deltas, boxes, valid, image_hw, gt = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    N, S = valid.shape
    dec = ops.apply_deltas(t(deltas), t(boxes).reshape(-1, 4), W1).reshape(N, S, 4)
    hw = t(image_hw).to(torch.float32)
    win = torch.stack([hw[:, 0], hw[:, 1], hw[:, 0], hw[:, 1]], 1)[:, None, :]
    out = torch.minimum(dec, win).clamp(min=0.0)
    if not training:
        return {"boxes": out, "is_valid": t(valid)}
    ok = t(valid) & ((out[..., 2] - out[..., 0]) * (out[..., 3] - out[..., 1]) > 0)
    matches, labels = ops.match_boxes_masks(
        t(gt["gt_boxes"]), t(gt["is_valid"]), out, [-INF, thr, INF], [0, 1], False,
        crowd=t(gt["gt_is_crowd"]) if masks else None,
        difficult=t(gt["gt_difficult"]) if masks else None, crowd_thr=1e-3, difficult_thr=thr)
    gcls = torch.gather(t(gt["gt_classes"]).long(), 1, matches)
    cls = torch.where(labels == 1, gcls, torch.where(labels == 0, 80, -1))
    cls = torch.where(ok, cls, -1)
    return {"boxes": out, "is_valid": ok, "gt_classes": cls, "gt_index": matches,
            "gt_boxes": torch.gather(t(gt["gt_boxes"]), 1, matches[..., None].expand(-1, -1, 4)),
            "loss_valid": ok & (cls >= 0)}


# ------------------------------------------------------- the refine kernel
@pytest.mark.parametrize("masks", [True, False], ids=["masks", "no_masks"])
@pytest.mark.parametrize("thr", [0.5, 0.6])
@pytest.mark.parametrize("name", list(CASES))
def test_cascade_refine_equals_the_composed_device_ops(dev, name, thr, masks):
    """Every output bit for bit, training mode."""
    case = _case(name)
    got = _fused(dev, case, thr, masks=masks)
    want = _composed(dev, case, thr, masks=masks)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    cls, ok = got["gt_classes"], got["is_valid"]
    assert (cls == 80).any() and (~ok).any() and (cls[~ok] == -1).all()
    if name == "1x512x256":  # every kind of row took part
        assert ((cls >= 0) & (cls < 80)).any()
        assert bool(((cls == -1) & ok).any()) == masks


@pytest.mark.parametrize("name", list(CASES))
def test_cascade_refine_inference_mode_equals_the_composed_device_ops(dev, name):
    case = _case(name)
    got = _fused(dev, case, None, training=False)
    want = _composed(dev, case, None, training=False)
    assert set(got) == {"boxes", "is_valid"}
    assert torch.equal(got["boxes"], want["boxes"])
    assert got["is_valid"].dtype == torch.bool and torch.equal(got["is_valid"], want["is_valid"])


@pytest.mark.parametrize("thr", [0.5, 0.6, 0.7])
@pytest.mark.parametrize("name", list(CASES))
def test_cascade_refine_matches_the_oracle_restatement(dev, name, thr):
    """Boxes within the project's box tolerance of the oracle's decode + clip;
    every label array_equal to the restatement fed the kernel's own boxes."""
    deltas, boxes, valid, image_hw, gt = case = _case(name)
    got = {k: v.cpu().numpy() for k, v in _fused(dev, case, thr).items()}
    want = cref.refine(deltas, boxes, valid, image_hw, W1, gt, thr, 80, decoded=got["boxes"])
    assert_boxes_close(got["boxes"], want["boxes"])
    for k in ("is_valid", "gt_classes", "gt_index", "gt_boxes", "loss_valid"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if name == "hand_made_2x70x5":
        v, c, i, lv = got["is_valid"], got["gt_classes"], got["gt_index"], got["loss_valid"]
        assert not v[0, 0] and c[0, 0] == -1
        assert i[0, 1] == 0 and c[0, 1] == 3
        assert c[0, 2] == (11 if thr == 0.5 else 80) and i[0, 2] == 2
        assert c[0, 3] == -1 and v[0, 3] and not lv[0, 3]
        assert not v[0, 4] and c[0, 4] == -1
        assert (c[1][v[1]] == 80).all() and (i[1] == 0).all()


# ------------------------------------------------ stage-averaged inference
def _frcnn_inputs(seed, N, P, K):
    rng = np.random.default_rng(seed)
    image_hw = np.array([[240, 320]] * N, np.int32)
    c = rng.uniform([0, 0], [240, 320], size=(N * P, 2))
    hw = rng.uniform(8, 160, size=(N * P, 2))
    props = oracle.clip_to_window(np.concatenate([c - hw / 2, c + hw / 2], 1).astype(F32),
                                  [0, 0, 240, 320])
    roi_img = np.repeat(np.arange(N, dtype=np.int32), P)
    roi_slot = np.tile(np.arange(P, dtype=np.int32), N)
    roi_slot[rng.random(N * P) < 0.05] = -1  # ignored rows (invalid proposals)
    logits = [rng.normal(0, 3, size=(N * P, K + 1)).astype(F32) for _ in range(3)]
    deltas = rng.normal(0, 0.5, size=(N * P, 4)).astype(F32)
    return image_hw, props, roi_img, roi_slot, logits, deltas


def test_staged_inference_one_stage_equals_fast_rcnn_inference(dev):
    ops = _ops()
    N, P, K = 2, 200, 80
    image_hw, props, roi_img, roi_slot, logits, deltas = _frcnn_inputs(11, N, P, K)
    t = lambda a: torch.from_numpy(a).to(dev)
    args = (t(deltas), t(props), t(roi_img), t(roi_slot), N, P, t(image_hw), W1, 0.05, 0.5, 100)
    for agnostic_nms in (False, True):
        want = ops.fast_rcnn_inference(t(logits[0]), *args, cls_agnostic=True,
                                       nms_cls_agnostic=agnostic_nms)
        got = ops.fast_rcnn_inference_stages([t(logits[0])], *args, cls_agnostic=True,
                                             nms_cls_agnostic=agnostic_nms)
        assert int(want[3].sum()) == N * 100
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g, w)


def test_staged_inference_three_stages_matches_the_oracle(dev):
    ops = _ops()
    N, P, K = 2, 200, 80
    w3 = (30.0, 30.0, 15.0, 15.0)
    image_hw, props, roi_img, roi_slot, logits, deltas = _frcnn_inputs(12, N, P, K)
    sm = [oracle.softmax(l) for l in logits]
    probs = ((sm[0] + sm[1]) + sm[2]) * F32(1.0 / 3)
    assert probs.dtype == F32
    # no averaged probability within 1e-6 relative of the threshold (else: another seed)
    assert np.abs(probs[:, :-1].astype(np.float64) - 0.05).min() > 1e-6 * 0.05
    boxes = np.tile(oracle.apply_deltas(deltas, props, w3), (1, K))
    keep = roi_slot >= 0
    want = oracle.fast_rcnn_inference(boxes[keep], probs[keep], roi_img[keep], roi_slot[keep], P,
                                      image_hw, 0.05, 0.5, 100)
    t = lambda a: torch.from_numpy(a).to(dev)
    gb, gs, gc, gv, groi = ops.fast_rcnn_inference_stages(
        [t(l) for l in logits], t(deltas), t(props), t(roi_img), t(roi_slot), N, P, t(image_hw),
        w3, 0.05, 0.5, 100, cls_agnostic=True)
    rows = np.nonzero(keep)[0]
    for n in range(N):
        wb, wsc, wc, wv, wroi = want[n]
        assert wv.sum() > 20
        np.testing.assert_array_equal(gv[n].cpu().numpy(), wv)
        np.testing.assert_array_equal(gc[n].cpu().numpy(), wc)
        np.testing.assert_array_equal(groi[n].cpu().numpy(), np.where(wroi >= 0, rows[wroi], -1))
        np.testing.assert_allclose(gs[n].cpu().numpy(), wsc, rtol=2e-6, atol=1e-7)
        assert_boxes_close(gb[n].cpu().numpy(), wb)


# ------------------------------------------------------------ the ROI heads
def _heads(dev, training, mask_on=False):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling.roi_heads import build_roi_heads
    cfg = get_cfg()
    cfg.merge_from_file(CASCADE)
    cfg.MODEL.MASK_ON = mask_on
    finalize(cfg, training, 1, CATS)
    torch.manual_seed(0)
    shapes = {f"p{l}": ShapeSpec(channels=256, stride=2 ** l) for l in (2, 3, 4, 5)}
    heads = build_roi_heads(cfg, shapes, scope="roi_heads").to(dev)
    with torch.no_grad():  # deltas that move the boxes, logits of O(1)
        for p in heads.box_predictor:
            p.bbox_pred.weights.normal_(0.0, 0.03)
            p.cls_score.weights.normal_(0.0, 0.1)
    return heads.train() if training else heads.eval()


def _head_inputs(dev, N=2, P=100, G=4, H=64, W=80):
    from detectron2_tensorflow_amd.structures import BoxList
    rng = np.random.default_rng(21)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    feats = {f"p{l}": t(rng.normal(size=(N, H >> l, W >> l, 256)).astype(F32)) for l in (2, 3, 4, 5)}
    c = rng.uniform([8, 8], [H - 8, W - 8], size=(N, G, 2))
    hw = rng.uniform(12, 40, size=(N, G, 2))
    gt_boxes = oracle.clip_to_window(np.concatenate([c - hw / 2, c + hw / 2], -1).reshape(-1, 4)
                                     .astype(F32), [0, 0, H, W]).reshape(N, G, 4)
    pick = rng.integers(0, G, size=(N, P))
    boxes = gt_boxes[np.arange(N)[:, None], pick] + rng.normal(0, 5, size=(N, P, 4))
    boxes[..., 2:] = np.maximum(boxes[..., 2:], boxes[..., :2] + 2)
    boxes = oracle.clip_to_window(boxes.reshape(-1, 4).astype(F32), [0, 0, H, W]).reshape(N, P, 4)
    valid = rng.random((N, P)) < 0.9
    boxes[~valid] = 0
    props = BoxList(t(boxes))
    props.add_field("is_valid", t(valid))
    targets = {"gt_boxes": t(gt_boxes), "gt_classes": t(rng.integers(0, 80, (N, G))),
               "is_valid": t(np.ones((N, G), bool)),
               "gt_is_crowd": t(np.array([[0] * (G - 1) + [1]] * N, bool)),
               "gt_difficult": t(np.zeros((N, G), bool))}
    images = types.SimpleNamespace(image_shapes=t(np.array([[H, W]] * N, np.int32)))
    return images, feats, props, targets


def test_cascade_heads_inference_equals_a_loop_of_public_pieces(dev):
    ops = _ops()
    heads = _heads(dev, False)
    images, feats, props, _ = _head_inputs(dev)
    with torch.no_grad():
        res, losses = heads(images, feats, props)
        assert losses == {}
        fl = [feats[f] for f in heads.in_features]
        boxes, valid = props.boxes, props.get_field("is_valid")
        N, P = valid.shape
        img = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(P)
        slot = torch.arange(P, dtype=torch.int32, device=dev).repeat(N)
        slot = torch.where(valid.reshape(-1), slot, torch.full_like(slot, -1))
        hw = images.image_shapes.to(torch.float32)
        win = torch.stack([hw[:, 0], hw[:, 1], hw[:, 0], hw[:, 1]], 1)[:, None, :]
        logits = []
        for k in range(3):
            if k > 0:
                dec = ops.apply_deltas(deltas, boxes.reshape(-1, 4),
                                       heads.box2box_transform[k - 1].weights)
                boxes = torch.minimum(dec.reshape(N, P, 4), win).clamp(min=0.0)
            x = heads.box_pooler.pool(fl, boxes.reshape(-1, 4).contiguous(), img)
            lg, deltas = heads.box_predictor[k](heads.box_head[k](x))
            logits.append(lg)
        assert (boxes != props.boxes).any()
        wb, ws, wc, wv, _ = ops.fast_rcnn_inference_stages(
            logits, deltas, boxes.reshape(-1, 4), img, slot, N, P, images.image_shapes,
            heads.box2box_transform[2].weights, heads.test_score_thresh, heads.test_nms_thresh,
            heads.test_detections_per_img, cls_agnostic=True)
    assert int(wv.sum()) > 10
    assert torch.equal(res.boxes, wb) and torch.equal(res.get_field("scores"), ws)
    assert torch.equal(res.get_field("pred_classes"), wc)
    assert torch.equal(res.get_field("is_valid"), wv)


def test_cascade_heads_training_losses_match_the_oracle_per_stage(dev):
    """Exactly the six stage keys, and each stage's pair against
    oracle.training.fast_rcnn_losses on that stage's own rows, fed the device's
    own logits, deltas and labels, so only the loss arithmetic differs: to
    2e-6 relative, the bound on the loss values of the box-head loss test
    tests/test_gpu_train.py::test_fused_fast_rcnn_loss_matches_tensor_formulation."""
    ops = _ops()
    heads = _heads(dev, True)
    images, feats, props, targets = _head_inputs(dev)
    torch.manual_seed(5)
    _, losses = heads(images, feats, props, targets)
    assert set(losses) == {f"{n}_stage{k}" for k in range(3) for n in ("loss_cls", "loss_box_reg")}
    with torch.no_grad():
        torch.manual_seed(5)
        s = heads.label_and_sample_proposals(props, targets)
        fl = [feats[f] for f in heads.in_features]
        N, S = s["is_valid"].shape
        img = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(S)
        cur = dict(s, loss_valid=s["is_valid"])
        seen = set()
        for k in range(3):
            if k > 0:
                cur = ops.cascade_refine(
                    deltas, cur["boxes"], cur["is_valid"], images.image_shapes,
                    heads.box2box_transform[k - 1].weights, gt_boxes=targets["gt_boxes"],
                    gt_valid=targets["is_valid"], gt_classes=targets["gt_classes"],
                    gt_crowd=targets["gt_is_crowd"], gt_difficult=targets["gt_difficult"],
                    iou_thr=(0.5, 0.6, 0.7)[k], num_classes=80)
            x = heads.box_pooler.pool(fl, cur["boxes"].reshape(-1, 4).contiguous(), img)
            logits, deltas = heads.box_predictor[k](heads.box_head[k](x))
            rows = cur["loss_valid"].reshape(-1).cpu().numpy()
            cls = cur["gt_classes"].reshape(-1).cpu().numpy()[rows]
            seen.update(np.unique(np.where(cls < 80, 0, 80)).tolist())
            want = otrain.fast_rcnn_losses(
                logits.cpu().numpy()[rows], deltas.cpu().numpy()[rows],
                cur["boxes"].reshape(-1, 4).cpu().numpy()[rows], cls,
                cur["gt_boxes"].reshape(-1, 4).cpu().numpy()[rows],
                heads.box2box_transform[k].weights)
            assert rows.sum() > 50
            for name, v in zip(("loss_cls", "loss_box_reg"), want):
                g = float(losses[f"{name}_stage{k}"])
                print(f"stage {k} {name}: gpu {g:.9g} oracle {v:.9g} "
                      f"rel {abs(g - v) / abs(v):.2e}")
                assert v > 0.1 and g == pytest.approx(v, rel=2e-6), (k, name, g, v)
        assert seen == {0, 80}  # foreground and background rows took part


def test_cascade_training_call_leaves_no_state_on_the_module(dev):
    """The step's image shapes and targets reach the stages as arguments: a
    training call adds no attribute to the head and removes none."""
    heads = _heads(dev, True)
    images, feats, props, targets = _head_inputs(dev)
    before = set(vars(heads))
    _, losses = heads(images, feats, props, targets)
    assert "loss_cls_stage2" in losses and set(vars(heads)) == before


def test_cascade_heads_scale_the_pooled_feature_gradient_by_one_third(dev, monkeypatch):
    """The gradient reaching each stage's pooled features through
    CascadeROIHeads is 1/3 of the gradient with the scale taken out (one f32
    multiply of the same values: torch.equal)."""
    ops = _ops()
    heads = _heads(dev, True)
    images, feats, props, targets = _head_inputs(dev)
    feats = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
    pool = heads.box_pooler.pool

    def run(scaled):
        pooled = []

        def recording_pool(*a, **kw):
            x = pool(*a, **kw)
            x.retain_grad()
            pooled.append(x)
            return x

        with monkeypatch.context() as m:
            m.setattr(heads.box_pooler, "pool", recording_pool)
            if not scaled:
                m.setattr(ops, "scale_gradient", lambda x, scale: x)
            torch.manual_seed(5)
            _, losses = heads(images, feats, props, targets)
            torch.stack(list(losses.values())).sum().backward()
        assert len(pooled) == 3
        return [x.grad for x in pooled]

    for k, (g_scaled, g_plain) in enumerate(zip(run(True), run(False))):
        assert float(g_plain.abs().max()) > 0, k
        assert torch.equal(g_scaled, g_plain * (1.0 / 3)), k


# ------------------------------------------- the cascade configs' RPN size
@pytest.mark.parametrize("post", [2000, 3264])
def test_rpn_proposals_post_nms_topk_past_8192_merge_entries(dev, post):
    """The cascade configs train with RPN.POST_NMS_TOPK_TRAIN = 2000 on five
    levels (10,000 merge entries per image, past the 8,192 the merge took
    before); 3264 is the most the host check admits on five levels (16,320
    entries: the merge rank's LDS).  tests/test_gpu_geometry.py::
    test_rpn_proposals_baseline_geometry's bars at 256x320 (kept scores and
    valid flags bit-exact, boxes within the box tolerance)."""
    import math
    rng = np.random.default_rng(202)
    N, A, H, W, pre = 2, 3, 256, 320, post
    strides = [4, 8, 16, 32, 64]
    hw = [(int(math.ceil(H / s)), int(math.ceil(W / s))) for s in strides]
    cells = [oracle.generate_cell_anchors([sz], [0.5, 1.0, 2.0]) for sz in [32, 64, 128, 256, 512]]
    logits = [rng.normal(size=(N, h, w, A)).astype(F32) for h, w in hw]
    deltas = [rng.normal(0, 0.1, size=(N, h, w, A * 4)).astype(F32) for h, w in hw]
    image_hw = np.array([[H, W], [H - 16, W - 20]], np.int32)
    props = []
    for (h, w), s, c, d in zip(hw, strides, cells, deltas):
        anc = oracle.grid_anchors(h, w, s, c)
        props.append(oracle.apply_deltas(d.reshape(-1, 4), np.tile(anc, (N, 1)), (1, 1, 1, 1))
                     .reshape(N, -1, 4))
    wb, ws, wv = oracle.find_top_rpn_proposals(props, [l.reshape(N, -1) for l in logits],
                                               image_hw, 0.7, pre, post, 0.0)
    gb, gs, gv = _ops().rpn_proposals([torch.from_numpy(l).to(dev) for l in logits],
                                      [torch.from_numpy(d).to(dev) for d in deltas], strides,
                                      [torch.from_numpy(c) for c in cells],
                                      torch.from_numpy(image_hw).to(dev), pre, post, 0.7, 0.0)
    np.testing.assert_array_equal(gv.cpu().numpy(), wv)
    np.testing.assert_array_equal(gs.cpu().numpy(), ws)
    assert_boxes_close(gb.cpu().numpy(), wb)
    assert wv.sum(axis=1).min() > 1638  # more survivors per image than 8,192 / 5


# ------------------------------------------------------------ whole models
def _model(dev, training, path=CASCADE):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(path)
    if cfg.MODEL.META_ARCHITECTURE != "PanopticFPN":  # (panoptic needs image-size masks)
        cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    if training:
        cfg.SOLVER.WARMUP_ITERS = 3
    finalize(cfg, training, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    return cfg, (model.train() if training else model.eval())


def _image(dev):
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.uniform(0, 255, size=(1, 256, 320, 3)).astype(F32)).to(dev)
    return {"image": img, "image_shape": torch.tensor([[256, 320]], device=dev)}


def test_cascade_model_inference(dev):
    from detectron2_tensorflow_amd import _C
    _, model = _model(dev, False)
    with torch.no_grad():
        inst = model.inference(_image(dev))["instances"]
    assert inst["boxes"].shape == (1, 100, 4) and inst["masks"].shape == (1, 100, 28, 28)
    for k in ("boxes", "scores", "masks"):
        assert torch.isfinite(inst[k]).all(), k
    _C.raise_on_errors(dev)


def test_cascade_model_training_step(dev):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg, model = _model(dev, True)
    batch = synthetic_train_batch(2, 256, 320, 0, dev)
    calibrate_rcnn_scores(model, batch)
    grads = {}
    hooks = [p.cls_score.weights.register_hook(
        lambda g, k=k: grads.__setitem__(k, float(g.abs().max())))
        for k, p in enumerate(model.roi_heads.box_predictor)]
    losses = Trainer(cfg, model).step(batch)
    _C.raise_on_errors(dev)
    for h in hooks:
        h.remove()
    want = {f"{n}_stage{k}" for k in range(3) for n in ("loss_cls", "loss_box_reg")}
    assert want | {"loss_mask", "loss_rpn_cls", "loss_rpn_loc"} == set(losses) - {"total_loss"}
    print({k: round(float(v), 4) for k, v in losses.items()})
    assert all(np.isfinite(float(v)) for v in losses.values()), losses
    assert len(grads) == 3 and all(np.isfinite(v) and v > 0.0 for v in grads.values()), grads
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_cascade_graphed_step_one_replay_matches_eager_step(dev, monkeypatch):
    """tests/test_gpu_deform.py::test_dconv_graphed_step_one_replay_matches_eager_step
    with the cascade config: losses, weights and momentum bit-identical, and
    no capture holds a memset node."""
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.engine.graphed import GraphedTrainer
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    cfg, m_eager = _model(dev, True)
    _, m_graph = _model(dev, True)
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
        assert set(le) == set(lg) and "loss_cls_stage2" in le
        for k in le:
            assert torch.equal(le[k].reshape(()), lg[k].reshape(())), (i, k, le[k], lg[k])
        for (n, pe), pg in zip(m_eager.named_parameters(), m_graph.parameters()):
            assert torch.equal(pe, pg), (i, n)
        for ae, ag in zip(eager.optimizer.accum, graphed.optimizer.accum):
            assert torch.equal(ae, ag), i
    assert graphed.replays == 1
    assert graphed.census and all(c.get("memset", 0) == 0 and c.get("kernel", 0) > 100
                                  for c in graphed.census.values()), graphed.census


def test_panoptic_cascade_config_inference(dev):
    from detectron2_tensorflow_amd import _C
    _, model = _model(dev, False, PANOPTIC_CASCADE)
    with torch.no_grad():
        out = model.inference(_image(dev))
    assert out

    def finite(v):
        if torch.is_tensor(v):
            return bool(torch.isfinite(v.float()).all()) if v.is_floating_point() else True
        if isinstance(v, dict):
            return all(finite(x) for x in v.values())
        if isinstance(v, (list, tuple)):
            return all(finite(x) for x in v)
        return True

    assert finite(out)
    _C.raise_on_errors(dev)
