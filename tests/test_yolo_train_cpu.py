"""YOLOv4 training without a GPU: the float64 restatement of the reference's
targets and loss (tests/yolo_train_reference.py) reproduces a hand-made case
whose slots, states, counts and multi-hot rows are literals here; the
package's tensor arm agrees with it in float64, gradients included; crowd and
difficult flags of GT that were not valid anyway change nothing; the shipped
config built in the training phase has batch-statistics BatchNorms where it
trains, built in the inference phase it has none and refuses ``.train()``; and
the new C entry points refuse null pointers and bad sizes on the host."""
import ctypes
import os

import pytest
import torch

import yolo_train_reference as R
from detectron2_tensorflow_amd.modeling.matcher import YOLOMatcher
from detectron2_tensorflow_amd.modeling.single_stage_heads import yolov4_outputs as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
YOLO = "COCO-Detection/yolov4_D_53_PAN_1x.yaml"
THRESH, CLS_NORM, IOU_NORM = 0.5, 1.0, 0.07
UP = {"conf_loss": 0.7, "cls_loss": 1.3, "box_loss": 2.1}
LOSSES = ("conf_loss", "cls_loss", "box_loss")


def restated(logits, gt, K, hw):
    out = R.losses(logits, gt, K, THRESH, CLS_NORM, IOU_NORM, hw)
    return out, R.gradients(out, UP)


def valid_of(gt):
    return gt["is_valid"] & ~gt["gt_is_crowd"] & ~gt["gt_difficult"]


def tensor_arm(logits, gt, K, hw):
    lv = [x.double().requires_grad_(True) for x in logits]
    dbg = {}
    conf, cls, box, npos, nneg = Y.yolov4_losses_dense(
        lv, R.STRIDES, R.cell_anchors(), R.SCALE_YX, K, gt["gt_boxes"], gt["gt_classes"],
        valid_of(gt), hw, THRESH, CLS_NORM, IOU_NORM, debug=dbg)
    total = UP["conf_loss"] * conf + UP["cls_loss"] * cls + UP["box_loss"] * box
    grads = torch.autograd.grad(total, lv, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, lv)]
    return {"conf_loss": conf, "cls_loss": cls, "box_loss": box, "num_pos": int(npos),
            "num_neg": int(nneg), **dbg}, grads


@pytest.fixture(scope="module")
def hand_made():
    logits, gt, expected = R.hand_made_case()
    out, grads = restated(logits, gt, 3, (64, 96))
    return logits, gt, expected, out, grads


def test_restatement_reproduces_the_hand_made_case(hand_made):
    logits, gt, expected, out, _ = hand_made
    state = out["state"]
    assert state.shape == (2, 378)
    # the maximum CIoU of every prediction is at least 1e-4 off the threshold:
    # the condition for comparing states exactly between float32 and float64
    assert R.threshold_margin(out, THRESH) >= 1e-4
    assert out["max_iou"][0].isfinite().all() and out["max_iou"][1].isnan().all()
    # positives: exactly the four slots, one per level plus the collision
    assert torch.nonzero(state == 2).tolist() == [[0, 78], [0, 162], [0, 333], [0, 372]]
    assert out["num_pos"] == 4 == expected["num_pos"]
    # image 1 has no valid GT: no positives and no negatives
    assert (state[1] == 0).all()
    # image 0: 372 negatives, and two predictions whose best CIoU with a valid
    # GT is 0.5 or more without being a slot ("neither")
    assert out["num_neg"] == 372 and int((state[0] == 1).sum()) == 372
    assert int((state[0] == 0).sum()) == 2
    # the slot two GT share keeps the box of the higher index and both classes
    assert out["label_prob"][0, 78].tolist() == [1.0, 0.0, 1.0]
    assert out["target_boxes"][0, 78].tolist() == [10.0, 18.0, 22.0, 26.0]
    assert out["label_prob"][0, 162].tolist() == [0.0, 1.0, 0.0]
    assert out["target_boxes"][0, 162].tolist() == [0.0, 0.0, 64.0, 96.0]
    assert out["label_prob"][0, 333].tolist() == [1.0, 0.0, 0.0]
    assert out["target_boxes"][0, 333].tolist() == [-368.0, -152.0, 432.0, 248.0]
    assert out["label_prob"][0, 372].tolist() == [0.0, 0.0, 1.0]
    assert out["target_boxes"][0, 372].tolist() == [-1568.0, -1552.0, 1632.0, 1648.0]
    assert (out["label_prob"].sum(-1)[state != 2] == 0).all()
    for k in LOSSES:
        assert torch.isfinite(out[k])


def test_tensor_arm_reproduces_the_literal_slots(hand_made):
    logits, gt, expected, out, _ = hand_made
    got, _ = tensor_arm(logits, gt, 3, (64, 96))
    assert got["slot"].tolist() == [[78, 78, 162, -1, -1, 333, 372, -1], [-1] * 8]
    assert got["slot"].tolist() == expected["slot"]
    owner = got["owner"]
    assert {(n, p): int(owner[n, p]) for n, p in torch.nonzero(owner >= 0).tolist()} == \
        {(0, 78): 1, (0, 162): 2, (0, 333): 5, (0, 372): 6}
    assert torch.equal(got["state"], out["state"])


CASES = {
    "hand_made": lambda: R.hand_made_case()[:2] + (3, (64, 96)),
    "random": lambda: R.random_case(3, 2, 80, 64, 96, 16, 10) + (80, (64, 96)),
    "collisions": lambda: R.random_case(7, 2, 3, 64, 96, 80, 70) + (3, (64, 96)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tensor_arm_agrees_with_the_restatement_in_float64(name):
    logits, gt, K, hw = CASES[name]()
    want, wgrads = restated(logits, gt, K, hw)
    assert R.threshold_margin(want, THRESH) >= 1e-4
    got, ggrads = tensor_arm(logits, gt, K, hw)
    assert got["num_pos"] == want["num_pos"] > 0 and got["num_neg"] == want["num_neg"] > 0
    assert torch.equal(got["state"], want["state"])
    # float64 against float64: the same expressions in another order of
    # evaluation (dense against per image), 1e-12 relative
    for k in LOSSES:
        assert abs(got[k].item() - want[k].item()) <= 1e-12 * abs(want[k].item()), k
    for g, w in zip(ggrads, wgrads):
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())
        assert torch.equal(g == 0, w == 0)  # the same elements are reached


def test_flags_of_gt_that_were_not_valid_change_nothing(hand_made):
    """Rows 3 (crowd) and 4 (difficult) of image 0 are out whichever of the
    two flags they carry, and the padding rows whatever flags they carry: the
    crowd and difficult matrices only turn zeros of respond_bgd into -1
    (matcher.py:244-266), which reads as 0 (yolov4_outputs.py:195, :278)."""
    logits, gt, _, out, grads = hand_made
    variants = []
    swapped = {k: v.clone() for k, v in gt.items()}
    swapped["gt_is_crowd"][0, 3], swapped["gt_difficult"][0, 3] = False, True
    swapped["gt_is_crowd"][0, 4], swapped["gt_difficult"][0, 4] = True, False
    variants.append(swapped)
    padded = {k: v.clone() for k, v in gt.items()}
    padded["gt_is_crowd"][:, 7] = True
    padded["gt_difficult"][1, 1:] = True
    variants.append(padded)
    both = {k: v.clone() for k, v in gt.items()}
    both["gt_is_crowd"][0, 4] = True   # difficult and crowd
    variants.append(both)
    for v in variants:
        assert torch.equal(valid_of(v), valid_of(gt))
        o, g = restated(logits, v, 3, (64, 96))
        assert torch.equal(o["state"], out["state"])
        assert all(o[k].item() == out[k].item() for k in LOSSES)
        assert all(torch.equal(a, b) for a, b in zip(g, grads))
        t, tg = tensor_arm(logits, v, 3, (64, 96))
        assert torch.equal(t["state"], out["state"])
        assert all(abs(t[k].item() - out[k].item()) <= 1e-12 * abs(out[k].item()) for k in LOSSES)


def test_matcher_is_the_references():
    m = YOLOMatcher(0.5)
    assert m.threshold == 0.5 and YOLOMatcher is Y.YOLOMatcher
    anchor = torch.tensor([[0.1, 0.4, 0.4], [0.3, 0.2, 0.1]])
    pred = torch.tensor([[0.6, 0.2, 0.1, 0.49], [0.1, 0.5, 0.2, 0.3]])
    best, bgd = m(anchor, pred)
    assert best.tolist() == [1, 0]                      # the first maximum
    assert bgd.tolist() == [0, 0, 1, 1]                 # max < threshold, strictly
    # no GT: zeros everywhere (matcher.py:236-242)
    best, bgd = m(anchor[:0], pred[:0])
    assert best.tolist() == [] and bgd.tolist() == [0, 0, 0, 0]
    # crowd / difficult only mark zeros with -1
    crowd = torch.tensor([[0.9, 0.0, 0.9, 0.0]])
    _, bgd = m(anchor, pred, crowd, None)
    assert bgd.tolist() == [-1, 0, 1, 1]
    _, bgd = m(anchor, pred, None, torch.tensor([[0.4, 0.6, 0.6, 0.6]]))
    assert bgd.tolist() == [0, -1, 1, 1]
    # dense rows with a validity mask: row 0 masked out
    _, bgd = m(anchor, pred, valid=torch.tensor([False, True]))
    assert bgd.tolist() == [1, 0, 1, 1]


# ------------------------------------------------------------- the builders
def _build(training, backbone_norm=None):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.training import set_training_phase
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", YOLO))
    if backbone_norm is not None:
        cfg.MODEL.RESNETS.NORM = backbone_norm
    cfg = finalize(cfg, training, 1, CATS)
    torch.manual_seed(0)
    try:
        return cfg, build_model(cfg)
    finally:
        set_training_phase(False)


def _bns(module):
    from detectron2_tensorflow_amd.layers import BatchNorm
    return [m for m in module.modules() if isinstance(m, BatchNorm)]


@pytest.mark.parametrize("backbone_norm", [None, "BN"])
def test_training_phase_builds_batch_statistics_where_the_model_trains(backbone_norm):
    """The shipped config leaves MODEL.RESNETS.NORM at "FrozenBN" (as the
    reference's does): its DarkNet keeps the inference form throughout and the
    neck and the tower (NORM "BN") train on batch statistics.  With
    MODEL.RESNETS.NORM "BN" the DarkNet stages that train do too."""
    cfg, model = _build(True, backbone_norm)
    bb = model.backbone
    assert cfg.MODEL.RESNETS.NORM == (backbone_norm or "FrozenBN")
    # FREEZE_AT = 2: the stem, res1 and res2 stay in the inference form
    frozen = _bns(bb.stem) + _bns(bb.stages[0]) + _bns(bb.stages[1])
    assert frozen and not any(m.batch_stats for m in frozen)
    assert not any(p.requires_grad for m in frozen for p in m.parameters())
    for part in (bb.stages[2], bb.stages[3], bb.stages[4]):
        bns = _bns(part)
        assert bns and all(m.batch_stats == (backbone_norm == "BN") and not m.sync for m in bns)
    for part in (model.neck, model.detector.head):
        bns = _bns(part)
        assert bns and all(m.batch_stats and not m.sync for m in bns)
    assert sum(len(_bns(m)) for m in (bb, model.neck, model.detector)) == 107
    head = model.detector
    assert head.built_for_training and isinstance(head.matcher, YOLOMatcher)
    assert head.matcher.threshold == 0.5
    # the tower's pred convs: still bias, no norm
    assert all(p.normalizer_fn is None and p.bias is not None for p in head.head.preds)


def test_inference_phase_builds_none_and_still_refuses_to_train():
    _, model = _build(False)
    assert not any(m.batch_stats for m in _bns(model))
    head = model.detector
    assert not head.built_for_training and head.matcher is None
    model.detector.train()
    with pytest.raises(NotImplementedError) as e:
        model.detector(None, {}, None)
    msg = str(e.value)
    assert "inference phase" in msg and "finalize(cfg, True" in msg
    assert "batch statistics" in msg and "YOLOMatcher" in msg and "CIoU" in msg


def test_head_losses_on_the_cpu_take_the_tensor_arm():
    """The head's own ``losses`` (targets dict -> the three named losses) on CPU
    tensors equals the restatement: is_valid & ~crowd & ~difficult, the padded
    batch tensor's area, MODEL.YOLOV4's normalisers."""
    from types import SimpleNamespace
    _, model = _build(True)
    head = model.detector
    logits, gt = R.random_case(3, 2, 80, 64, 96, 16, 10)
    want, _ = restated(logits, gt, 80, (64, 96))
    images = SimpleNamespace(tensor=torch.zeros(2, 64, 96, 3))
    got = head.losses(images, [x.double() for x in logits], gt)
    assert set(got) == set(LOSSES)
    for k in LOSSES:
        assert abs(got[k].item() - want[k].item()) <= 1e-12 * abs(want[k].item()), k


# ------------------------------------------------------------------ the ABI
def _lib():
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    return _C, _C.load()


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def test_new_entries_refuse_bad_arguments_without_gpu():
    _C, lib = _lib()
    f, i32 = ctypes.c_float, ctypes.c_int32
    lhw = _arr(i32, [2, 2] * 9)
    st = _arr(f, [8.0, 16.0, 32.0] * 3)
    chw = _arr(f, [8.0] * (9 * 13 * 2))
    sc = _arr(f, [1.0, 0.0] * 9)
    fake = ctypes.c_void_p(256)  # non-null, never dereferenced: refused before any launch
    ptrs = _arr(ctypes.c_void_p, [256, 256, 256])
    assert lib.d2mi_yolov4_loss_blocks() >= 1

    def assign(L=3, A=3, N=1, G=4, lhw=lhw, st=st, gt=fake, valid=fake, slot=fake, owner=fake):
        return lib.d2mi_yolov4_assign(lhw, st, chw, L, A, N, gt, valid, G, slot, owner, None)

    def fwd(L=3, A=3, K=80, N=1, G=4, logits=ptrs, gt=fake, owner=fake, part=fake, state=fake,
            area=64.0 * 96.0):
        return lib.d2mi_yolov4_loss_fwd(logits, lhw, st, chw, sc, L, A, K, N, gt, fake, fake, G, fake,
                                        owner, area, 0.5, 0.07, part, state, None)

    def bwd(L=3, A=3, K=80, N=1, G=4, logits=ptrs, d=ptrs, gt=fake, owner=fake, state=fake):
        return lib.d2mi_yolov4_loss_bwd(logits, d, lhw, st, chw, sc, L, A, K, N, gt, fake, G, fake,
                                        owner, state, 64.0 * 96.0, 0.07, 1.0, 1.0, None, None, None,
                                        None)

    for fn in (assign, fwd, bwd):
        assert fn(L=9) < 0 and "L=9" in _C.last_error()           # D2MI_MAX_LEVELS = 8
        assert fn(L=2) < 0 and "3 levels" in _C.last_error()
        assert fn(A=13) < 0 and "A=13" in _C.last_error()         # yolo.hip's own limit
        assert fn(N=0) < 0 and "N=0" in _C.last_error()
        assert fn(G=-1) < 0 and "G=-1" in _C.last_error()
        assert fn(gt=None) < 0 and "null" in _C.last_error()
        assert fn(gt=ctypes.c_void_p(260)) < 0 and "16B aligned" in _C.last_error()
        assert fn(owner=None) < 0 and "owner is null" in _C.last_error()
    assert assign(lhw=None) < 0 and "level_hw is null" in _C.last_error()
    assert assign(st=None) < 0 and "null host array" in _C.last_error()
    assert assign(slot=None) < 0 and "null" in _C.last_error()
    assert assign(valid=None) < 0 and "null" in _C.last_error()
    for fn in (fwd, bwd):
        assert fn(K=0) < 0 and "K=0" in _C.last_error()
        assert fn(logits=None) < 0 and "null" in _C.last_error()
        assert fn(logits=_arr(ctypes.c_void_p, [256, 0, 256])) < 0 and "level 1" in _C.last_error()
    assert fwd(part=None) < 0 and "null outputs" in _C.last_error()
    assert fwd(state=None) < 0 and "null outputs" in _C.last_error()
    assert fwd(area=0.0) < 0 and "image_area" in _C.last_error()
    assert bwd(d=None) < 0 and "null" in _C.last_error()
    assert bwd(d=_arr(ctypes.c_void_p, [256, 256, 0])) < 0 and "level 2 gradient" in _C.last_error()
    assert bwd(state=None) < 0 and "null" in _C.last_error()
