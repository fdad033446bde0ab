"""GPU tests of the Panoptic FPN kernels (csrc/sem_seg.hip) and models.

The references are written here: the fused loss against a float64 torch
restatement (TF half-pixel bilinear x4, then cross_entropy with ignore); the
fused argmax against the unfused ops.resize_bilinear + zero pad +
torch.argmax (the same arithmetic: exact); the panoptic merge against a numpy
restatement of panoptic_fpn.py:184-279 (exact).

Loss tolerance: the same formula evaluated in float32 on the CPU gives the
format's own error err32 against float64; the GPU may have 4 x that + 1e-6
(the rule of test_gpu_model.py's FPN / mask-head parity test) and never more
than the project's 1e-4; gradients are compared relative to max |g|.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, LDC, SCALE, IGNORE = 54, 56, 4, 255
CATEGORY_MAP = {"num_thing_classes": 80, "num_stuff_classes": 54, "stuff_ignore_value": IGNORE}


# ------------------------------------------------------------------ references
def resize_half_pixel(x, oh, ow):
    """TF ResizeBilinear with half-pixel centres on [N, H, W, C] in x's dtype,
    term by term (lower = max(floor, 0), upper = min(ceil, size - 1), lerp =
    in - floor(in); top + (bottom - top) * yl); differentiable."""
    N, H, W, _ = x.shape

    def interp(o, i):
        scale = torch.tensor(np.float32(i) / np.float32(o), dtype=x.dtype)
        v = (torch.arange(o, dtype=x.dtype) + 0.5) * scale - 0.5
        f = torch.floor(v)
        return f.long().clamp(min=0), torch.ceil(v).long().clamp(max=i - 1), v - f

    ylo, yhi, yl = interp(oh, H)
    xlo, xhi, xl = interp(ow, W)
    top_rows, bot_rows = x[:, ylo], x[:, yhi]
    tl, tr = top_rows[:, :, xlo], top_rows[:, :, xhi]
    bl, br = bot_rows[:, :, xlo], bot_rows[:, :, xhi]
    xl, yl = xl.view(1, 1, ow, 1), yl.view(1, oh, 1, 1)
    top = tl + (tr - tl) * xl
    bottom = bl + (br - bl) * xl
    return top + (bottom - top) * yl


def padded_labels(labels, shapes, H, W):
    """ImageList.from_tensors(labels, shapes, pad_value=IGNORE) on the [H, W] canvas."""
    N, Hl, Wl = labels.shape
    full = torch.full((N, H, W), IGNORE, dtype=torch.long)
    full[:, :Hl, :Wl] = labels.long()
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    inside = (ys < shapes[:, 0, None, None]) & (xs < shapes[:, 1, None, None])
    return torch.where(inside, full, torch.full_like(full, IGNORE))


def loss_reference(logits, labels, shapes, loss_weight, upstream, dtype):
    """(loss, d(upstream * loss) / d logits) of semantic_seg.py:197-218 in ``dtype`` on the CPU."""
    x = logits[..., :C].to(dtype).clone().requires_grad_(True)
    N, h, w, _ = x.shape
    H, W = h * SCALE, w * SCALE
    up = resize_half_pixel(x, H, W)
    target = padded_labels(labels, shapes, H, W)
    count = int((target != IGNORE).sum())
    if count == 0:
        return torch.zeros((), dtype=dtype), torch.zeros_like(x)
    ce = F.cross_entropy(up.reshape(-1, C), target.reshape(-1), ignore_index=IGNORE,
                         reduction="sum")
    loss = ce / count * loss_weight
    (loss * upstream).backward()
    return loss.detach(), x.grad


def loss_case(case, h, w):
    """(logits [2, h, w, LDC], labels, image_shapes) of one of the issue's four cases."""
    g = torch.Generator().manual_seed(100 * h + w)
    H, W = h * SCALE, w * SCALE
    logits = torch.randn(2, h, w, LDC, generator=g) * 3.0
    logits[..., C:] = 37.0  # pad channels: must be ignored, whatever they hold
    Hl, Wl = (H - 3, W - 5) if case == "short_labels" else (H, W)
    labels = torch.randint(0, C, (2, Hl, Wl), generator=g, dtype=torch.int32)
    if case == "all_ignored":
        labels[:] = IGNORE
    else:
        labels[torch.rand(2, Hl, Wl, generator=g) < 0.3] = IGNORE
    shapes = torch.tensor([[H, W], [H, W]], dtype=torch.int32)
    if case == "small_image":
        shapes[1] = torch.tensor([H - 6, W - 9])
    return logits, labels, shapes


_REFERENCES = {}


def references(case, h, w):
    """The float64 and float32 CPU results of a case, computed once."""
    key = (case, h, w)
    if key not in _REFERENCES:
        logits, labels, shapes = loss_case(case, h, w)
        _REFERENCES[key] = (loss_reference(logits, labels, shapes, 0.5, 3.0, torch.float64),
                            loss_reference(logits, labels, shapes, 0.5, 3.0, torch.float32))
    return _REFERENCES[key]


def close_enough(got, want64, want32, what):
    """The loss: err <= 4 * err32 + 1e-6 and err <= 1e-4 * max(|want|, 1).  A
    gradient: the same two bounds on the errors divided by max |g| (a zero
    reference must be met exactly)."""
    want64 = want64.double()
    err = (got.cpu().double() - want64).abs().max().item()
    err32 = (want32.double() - want64).abs().max().item()
    scale = want64.abs().max().item()
    print(f"{what}: err {err:.3e} err32 {err32:.3e} scale {scale:.3e}")
    if what == "loss":
        assert err <= 1e-4 * max(scale, 1.0), (what, err, scale)
        assert err <= 4 * err32 + 1e-6, (what, err, err32)
    elif scale == 0.0:
        assert err == 0.0, (what, err)
    else:
        assert err / scale <= 1e-4, (what, err, scale)
        assert err / scale <= 4 * err32 / scale + 1e-6, (what, err, err32, scale)


# ------------------------------------------------------------------------ loss
@pytest.mark.parametrize("h,w", [(5, 7), (19, 35)])
@pytest.mark.parametrize("case", ["random", "small_image", "short_labels", "all_ignored"])
def test_sem_seg_loss_forward_and_backward(dev, case, h, w):
    from detectron2_tensorflow_amd.layers import ops
    logits, labels, shapes = loss_case(case, h, w)
    (loss64, grad64), (loss32, grad32) = references(case, h, w)

    def run():
        x = logits.to(dev).requires_grad_(True)
        loss = ops.sem_seg_loss(x, labels.to(dev), shapes.to(dev), IGNORE, SCALE, 0.5,
                                num_classes=C)
        (loss * 3.0).backward()
        return loss.detach(), x.grad

    loss, grad = run()
    assert loss.shape == () and grad.shape == logits.shape
    assert torch.all(grad[..., C:] == 0)  # pad channels: exactly 0
    if case == "all_ignored":
        assert loss.item() == 0.0 and torch.all(grad == 0)
    else:
        assert loss64.item() > 1.0  # ~log(54) + the spread of N(0, 3^2) logits
    close_enough(loss, loss64, loss32, "loss")
    close_enough(grad[..., :C], grad64, grad32, "grad")
    loss2, grad2 = run()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)  # fixed-order sums


# ---------------------------------------------------------------------- argmax
@pytest.mark.parametrize("h,w", [(5, 7), (19, 35)])
def test_sem_seg_argmax_equals_the_unfused_composition(dev, h, w):
    from detectron2_tensorflow_amd.layers import ops
    g = torch.Generator().manual_seed(7 * h + w)
    H, W = h * SCALE, w * SCALE
    logits = torch.randn(2, h, w, LDC, generator=g) * 3.0
    logits[..., C:] = 37.0
    # ties: channels 9 and 4 equal and the largest over a block (the interpolated values tie too)
    logits[0, 1:4, 2:6, 9] = 20.0
    logits[0, 1:4, 2:6, 4] = 20.0
    shapes = torch.tensor([[H, W], [H - 6, W - 9]], dtype=torch.int32)
    x = logits.to(dev)
    got = ops.sem_seg_argmax(x, shapes.to(dev), SCALE, num_classes=C)
    full = ops.resize_bilinear(x[..., :C].contiguous(), (H, W))
    for n in range(2):  # sem_seg_postprocess "conventional": crop to the true shape, zero pad
        full[n, int(shapes[n, 0]):] = 0
        full[n, :, int(shapes[n, 1]):] = 0
    want = torch.argmax(full, dim=-1)
    assert got.dtype == torch.int64 and got.shape == (2, H, W)
    assert torch.equal(got, want)
    assert torch.all(got[1, H - 6:] == 0) and torch.all(got[1, :, W - 9:] == 0)
    assert torch.all(got[0, 8:12, 12:20] == 4)  # inside the tie block: the lower index


# --------------------------------------------------------------------- combine
def combine_reference(masks, scores, classes, boxes, valid, sem_seg, overlap, area_limit, conf,
                      num_stuff):
    """combine_single_image (panoptic_fpn.py:184-279) in numpy, one image."""
    D = masks.shape[0]
    pan = np.zeros(sem_seg.shape, np.int32)
    rows = {k: [] for k in ("id", "isthing", "score", "category_id", "instance_id", "bbox",
                            "is_valid", "area")}

    def add(**kw):
        for k, v in kw.items():
            rows[k].append(v)

    order = np.argsort(-scores, kind="stable")
    seg_id = 0
    for i in range(D):
        idx = order[i]
        m = masks[idx]
        area = np.float32(m.astype(np.float32).sum())
        inter = np.float32(((m > 0) & (pan > 0)).astype(np.float32).sum())
        ok = bool(valid[idx]) and bool(scores[idx] > np.float32(conf)) and bool(area > 0) \
            and bool(inter / area < np.float32(overlap))
        mask = (m > 0) & ~(pan > 0) if ok else np.zeros_like(pan, bool)
        seg_id += 1
        pan += seg_id * mask.astype(np.int32)
        add(id=seg_id, isthing=True, score=scores[idx], category_id=classes[idx],
            instance_id=idx, bbox=boxes[idx], is_valid=ok, area=area)
    for label in range(1, num_stuff):
        mask = (sem_seg == label) & ~(pan > 0)
        area = np.float32(mask.astype(np.float32).sum())
        ok = bool(area > area_limit)
        if ok:
            nz = np.argwhere(mask)
            box = np.concatenate([nz.min(0), nz.max(0)]).astype(np.float32)
        else:
            mask = np.zeros_like(mask)
            box = np.zeros(4, np.float32)
        seg_id += 1
        pan += seg_id * mask.astype(np.int32)
        add(id=seg_id, isthing=False, score=np.float32(0.5), category_id=label, instance_id=0,
            bbox=box, is_valid=ok, area=area)
    out = {k: np.stack([np.asarray(v) for v in vs]) for k, vs in rows.items()}
    out["panoptic_seg"] = pan
    return out


def combine_inputs():
    """Two images, D = 8, 24 x 40, labels 0..5 (+ one label past the stuff
    classes).  Image 0 by instance index: 0 a plain instance; 1 overlaps it
    above the threshold; 2 overlaps it below; 3 and 4 tie in score and cover
    each other (the lower index wins); 5 an empty mask with the top score;
    6 an invalid row; 7 below the confidence threshold.  Image 1: the same
    instances in another order, another class map."""
    H, W, D = 24, 40, 8
    m = np.zeros((D, H, W), np.uint8)
    m[0, 2:10, 2:12] = 1
    m[1, 3:10, 3:12] = 1
    m[2, 8:14, 10:20] = 1
    m[3, 15:20, 0:10] = 1
    m[4, 15:20, 2:10] = 1
    m[6, 0:5, 30:40] = 1
    m[7, 18:24, 30:40] = 1
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.6, 0.95, 0.85, 0.3], np.float32)
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 1], bool)
    classes = np.array([3, 17, 5, 60, 61, 2, 9, 44], np.int64)
    rng = np.random.default_rng(5)
    boxes = rng.uniform(0, 24, size=(D, 4)).astype(np.float32)
    sem = np.zeros((H, W), np.int64)
    sem[0:12, 20:40] = 1      # large: claimed (minus nothing: instance 6 is invalid)
    sem[20:23, 12:15] = 2     # 9 pixels: under the limit
    sem[0:14, 0:20] = 3       # mostly under instances 0 and 2: the rest is still > 20
    sem[14:18, 20:25] = 5     # exactly 20 pixels: not above the limit
    sem[12:14, 30:40] = 7     # past the stuff classes: no segment
    perm = np.array([4, 2, 7, 0, 5, 3, 6, 1])
    sem1 = np.zeros((H, W), np.int64)
    sem1[10:24, 10:40] = 4    # label 4 absent from image 0
    sem1[0:3, 0:5] = 1        # 15 pixels: under the limit
    return (np.stack([m, m[perm]]), np.stack([scores, scores[perm]]),
            np.stack([classes, classes[perm]]), np.stack([boxes, boxes[perm]]),
            np.stack([valid, valid[perm]]), np.stack([sem, sem1]))


def test_panoptic_combine_equals_the_reference_loop(dev):
    from detectron2_tensorflow_amd.layers import ops
    masks, scores, classes, boxes, valid, sem = combine_inputs()
    S, limit = 6, 20
    got = ops.panoptic_combine(*(torch.from_numpy(a).to(dev)
                                 for a in (masks, scores, classes, boxes, valid, sem)),
                               0.5, limit, 0.5, S)
    dtypes = {"id": torch.int32, "isthing": torch.bool, "score": torch.float32,
              "category_id": torch.int64, "instance_id": torch.int32, "bbox": torch.float32,
              "is_valid": torch.bool, "area": torch.float32, "panoptic_seg": torch.int32}
    assert set(got) == set(dtypes)
    seen = set()
    for n in range(2):
        want = combine_reference(masks[n], scores[n], classes[n], boxes[n], valid[n], sem[n], 0.5,
                                 limit, 0.5, S)
        for k, dt in dtypes.items():
            assert got[k].dtype == dt, k
            g = got[k][n].cpu().numpy()
            assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
            assert np.array_equal(g, want[k].astype(g.dtype)), (n, k, g, want[k])
        seen.update((bool(t), bool(v)) for t, v in zip(want["isthing"], want["is_valid"]))
        assert want["id"].tolist() == list(range(1, 8 + S))
    # both branches of both passes occur
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


# ----------------------------------------------------------------------- model
def _cfg(training, meta_arch=None):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(
        ROOT, "configs", "COCO-PanopticSegmentation", "panoptic_fpn_R_50_1x.yaml"))
    if meta_arch is not None:
        cfg.MODEL.META_ARCHITECTURE = meta_arch
    finalize(cfg, training=training, world_size=1, category_map=CATEGORY_MAP)
    return cfg


@pytest.fixture(scope="module")
def panoptic(dev):
    from detectron2_tensorflow_amd.modeling import build_model
    torch.manual_seed(0)
    return build_model(_cfg(False)).to(dev).eval()


def _images(dev):
    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 256, 320, 3, generator=g) * 255
    return {"image": img.to(dev),
            "image_shape": torch.tensor([[256, 320], [240, 300]], dtype=torch.int32, device=dev)}


def test_panoptic_fpn_inference_outputs(dev, panoptic):
    from detectron2_tensorflow_amd import _C
    with torch.no_grad():
        out = panoptic(_images(dev))
    _C.raise_on_errors(dev)
    assert set(out) == {"instances", "sem_seg", "panoptic_seg"}
    inst, sem, pan = out["instances"], out["sem_seg"], out["panoptic_seg"]
    assert inst["boxes"].shape == (2, 100, 4) and inst["scores"].shape == (2, 100)
    assert inst["masks"].shape == (2, 100, 256, 320) and inst["masks"].dtype == torch.uint8
    assert sem.shape == (2, 256, 320) and sem.dtype == torch.int64
    assert int(sem.min()) >= 0 and int(sem.max()) < 54
    assert torch.all(sem[1, 240:] == 0) and torch.all(sem[1, :, 300:] == 0)
    rows = 100 + 54 - 1
    assert pan["panoptic_seg"].shape == (2, 256, 320) and pan["panoptic_seg"].dtype == torch.int32
    assert pan["id"].shape == (2, rows) and pan["bbox"].shape == (2, rows, 4)
    assert pan["isthing"].dtype == torch.bool and pan["category_id"].dtype == torch.int64
    assert torch.equal(pan["id"][0].cpu(), torch.arange(1, rows + 1, dtype=torch.int32))
    assert int(pan["isthing"].sum()) == 200
    # every claimed pixel belongs to a valid segment
    for n in range(2):
        ids = torch.unique(pan["panoptic_seg"][n])
        ids = ids[ids > 0].long()
        assert torch.all(pan["is_valid"][n][ids - 1])


def test_semantic_segmentor_matches_the_panoptic_model(dev, panoptic):
    from detectron2_tensorflow_amd.modeling import SemanticSegmentor, build_model
    seg = build_model(_cfg(False, "SemanticSegmentor")).to(dev).eval()
    assert type(seg) is SemanticSegmentor
    state = {k: v for k, v in panoptic.state_dict().items()
             if k.split(".")[0] in ("backbone", "neck", "sem_seg_head")}
    seg.load_state_dict(state, strict=True)
    with torch.no_grad():
        a = seg(_images(dev))
        b = panoptic(_images(dev))
    assert set(a) == {"sem_seg"} and torch.equal(a["sem_seg"], b["sem_seg"])


def test_panoptic_fpn_training_step(dev):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.layers import ops
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 0, dev)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 54, (2, 256, 320), generator=g, dtype=torch.int32)
    labels[torch.rand(2, 256, 320, generator=g) < 0.2] = IGNORE
    batch["sem_seg"] = labels.to(dev)
    calibrate_rcnn_scores(model, batch)
    seen = {}
    hook = model.sem_seg_head.register_forward_hook(
        lambda mod, inp, out: seen.update(logits=out[0].detach(), loss=out[1]["loss_sem_seg"].detach()))
    losses = Trainer(cfg, model).step(batch)
    hook.remove()
    _C.raise_on_errors(dev)
    assert set(losses) == {"loss_sem_seg", "loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls",
                           "loss_rpn_loc", "total_loss"}
    for k, v in losses.items():
        assert torch.isfinite(v).all() and float(v) >= 0.0, (k, v)
    # the head's loss is ops.sem_seg_loss on its own stride-4 logits ...
    logits = seen["logits"]
    assert logits.shape == (2, 64, 80, LDC) and torch.all(logits[..., C:] == 0)
    shapes = batch["image_shape"].to(torch.int32)
    again = ops.sem_seg_loss(logits, batch["sem_seg"], shapes, IGNORE, 4, 0.5, num_classes=C)
    assert torch.equal(again, seen["loss"]) and torch.equal(losses["loss_sem_seg"], seen["loss"])
    # ... which is the reference's resize + cross-entropy of them
    cpu = logits.cpu()
    w64, _ = loss_reference(cpu, labels, shapes.cpu(), 0.5, 1.0, torch.float64)
    w32, _ = loss_reference(cpu, labels, shapes.cpu(), 0.5, 1.0, torch.float32)
    close_enough(again, w64, w32, "loss")
    # the semantic head trains: its parameters moved
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.sem_seg_head.parameters())
