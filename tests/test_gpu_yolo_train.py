"""GPU tests of YOLOv4 training: ops.yolov4_loss (csrc/yolo_loss.hip: the
target assignment, the fused CIoU loss and its backward) against the float64
line-by-line restatement of the reference (tests/yolo_train_reference.py),
the tensor arm on the GPU, and one eager Trainer step of the shipped config
built in the training phase.

Tolerance of every floating-point comparison (``allowed``): the restatement
is run once more in float32 on the CPU; its error against the float64 result
-- per loss |l32 - l64| / |l64|, per gradient tensor max|g32 - g64| / max|g64|
-- is the reference's own float32 error for that input.  The kernel is
allowed 4 x that (its summation order and its closed-form derivatives differ
from torch's, neither privileged), with a floor of 2 ulp of the value
(2 * 2^-23 relative).  Discrete outputs (slot, owner, state, counts) are
exact: every case's maximum CIoU stays 1e-4 or more away from the threshold
in float64 (asserted), two hundred times the float32 error of a CIoU.

Measured on an MI355X (relative errors; each test prints its own figures):
losses -- reference float32 2.0e-9 .. 1.2e-7, kernel 2.0e-9 .. 6.5e-8 (allowed
2.4e-7 .. 4.9e-7); gradient tensors -- reference float32 2.9e-9 .. 2.6e-7,
kernel 2.9e-9 .. 2.6e-7 (allowed 2.4e-7 .. 1.0e-6).  The table per case is in
DESIGN.md section 5, "YOLOv4 training".
"""
import os

import pytest
import torch

import yolo_train_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
THRESH, CLS_NORM, IOU_NORM = 0.5, 1.0, 0.07
UP = {"conf_loss": 0.7, "cls_loss": 1.3, "box_loss": 2.1}   # distinct upstream gradients, none 1
LOSSES = ("conf_loss", "cls_loss", "box_loss")
ULP2 = 2.0 * 2.0 ** -23
GT_CHUNK = 64  # csrc/yolo_loss.hip kGtChunk


def _hand_made():
    logits, gt, _ = R.hand_made_case()
    return logits, gt, 3, (64, 96)


# name -> (logits, gt, K, image_hw).  "chunked": 70 valid GT, more than the 64
# the forward kernel stages in LDS at a time; "tiny": P = 63, under one wave.
CASES = {
    "hand_made": _hand_made,
    "k80": lambda: R.random_case(3, 2, 80, 64, 96, 16, 10) + (80, (64, 96)),
    "k3": lambda: R.random_case(5, 2, 3, 64, 96, 16, 10) + (3, (64, 96)),
    "tiny": lambda: R.random_case(4, 1, 3, 32, 32, 4, 3) + (3, (32, 32)),
    "chunked": lambda: R.random_case(7, 2, 3, 64, 96, 80, 70) + (3, (64, 96)),
}
_ref = {}


def reference(name):
    """The case, its float64 result and gradients, and the float32
    restatement's error against them: computed once, never modified."""
    if name not in _ref:
        logits, gt, K, hw = CASES[name]()
        out = R.losses(logits, gt, K, THRESH, CLS_NORM, IOU_NORM, hw)
        grads = R.gradients(out, UP)
        o32 = R.losses(logits, gt, K, THRESH, CLS_NORM, IOU_NORM, hw, dtype=torch.float32)
        g32 = R.gradients(o32, UP)
        assert torch.equal(o32["state"], out["state"])
        err = {k: rel(o32[k].detach(), out[k].detach()) for k in LOSSES}
        gerr = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(g32, grads)]
        _ref[name] = dict(logits=logits, gt=gt, K=K, hw=hw, out=out, grads=grads, err=err, gerr=gerr,
                          margin=R.threshold_margin(out, THRESH))
    return _ref[name]


def allowed(ref_err):
    return max(4.0 * ref_err, ULP2)


def valid_of(gt):
    return gt["is_valid"] & ~gt["gt_is_crowd"] & ~gt["gt_difficult"]


def run_op(ref, dev, fn=None, requires_grad=True):
    from detectron2_tensorflow_amd.layers import ops
    fn = fn or ops.yolov4_loss
    gt = ref["gt"]
    lv = [x.to(dev).requires_grad_(requires_grad) for x in ref["logits"]]
    dbg = {}
    out = fn(lv, R.STRIDES, R.cell_anchors(), R.SCALE_YX, ref["K"], gt["gt_boxes"].to(dev),
             gt["gt_classes"].to(dev), valid_of(gt).to(dev), ref["hw"], THRESH, CLS_NORM, IOU_NORM,
             debug=dbg)
    return lv, out, dbg


def expected_slot_owner(ref):
    """slot [N, G] by the package's dense assignment in float64 (checked
    against the literals and the restatement in tests/test_yolo_train_cpu.py)
    and owner [N, P], the highest GT index of each slot; the caller checks the
    owners against the restatement's positives."""
    from detectron2_tensorflow_amd.modeling.single_stage_heads import yolov4_outputs as Y
    gt = ref["gt"]
    grid = [(int(x.shape[1]), int(x.shape[2])) for x in ref["logits"]]
    slot, _ = Y.assign(None, gt["gt_boxes"].double(), valid_of(gt), R.STRIDES, R.cell_anchors(), grid)
    N, P = ref["out"]["state"].shape
    owner = torch.full((N, P), -1, dtype=torch.int64)
    for n in range(N):
        for g, s in enumerate(slot[n].tolist()):
            if s >= 0:
                owner[n, s] = max(int(owner[n, s]), g)
    return slot, owner


def rel(got, want):
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    return abs(got - want) / max(abs(want), 1e-300)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(CASES))
def test_forward_against_float64(dev, name):
    ref = reference(name)
    assert ref["margin"] >= 1e-4, ref["margin"]
    if name == "chunked":
        assert int(valid_of(ref["gt"]).sum(1).max()) > GT_CHUNK
    _, (conf, cls, box, npos, nneg), dbg = run_op(ref, dev, requires_grad=False)
    out = ref["out"]
    slot, owner = expected_slot_owner(ref)
    assert (owner >= 0).eq(out["state"] == 2).all()
    assert torch.equal(dbg["slot"].cpu().long(), slot)
    assert torch.equal(dbg["owner"].cpu().long(), owner)
    assert torch.equal(dbg["state"].cpu(), out["state"])
    assert int(npos) == out["num_pos"] and int(nneg) == out["num_neg"]
    assert out["num_pos"] > 0 and out["num_neg"] > 0
    for k, got in zip(LOSSES, (conf, cls, box)):
        e = rel(got, out[k])
        print(f"{name} {k}: reference f32 {ref['err'][k]:.3e}, kernel {e:.3e}, "
              f"allowed {allowed(ref['err'][k]):.3e}")
    for k, got in zip(LOSSES, (conf, cls, box)):
        assert got.dtype == torch.float32 and rel(got, out[k]) <= allowed(ref["err"][k]), k


# ----------------------------------------------------------------- backward
def untouched(ref):
    """Per level, the elements no loss reaches: the class logits and the four
    box terms of every non-positive, and the conf logit of a "neither"."""
    K = ref["K"]
    st = ref["out"]["state"]
    masks, p0 = [], 0
    for x in ref["logits"]:
        N, H, W, _ = x.shape
        n = H * W * 3
        s = st[:, p0:p0 + n].reshape(N, H, W, 3, 1)
        m = torch.zeros((N, H, W, 3, 5 + K), dtype=torch.bool)
        m[..., :4] = s != 2
        m[..., 5:] = s != 2
        m[..., 4:5] = s == 0
        masks.append(m.reshape(N, H, W, -1))
        p0 += n
    return masks


@pytest.mark.parametrize("name", list(CASES))
def test_backward_against_float64_autograd(dev, name):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers import ops
    ref = reference(name)
    lv, (conf, cls, box, _, _), dbg = run_op(ref, dev)
    total = UP["conf_loss"] * conf + UP["cls_loss"] * cls + UP["box_loss"] * box
    got = torch.autograd.grad(total, lv)
    for l, (g, want, m) in enumerate(zip(got, ref["grads"], untouched(ref))):
        g = g.cpu()
        assert (want[m] == 0).all()            # the restatement agrees that nothing reaches them
        assert (g[m] == 0).all(), f"level {l}: an untouched element is not exactly 0"
        e = float((g.double() - want).abs().max() / want.abs().max())
        print(f"{name} d_logits[{l}]: reference f32 {ref['gerr'][l]:.3e}, kernel {e:.3e}, "
              f"allowed {allowed(ref['gerr'][l]):.3e}")
    for l, (g, want) in enumerate(zip(got, ref["grads"])):
        e = float((g.cpu().double() - want).abs().max() / want.abs().max())
        assert e <= allowed(ref["gerr"][l]), (l, e)
    # the C entry writes EVERY element: buffers the test owns, pre-filled with NaN
    gt = ref["gt"]
    hw = [(x.shape[1], x.shape[2]) for x in lv]
    lhw, st, chw, sc, L, A = ops.yolo_host_arrays(hw, R.STRIDES, R.cell_anchors(), R.SCALE_YX)
    N = lv[0].shape[0]
    logits = [x.detach().contiguous() for x in lv]
    bufs = [torch.full_like(x, float("nan")) for x in logits]
    gb = gt["gt_boxes"].to(dev).float().contiguous()
    gc = gt["gt_classes"].to(dev).long().contiguous()
    ups = [torch.tensor(UP[k], dtype=torch.float32, device=dev) for k in LOSSES]
    rc = _C.lib().d2mi_yolov4_loss_bwd(
        _C.host_array(_C.c_void_p, [t.data_ptr() for t in logits]),
        _C.host_array(_C.c_void_p, [t.data_ptr() for t in bufs]), lhw, st, chw, sc, L, A, ref["K"], N,
        _C.ptr(gb), _C.ptr(gc), gb.shape[1], _C.ptr(dbg["slot"]), _C.ptr(dbg["owner"]),
        _C.ptr(dbg["state"]), float(ref["hw"][0] * ref["hw"][1]), IOU_NORM, 1.0 / N, CLS_NORM / N,
        _C.ptr(ups[0]), _C.ptr(ups[1]), _C.ptr(ups[2]), _C.stream_of(dev))
    _C.check(rc, "d2mi_yolov4_loss_bwd")
    for b, g in zip(bufs, got):
        assert torch.equal(b, g)  # no NaN left, and the bits of the autograd path


def test_two_runs_are_bit_identical(dev):
    ref = reference("chunked")  # collisions: many GT per slot, the integer max decides
    runs = []
    for _ in range(2):
        lv, out, dbg = run_op(ref, dev)
        total = UP["conf_loss"] * out[0] + UP["cls_loss"] * out[1] + UP["box_loss"] * out[2]
        runs.append((out, torch.autograd.grad(total, lv), dbg))
    (o1, g1, d1), (o2, g2, d2) = runs
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(torch.equal(d1[k], d2[k]) for k in d1)


@pytest.mark.parametrize("kind", ["no_gt", "all_invalid"])
def test_no_valid_gt_gives_zero_losses_and_gradients(dev, kind):
    from detectron2_tensorflow_amd import _C
    ref = dict(reference("k3"))
    gt = {k: v.clone() for k, v in ref["gt"].items()}
    if kind == "no_gt":
        gt = {k: v[:, :0] for k, v in gt.items()}
    else:
        gt["is_valid"][:] = False
    ref["gt"] = gt
    lv, out, dbg = run_op(ref, dev)
    _C.raise_on_errors(dev)
    assert all(v.item() == 0 for v in out)
    assert (dbg["owner"] == -1).all() and (dbg["state"] == 0).all() and (dbg["slot"] == -1).all()
    grads = torch.autograd.grad(out[0] + out[1] + out[2], lv)
    assert all((g == 0).all() for g in grads)


@pytest.mark.parametrize("name", ["hand_made", "k80"])
def test_fused_and_tensor_arms_agree_on_the_gpu(dev, name):
    """The tensor arm in float32 is another float32 evaluation of the same
    loss: each arm is allowed 4 x the reference's float32 error (floor 2 ulp)
    against float64, so the two differ by at most twice that."""
    from detectron2_tensorflow_amd.modeling.single_stage_heads import yolov4_outputs as Y
    ref = reference(name)
    lf, of, df = run_op(ref, dev)
    lt, ot, dt = run_op(ref, dev, fn=Y.yolov4_losses_dense)
    assert int(of[3]) == int(ot[3]) and int(of[4]) == int(ot[4])
    assert torch.equal(df["state"], dt["state"]) and torch.equal(df["slot"].long(), dt["slot"])
    assert torch.equal(df["owner"].long(), dt["owner"])
    for k, a, b in zip(LOSSES, of, ot):
        assert rel(a, b) <= 2 * allowed(ref["err"][k]), (k, float(a), float(b))
    gf = torch.autograd.grad(sum(UP[k] * v for k, v in zip(LOSSES, of)), lf)
    gtn = torch.autograd.grad(sum(UP[k] * v for k, v in zip(LOSSES, ot)), lt)
    for l, (a, b) in enumerate(zip(gf, gtn)):
        assert float((a - b).abs().max() / b.abs().max()) <= 2 * allowed(ref["gerr"][l]), l


# ---------------------------------------------------- one eager Trainer step
def test_trainer_step_of_the_shipped_config(dev, monkeypatch):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.layers import BatchNorm
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.modeling.single_stage_heads import yolov4_outputs as Y
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    from detectron2_tensorflow_amd.utils.training import set_training_phase
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-Detection", "yolov4_D_53_PAN_1x.yaml"))
    finalize(cfg, True, 1, CATS)
    torch.manual_seed(0)
    try:
        model = build_model(cfg)
    finally:
        set_training_phase(False)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # the perturbation of test_gpu_yolo.py::yolo_model
        for m in model.modules():
            if isinstance(m, BatchNorm):
                m.gamma.copy_(torch.rand(m.gamma.shape, generator=g) + 0.5)
                m.beta.copy_(torch.randn(m.beta.shape, generator=g) * 0.1)
                m.moving_mean.copy_(torch.randn(m.moving_mean.shape, generator=g) * 0.1)
                m.moving_variance.copy_(torch.rand(m.moving_variance.shape, generator=g) + 0.5)
        for pred in model.detector.head.preds:
            pred.bias.copy_(torch.randn(pred.bias.shape, generator=g) * 2 - 2)
    model = model.to(dev).train()
    assert model.detector.built_for_training
    batch = synthetic_train_batch(2, 64, 96, 3, dev, num_gt=5, sqrt_area=(8.0, 48.0))
    bns = [m for m in model.modules() if isinstance(m, BatchNorm)]
    live = [m for m in bns if m.batch_stats]
    assert live and len(live) < len(bns)
    # the head's logits of this batch, and both arms' losses on them
    seen = {}
    hook = model.detector.head.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o))
    with torch.no_grad():
        monkeypatch.setattr(Y, "FUSED_YOLO_LOSS", False)
        tensor_arm = model(batch)
        monkeypatch.setattr(Y, "FUSED_YOLO_LOSS", True)
        fused_arm = model(batch)
    hook.remove()
    logits = [t.detach().cpu() for t in seen["logits"]]
    gt = {k: v.cpu() for k, v in batch["instances"].items()}
    hw = (64, 96)
    out = R.losses(logits, gt, 80, THRESH, CLS_NORM, IOU_NORM, hw)
    o32 = R.losses(logits, gt, 80, THRESH, CLS_NORM, IOU_NORM, hw, dtype=torch.float32)
    assert R.threshold_margin(out, THRESH) >= 1e-4
    for k in LOSSES:
        tol = allowed(rel(o32[k], out[k]))
        assert rel(fused_arm[k], out[k]) <= tol and rel(tensor_arm[k], out[k]) <= tol, k
    before = [(m.moving_mean.clone(), m.moving_variance.clone()) for m in bns]
    losses = Trainer(cfg, model).step(batch)
    _C.raise_on_errors(dev)
    assert set(LOSSES) <= set(losses)
    assert all(torch.isfinite(v).all() for v in losses.values()), losses
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    for pred in model.detector.head.preds:
        assert (pred.bias.grad != 0).any()
    for m, (mm, mv) in zip(bns, before):
        changed = not torch.equal(m.moving_mean, mm) and not torch.equal(m.moving_variance, mv)
        assert changed == m.batch_stats
