"""GPU tests of YOLOv4 inference: the dense predictions and the fused
threshold + NMS (d2mi_yolov4_*) against tests/yolo_reference.py, the SPP pool
and the activation kernels, and the whole model built from the shipped
config."""
import os

import numpy as np
import pytest
import torch

import yolo_reference as yref
from test_gpu_ops import assert_boxes_close

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}

STRIDES = [8, 16, 32]
CELL_HW = [np.array([[16, 12], [36, 19], [28, 40]], F32), np.array([[75, 36], [55, 76], [146, 72]], F32),
           np.array([[110, 142], [243, 192], [410, 459]], F32)]
SCALE_YX = [1.2, 1.1, 1.05]
SMALL = [(12, 8), (6, 4), (3, 2)]       # P = 378
LARGE = [(56, 56), (28, 28), (14, 14)]  # P = 12,348 > kLdsSortCap = 8,192
E2E_SEED = 5  # test_fused_inference_end_to_end asserts the reference's margins for it


def ops():
    from detectron2_tensorflow_amd.layers import ops as _ops
    return _ops


def make_case(seed, N, K, hw, quantized=False, conf_mean=-2.0, cls_mean=-2.0, cell_hw=None,
              dhdw=1.0, thresh=0.05, max_det=100):
    """Finite logits with |raw_dhdw| <= 4: (dy, dx) ~ N(0, 2), (dh, dw) ~ N(0, dhdw)
    clipped, conf ~ N(conf_mean, 2), classes ~ N(cls_mean, 2)."""
    rng = np.random.default_rng(seed)
    A = 3
    logits = []
    for h, w in hw:
        x = rng.normal(0, 2, size=(N, h, w, A, 5 + K))
        x[..., 2:4] = np.clip(rng.normal(0, dhdw, size=x[..., 2:4].shape), -4, 4)
        x[..., 4] = rng.normal(conf_mean, 2, size=x[..., 4].shape)
        x[..., 5:] = rng.normal(cls_mean, 2, size=x[..., 5:].shape)
        if quantized:
            x = np.round(x * 4) / 4
        logits.append(x.reshape(N, h, w, A * (5 + K)).astype(F32))
    return {"logits": logits, "strides": STRIDES, "cell_hw": cell_hw or CELL_HW, "scale_yx": SCALE_YX,
            "num_classes": K, "thresh": thresh, "nms_thresh": 0.5, "max_det": max_det}


def hand_made():
    return yref.hand_made_case()[0]


CASES = {
    "hand_made": hand_made,
    "k80": lambda: make_case(1, 2, 80, SMALL),
    "k80_quantized": lambda: make_case(2, 2, 80, SMALL, quantized=True),
    "k1": lambda: make_case(3, 2, 1, SMALL, conf_mean=0.0),
}

_dense_cache = {}


def cell_anchors(case):
    return [np.concatenate([np.zeros_like(c), c], 1) for c in case["cell_hw"]]


def dense_on_gpu(name, case, dev):
    """The kernel's dense predictions of a case, computed once per session."""
    if name not in _dense_cache:
        out = ops().yolov4_predictions([torch.from_numpy(x).to(dev) for x in case["logits"]],
                                       case["strides"], cell_anchors(case), case["scale_yx"],
                                       case["num_classes"])
        _dense_cache[name] = tuple(t.cpu().numpy() for t in out)
    return _dense_cache[name]


def fused_on_gpu(case, dev, **over):
    c = dict(case, **over)
    out = ops().yolov4_inference([torch.from_numpy(x).to(dev) for x in c["logits"]], c["strides"],
                                 cell_anchors(c), c["scale_yx"], c["num_classes"], c["thresh"],
                                 c["nms_thresh"], c["max_det"])
    return tuple(t.cpu().numpy() for t in out)


def ulps(got, want):
    """|got - want| in units of want's float32 spacing."""
    want = np.asarray(want, F32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))


# ------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("name", list(CASES))
def test_dense_predictions_vs_reference(dev, name):
    """Boxes within assert_boxes_close; conf within 2 ulp (one sigmoid, as
    assert_sigmoid_scores_close states); score within 5 ulp (two such
    sigmoids, 2 + 2, and the product's rounding).  cls is exact wherever the
    reference's best and second-best products differ by more than 8 ulp, and
    also where they are equal because their logits are (the tie groups of the
    quantized case: tf.argmax's lowest index is then required); elsewhere
    either of the two classes is accepted, and such predictions are under 1 %
    of the case (checked on the CPU side first)."""
    case = CASES[name]()
    K = case["num_classes"]
    wb, wc, ws, wk, prob = yref.predictions(case["logits"], case["strides"], case["cell_hw"],
                                            case["scale_yx"], K)
    N, P = wc.shape
    raw = np.concatenate([x.reshape(N, -1, 5 + K)[..., 5:] for x in case["logits"]], 1)
    if K > 1:
        order = np.argsort(-prob, axis=-1, kind="stable")
        i1, i2 = order[..., 0], order[..., 1]
        take = lambda a, i: np.take_along_axis(a, i[..., None], -1)[..., 0]  # noqa: E731
        best, second = take(prob, i1), take(prob, i2)
        assert np.array_equal(i1, wk)
        same_input = take(raw, i1) == take(raw, i2)
        lenient = ((best - second) <= 8 * np.spacing(best)) & ~same_input
    else:
        i2 = np.zeros_like(wk)
        lenient = np.zeros(wk.shape, bool)
    assert lenient.mean() < 0.01, lenient.mean()
    gb, gc, gs, gk = dense_on_gpu(name, case, dev)
    assert gb.shape == (N, P, 4) and gk.dtype == np.int32
    assert_boxes_close(gb, wb)
    print(f"{name}: conf max {ulps(gc, wc).max():.2f} ulp, score max {ulps(gs, ws).max():.2f} ulp, "
          f"lenient {int(lenient.sum())} of {lenient.size}")
    assert ulps(gc, wc).max() <= 2
    assert ulps(gs, ws).max() <= 5
    ok = (gk == wk) | (lenient & (gk == i2))
    assert ok.all(), (int((~ok).sum()), gk[~ok][:5], wk[~ok][:5])


# ------------------------------------------------------ 2. fused vs select
def assert_fused_equals_select(got, dense, case):
    """Bit-equal: the fused op against yref.select on the kernel's own dense
    boxes / scores / classes (identical inputs: no tolerance)."""
    gb, gc, gs, gk = dense
    want = yref.select(gb, gs, gk, case["thresh"], case["nms_thresh"], case["max_det"])
    for g, w, k in zip(got, want, ("boxes", "scores", "classes", "is_valid")):
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert np.array_equal(g.view(np.uint8) if g.dtype == F32 else g,
                              w.view(np.uint8) if w.dtype == F32 else w), k
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_fused_inference_equals_select_on_own_dense(dev, name):
    case = CASES[name]()
    want = assert_fused_equals_select(fused_on_gpu(case, dev), dense_on_gpu(name, case, dev), case)
    assert want[3].any()


def test_fused_inference_nothing_passes(dev):
    case = CASES["k80"]()
    got = fused_on_gpu(case, dev, thresh=1.5)
    assert_fused_equals_select(got, dense_on_gpu("k80", case, dev), dict(case, thresh=1.5))
    assert not got[3].any()
    assert not got[0].any() and not got[1].any() and not got[2].any()


def test_fused_inference_pads_when_few_survive(dev):
    case = CASES["k80"]()
    dense = dense_on_gpu("k80", case, dev)
    thresh = float(np.sort(dense[2][0])[-8])  # 7 scores of image 0 above it
    got = fused_on_gpu(case, dev, thresh=thresh)
    want = assert_fused_equals_select(got, dense, dict(case, thresh=thresh))
    nv = want[3].sum(1)
    assert 1 <= nv[0] <= 7 and (nv < case["max_det"]).all()
    for n in range(got[0].shape[0]):
        assert got[3][n, :nv[n]].all() and not got[3][n, nv[n]:].any()
        assert not got[0][n, nv[n]:].any() and not got[1][n, nv[n]:].any()


@pytest.mark.parametrize("boxes", ["scattered", "coincident"])
def test_fused_inference_merge_sort_path(dev, boxes):
    """P = 12,348 and every prediction passes: more candidates than
    kLdsSortCap = 8,192, so the sort takes its tile + merge path.  Scattered
    2 px boxes: the scan stops early at 100 kept.  Boxes of ~3,000 px that
    all but coincide: the scan walks every candidate and keeps fewer."""
    if boxes == "scattered":
        cells, dhdw = [np.full((3, 2), 2.0, F32)] * 3, 0.2
    else:
        cells, dhdw = [np.full((3, 2), 3000.0, F32)] * 3, 0.01
    case = make_case(4, 1, 4, LARGE, conf_mean=12.0, cls_mean=2.0, cell_hw=cells, dhdw=dhdw)
    name = "large_" + boxes
    dense = dense_on_gpu(name, case, dev)
    P = dense[2].shape[1]
    assert P == 12348 and (dense[2] > case["thresh"]).all()
    want = assert_fused_equals_select(fused_on_gpu(case, dev), dense, case)
    if boxes == "scattered":
        assert want[3].sum() == 100
    else:
        assert 1 <= want[3].sum() < 100


def test_fused_inference_images_are_independent(dev):
    case = make_case(6, 3, 80, SMALL)
    dense = dense_on_gpu("n3", case, dev)
    got = fused_on_gpu(case, dev)
    assert_fused_equals_select(got, dense, case)
    assert len({got[3][n].sum() for n in range(3)}) > 1 or not np.array_equal(got[0][0], got[0][1])
    for n in range(3):
        one = fused_on_gpu(dict(case, logits=[x[n:n + 1] for x in case["logits"]]), dev)
        for g, o in zip(got, one):
            assert np.array_equal(g[n], o[0])


# --------------------------------------------------------- 3. end to end
def tf_iou_matrix(b):
    """oracle_nms's IoU (corner-normalised, float32) of every pair of rows."""
    b = np.asarray(b, F32)
    y0, x0 = np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3])
    y1, x1 = np.maximum(b[:, 0], b[:, 2]), np.maximum(b[:, 1], b[:, 3])
    area = (y1 - y0) * (x1 - x0)
    ih = np.maximum(np.minimum(y1[:, None], y1[None]) - np.maximum(y0[:, None], y0[None]), F32(0))
    iw = np.maximum(np.minimum(x1[:, None], x1[None]) - np.maximum(x0[:, None], x0[None]), F32(0))
    inter = ih * iw
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((area[:, None] > 0) & (area[None] > 0),
                        inter / (area[:, None] + area[None] - inter), F32(0))


def assert_reference_margins(case, exact_at_threshold=0):
    """The decisions of yref.inference on this case survive an ulp of expf:
    no score within 1e-5 (relative) of the threshold, no two distinct
    adjacent scores of the sorted survivors within 1e-5 (relative), no IoU of
    two survivors within 1e-5 of the NMS threshold."""
    boxes, _, score, _, _ = yref.predictions(case["logits"], case["strides"], case["cell_hw"],
                                             case["scale_yx"], case["num_classes"])
    t = case["thresh"]
    for n in range(score.shape[0]):
        near = np.abs(score[n].astype(np.float64) - t) <= 1e-5 * t
        assert near.sum() == exact_at_threshold, score[n][near]
        idx = np.nonzero(score[n] > F32(t))[0]
        s = np.sort(score[n][idx].astype(np.float64))
        gap = np.diff(s)
        assert not ((gap > 0) & (gap <= 1e-5 * s[1:])).any()
        iou = tf_iou_matrix(boxes[n][idx])
        assert not (np.abs(iou.astype(np.float64) - case["nms_thresh"]) <= 1e-5).any()


@pytest.mark.parametrize("name", ["hand_made", "k80_e2e"])
def test_fused_inference_end_to_end(dev, name):
    """Against yref.inference, decisions exact.  The hand-made case's scores
    are exact in any arithmetic (sigmoid of 0 and of +-40), one of them
    exactly at the threshold by design; the seeded case's margins are asserted
    first."""
    if name == "hand_made":
        case, expected = yref.hand_made_case()
        assert_reference_margins(case, exact_at_threshold=1)
    else:
        case = make_case(E2E_SEED, 2, 80, SMALL)
        assert_reference_margins(case)
    wb, ws, wk, wv = yref.inference(case["logits"], case["strides"], case["cell_hw"],
                                    case["scale_yx"], case["num_classes"], case["thresh"],
                                    case["nms_thresh"], case["max_det"])
    gb, gs, gk, gv = fused_on_gpu(case, dev)
    assert wv.any()
    assert np.array_equal(gv, wv) and np.array_equal(gk, wk)
    assert_boxes_close(gb, wb)
    assert ulps(gs[wv], ws[wv]).max() <= 5 and not gs[~wv].any()
    if name == "hand_made":
        for g, k in zip((gb, gs, gk, gv), ("boxes", "scores", "classes", "is_valid")):
            assert np.array_equal(g, expected[k]), k


# ------------------------------------------------------------------ 4. SPP
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 19, 19, 512), (2, 7, 20, 12)])
def test_spp_pool_bit_equal(dev, shape):
    """Mostly negative inputs: a -inf border instead of the zero one would show."""
    from detectron2_tensorflow_amd.layers import MaxPool2D
    rng = np.random.default_rng(shape[1])
    x = rng.normal(-1.0, 1.0, size=shape).astype(F32)
    assert (x < 0).mean() > 0.7
    xd = torch.from_numpy(x).to(dev)
    got = ops().spp_pool(xd)
    want = torch.cat([MaxPool2D(kernel_size=k)(xd) for k in (13, 9, 5)] + [xd], dim=3)
    assert got.shape == want.shape == shape[:3] + (4 * shape[3],)
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), yref.spp(x))
    assert torch.equal(xd, torch.from_numpy(x).to(dev))


def test_spp_module_uses_the_kernel_and_the_composition_with_a_gradient(dev):
    from detectron2_tensorflow_amd.modeling.necks import SPP
    spp = SPP(8, 4, scope="process1").to(dev)
    x = torch.randn(1, 6, 5, 4, device=dev) - 1
    with torch.no_grad():
        fused = spp.pool_concat(x)
    xg = x.clone().requires_grad_(True)
    comp = spp.pool_concat(xg)
    assert comp.requires_grad and torch.equal(fused, comp.detach())


# ----------------------------------------------------------- 5. activation
def activation_inputs():
    rng = np.random.default_rng(11)
    return np.concatenate([rng.normal(0, 3, size=100003), np.linspace(-30, 30, 24001),
                           np.zeros(5), rng.uniform(-30, 30, size=1000)]).astype(F32)


def test_mish_error_and_leaky_relu_bits(dev):
    """Mish against a float64 evaluation rounded to float32; the error of the
    torch composition x * tanh(softplus(x)) is measured on the same inputs,
    and the kernel's maximum error must not exceed the larger of it and
    2 ulp.  Inputs: normal values, |x| up to 30 (softplus saturates), zeros, a
    length that is no multiple of 4, and a view that is not 16-byte aligned.
    Leaky ReLU is bit-equal to F.leaky_relu(x, 0.1)."""
    import torch.nn.functional as F
    x = activation_inputs()
    assert x.size % 4 != 0
    x64 = x.astype(np.float64)
    exact = x64 * np.tanh(np.log1p(np.exp(x64)))
    ref32 = exact.astype(F32)
    unit = np.spacing(np.abs(ref32)).astype(np.float64)
    xd = torch.from_numpy(x).to(dev)
    comp = (xd * torch.tanh(F.softplus(xd))).cpu().numpy()
    got = ops().activation_(xd.clone(), ops().ACT_MISH).cpu().numpy()
    err_torch = (np.abs(comp.astype(np.float64) - exact) / unit).max()
    err_kernel = (np.abs(got.astype(np.float64) - exact) / unit).max()
    print(f"mish max error: kernel {err_kernel:.3f} ulp, torch composition {err_torch:.3f} ulp")
    assert err_kernel <= max(err_torch, 2.0), (err_kernel, err_torch)
    assert not got[x == 0].any()
    # an unaligned view (4 bytes past a 16-byte boundary), every length 1..9
    base = torch.from_numpy(np.concatenate([[0.0], x[:64]]).astype(F32)).to(dev)
    for n in range(1, 10):
        buf = base.clone()
        view = buf[1:1 + n]
        assert view.data_ptr() % 16 == 4
        ops().activation_(view, ops().ACT_MISH)
        assert np.array_equal(buf[1:1 + n].cpu().numpy(), got[:n])
        assert torch.equal(buf[1 + n:], base[1 + n:]) and torch.equal(buf[:1], base[:1])
    lk = ops().activation_(xd.clone(), ops().ACT_LEAKY_RELU, 0.1)
    assert torch.equal(lk, F.leaky_relu(xd, 0.1))
    buf = base.clone()
    ops().activation_(buf[1:], ops().ACT_LEAKY_RELU, 0.1)
    assert torch.equal(buf[1:], F.leaky_relu(base[1:], 0.1)) and torch.equal(buf[:1], base[:1])


def test_get_activation_dispatch(dev, monkeypatch):
    from detectron2_tensorflow_amd.layers import activation, get_activation
    x = torch.from_numpy(activation_inputs()[:1001]).to(dev)
    want = ops().activation_(x.clone(), ops().ACT_MISH)
    with torch.no_grad():
        y = x.clone()
        out = get_activation("mish")(y)
        assert out.data_ptr() == y.data_ptr() and torch.equal(out, want)     # one in-place pass
        z = x.clone()
        assert get_activation("leaky_relu")(z).data_ptr() == z.data_ptr()
        assert torch.equal(z, torch.nn.functional.leaky_relu(x, 0.1))
    xg = x.clone().requires_grad_(True)                                       # needs a gradient
    yg = get_activation("mish")(xg)
    assert yg.requires_grad and torch.equal(xg.detach(), x)
    monkeypatch.setattr(activation, "FUSED", False)
    with torch.no_grad():
        y = x.clone()
        out = get_activation("mish")(y)
        assert torch.equal(y, x) and torch.equal(out, x * torch.tanh(torch.nn.functional.softplus(x)))


# ---------------------------------------------------------- 6. whole model
@pytest.fixture(scope="module")
def yolo_model(dev):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.layers import BatchNorm
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-Detection", "yolov4_D_53_PAN_1x.yaml"))
    finalize(cfg, False, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, BatchNorm):  # so that the fold matters
                m.gamma.copy_(torch.rand(m.gamma.shape, generator=g) + 0.5)
                m.beta.copy_(torch.randn(m.beta.shape, generator=g) * 0.1)
                m.moving_mean.copy_(torch.randn(m.moving_mean.shape, generator=g) * 0.1)
                m.moving_variance.copy_(torch.rand(m.moving_variance.shape, generator=g) + 0.5)
        for pred in model.detector.head.preds:  # scores spread around the threshold
            pred.bias.copy_(torch.randn(pred.bias.shape, generator=g) * 2 - 2)
    return model.to(dev).eval()


def yolo_inputs(dev, shape):
    g = torch.Generator().manual_seed(shape[1])
    img = (torch.rand(shape + (3,), generator=g) * 255).to(dev)
    return {"image": img, "image_shape": torch.tensor([list(shape[1:])] * shape[0], device=dev)}


def head_logits(model, inp):
    images = model.preprocess_image(inp)
    c = model.backbone(images.tensor)
    p = model.neck(c)
    logits = model.detector.head([p[f] for f in model.detector.in_features])
    return images, c, p, logits


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 70, 100)])
def test_yolov4_model_forward(dev, yolo_model, shape, monkeypatch):
    from detectron2_tensorflow_amd.layers import Conv2D, activation
    from detectron2_tensorflow_amd.modeling.necks import SPP
    model = yolo_model
    inp = yolo_inputs(dev, shape)
    with torch.no_grad():
        images, c, p, logits = head_logits(model, inp)
        out = model(inp)["instances"]
        again = model(inp)["instances"]
    H, W = images.tensor.shape[1:3]
    assert H % 32 == 0 and W % 32 == 0 and H >= shape[1] and W >= shape[2]
    assert [tuple(t.shape[1:]) for t in logits] == [(H // s, W // s, 255) for s in (8, 16, 32)]
    for k in out:  # two runs are bit-identical
        assert torch.equal(out[k], again[k]), k
    # the instances: the threshold / NMS restatement on the kernel's dense
    # predictions of the model's own head logits, bit-equal
    head = model.detector
    ag = head.anchor_generator
    dense = tuple(t.cpu().numpy() for t in ops().yolov4_predictions(
        logits, ag.strides, ag.cell_anchors, head.scale_yx, head.num_classes))
    case = {"thresh": head.score_threshold, "nms_thresh": head.nms_threshold,
            "max_det": head.max_detections_per_image}
    got = tuple(out[k].cpu().numpy() for k in ("boxes", "scores", "classes", "is_valid"))
    want = assert_fused_equals_select(got, dense, case)
    assert 0 < want[3].sum() and (dense[2] <= case["thresh"]).any()
    # backbone, neck and tower against the same modules on torch's convs, the
    # torch activations and the MaxPool2D composition (the tolerance of
    # test_fpn_and_mask_head_logits_on_identical_inputs for conv stacks)
    convs = [m for m in model.modules() if isinstance(m, Conv2D)]
    for m in convs:
        monkeypatch.setattr(m, "impl", "torch")
    monkeypatch.setattr(activation, "FUSED", False)
    monkeypatch.setattr(SPP, "FUSED_POOL", False)
    with torch.no_grad():
        _, c_t, p_t, logits_t = head_logits(model, inp)
    pairs = [(f"backbone {k}", c[k], c_t[k]) for k in c] + [(f"neck {k}", p[k], p_t[k]) for k in p]
    pairs += [(f"tower {i}", a, b) for i, (a, b) in enumerate(zip(logits, logits_t))]
    for what, a, b in pairs:
        err = (a.double() - b.double()).abs().max().item()
        scale = b.abs().max().item()
        print(f"{what}: err {err:.3e} scale {scale:.3e}")
        assert np.isfinite(scale) and err <= 1e-4 * max(scale, 1.0), (what, err, scale)


def test_yolov4_model_under_graph_capture(dev, yolo_model):
    """The forward pass captures into a hipGraph (a host synchronisation
    inside the capture is an error) and its replay gives the eager output."""
    from detectron2_tensorflow_amd.utils import capture
    model = yolo_model
    inp = yolo_inputs(dev, (2, 64, 96))
    with torch.no_grad():
        eager = model(inp)["instances"]  # (also warms the folded / packed weight caches)
        torch.cuda.synchronize(dev)
        static = {k: v.clone() for k, v in inp.items()}
        graph = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream(device=dev)
        capture.begin(dev)
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            out = model(static)["instances"]
        keep = []
        capture.flush(keep)
        for v in out.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
    for k in eager:
        assert torch.equal(out[k], eager[k]), k
    assert out["is_valid"].any()
