"""SOLOv2 R50-FPN inference (BASELINE config C5): SingleStageDetector +
SOLOv2Head (lib/modeling/single_stage_heads/solo_v2.py:67-721) and the TF
ResizeBilinear kernel its head resamples with (lib/layers/functional.py:9-36).

CPU: known answers for the oracle's restatements (bilinear weights, linspace,
point NMS, the box-from-mask rule).
GPU: d2mi_resize_bilinear bit-exact vs the oracle; the inference tail
(ops.solo_inference) vs oracle/solo.py — probs to the sigmoid's 1 ulp, then,
fed the GPU's own probs and dynamic-conv logits, classes / valid flags /
pasted uint8 masks bit-exact, scores to 1e-5 relative (the mask score is a
f32 sum over the mask in a different order), boxes to max(1e-4, 2 ulp); the
dynamic-conv logits vs float64; the whole model at 256x320 vs the CPU
restatement (oracle/cpu_pipeline.py: CPUSOLOv2); and the 1333x800 geometry
(800x1344 padded: masks 200x336, 67,200 mask pixels) with determinism and
the reference's padded output layout.

Synthetic weights: random init with solo_cate / solo_kernel rescaled
(utils/synthetic.py: calibrate_solo_head) so a realistic number of
candidates pass SCORE_THRESH_TEST (BASELINE.md score injection)."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CM = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}


# ------------------------------------------------------------------ CPU KATs
def test_resize_bilinear_known_answers():
    """2x2 -> 4x4 half-pixel (scale 0.5): in = (i + 0.5) * 0.5 - 0.5 =
    -0.25, 0.25, 0.75, 1.25 -> (lo, hi, lerp) = (0,0,.75) (0,1,.25) (0,1,.75)
    (1,1,.25); downscale 4 -> 2 (scale 2): in = 0.5, 2.5."""
    import solo
    x = np.array([[0, 1], [2, 3]], F32).reshape(1, 2, 2, 1)
    y = solo.resize_bilinear_tf(x, 4, 4)[0, ..., 0]
    row = np.array([0, 0.25, 0.75, 1], F32)
    want = np.stack([row, row + 0.5, row + 1.5, row + 2.0])
    np.testing.assert_array_equal(y, want)
    x = np.arange(4, dtype=F32).reshape(1, 1, 4, 1)
    np.testing.assert_array_equal(solo.resize_bilinear_tf(x, 1, 2)[0, 0, :, 0], [0.5, 2.5])
    # align_corners (legacy scaler): scale (4-1)/(2-1) = 3 -> samples 0, 3
    np.testing.assert_array_equal(
        solo.resize_bilinear_tf(x, 1, 2, half_pixel=False, align_corners=True)[0, 0, :, 0], [0, 3])


def test_linspace_and_coords_known_answers():
    import solo
    np.testing.assert_array_equal(solo.linspace_tf(5), np.array([-1, -0.5, 0, 0.5, 1], F32))
    np.testing.assert_array_equal(solo.linspace_tf(1), np.array([-1], F32))
    c = solo.coord_channels(1, 2, 3)
    np.testing.assert_array_equal(c[0, :, :, 0], [[-1, 0, 1], [-1, 0, 1]])   # xx along W
    np.testing.assert_array_equal(c[0, :, :, 1], [[-1, -1, -1], [1, 1, 1]])  # yy along H


def test_point_nms_known_answer():
    """keep p where p >= its up, left and up-left neighbours (zero padded)."""
    import solo
    p = np.array([[0.2, 0.5, 0.1],
                  [0.6, 0.3, 0.7],
                  [0.1, 0.6, 0.2]], F32).reshape(1, 3, 3, 1)
    got = solo.point_nms(p)[0, ..., 0]
    want = np.array([[0.2, 0.5, 0.0],
                     [0.6, 0.0, 0.7],
                     [0.0, 0.6, 0.0]], F32)
    np.testing.assert_array_equal(got, want)


def test_boxes_from_masks_known_answer():
    """solo_v2.py:604-623 on a 1x1 -> 4x4 identity resize: a mask on rows 1-2,
    cols 2-3 gives (1, 2, 2, 3); a mask touching row / column 0 pulls in the
    mean (the zeros of y * mask are replaced by it); an empty mask gives 0."""
    import solo
    m = np.zeros((3, 4, 4), F32)
    m[0, 1:3, 2:4] = 1
    m[1, 0:2, 0:2] = 1      # rows 0-1: y-mean = (0+0+1+1)/4 = 0.5 -> ymin 0.5
    _, boxes = solo.masks_to_image(m.reshape(3, 16), 4, 4, 4, 4)
    np.testing.assert_array_equal(boxes[0], [1, 2, 2, 3])
    den = F32(4) + F32(1e-5)
    np.testing.assert_array_equal(boxes[1], [F32(2) / den, F32(2) / den, 1, 1])
    np.testing.assert_array_equal(boxes[2], [0, 0, 0, 0])


def _cfg():
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/COCO-InstanceSegmentation/solo_v2_R_50_FPN_1x.yaml"))
    finalize(cfg, False, 1, CM)
    return cfg


def test_solo_model_builds_with_reference_variables():
    """SOLOv2 R50-FPN: 46.6 M parameters; the heads' variables carry the
    reference scopes (solo_v2.py:192-218, :684-703)."""
    from detectron2_tensorflow_amd.modeling import build_model
    torch.manual_seed(0)
    m = build_model(_cfg())
    assert abs(sum(p.numel() for p in m.parameters()) / 1e6 - 46.59) < 0.05
    names = {n for n, _ in m.reference_variables(include_scope=False)}
    for want in ("head/mask_kernel/cate_subnet0/weights", "head/mask_kernel/cate_subnet0/norm/gamma",
                 "head/mask_kernel/kernel_subnet6/weights", "head/mask_kernel/solo_cate/bias",
                 "head/mask_kernel/solo_kernel/weights", "head/mask_feature/p5_4/weights",
                 "head/mask_feature/predictor/norm/beta"):
        assert want in names, (want, sorted(n for n in names if "head/" in n)[:20])
    kw = [p for n, p in m.reference_variables(include_scope=False)
          if n == "head/mask_kernel/kernel_subnet0/weights"][0]
    assert tuple(kw.shape) == (3, 3, 258, 512)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape,out,ac", [((2, 7, 9, 4), (3, 5), False), ((1, 13, 21, 258), (25, 42), False),
                                          ((2, 100, 168, 256), (40, 40), False),
                                          ((1, 5, 6, 3), (11, 13), False), ((1, 5, 6, 3), (11, 13), True),
                                          ((1, 64, 80, 100), (256, 320), False)])
def test_resize_bilinear_vs_oracle(dev, shape, out, ac):
    import solo
    from detectron2_tensorflow_amd.layers import ops
    x = np.random.default_rng(1).normal(size=shape).astype(F32)
    got = ops.resize_bilinear(torch.from_numpy(x).to(dev), out, align_corners=ac,
                              half_pixel_centers=not ac).cpu().numpy()
    want = solo.resize_bilinear_tf(x, *out, half_pixel=not ac, align_corners=ac)
    np.testing.assert_array_equal(got, want)


def _random_head(rng, N, grids, K, D, Hm, Wm, cls_mean=-4.5):
    cate = [rng.normal(cls_mean, 1.0, size=(N, s, s, K)).astype(F32) for s in grids]
    kern = [rng.normal(0, 0.1, size=(N, s, s, D)).astype(F32) for s in grids]
    feats = np.maximum(rng.normal(size=(N, Hm, Wm, D)), 0).astype(F32)
    return cate, kern, feats


def _oracle_tail(probs, dbg, strides, grids, Hm, Wm, OH, OW, kernel="gaussian", **kw):
    """The oracle's inference tail on the GPU's probs and mask logits."""
    import solo
    logits = dbg["logits"].cpu().numpy()
    live_row = dbg["live_row"].cpu().numpy()
    offs = dbg["row_off"]

    def cell_logits(n, cells):
        rows = live_row[n][cells]
        assert (rows >= 0).all(), "oracle candidate in a cell the GPU did not keep live"
        return logits[offs[n] + rows]

    st = solo.cell_strides(grids, strides)
    res = []
    for n in range(probs.shape[0]):
        m, c, s, v, info = solo.inference_single_image(probs[n], lambda cells, n=n: cell_logits(n, cells),
                                                       st, kernel=kernel, **kw)
        im, bx = solo.masks_to_image(m, Hm, Wm, OH, OW)
        res.append((im, bx, c, s, v, info))
    return res


# A mask pixel's fate is sigmoid(logit) > 0.5.  Within 4 ulp(1.0) = 2^-21 of
# logit 0 the float sigmoid is 0.5 +- 1 ulp, so an expf one ulp apart (ocml on
# the device, libm / numpy in the oracle) can flip the test; anywhere else the
# two sides must agree.
THRESH_AMBIGUOUS = 4 * 2.0 ** -23


def _unpack_bits(words, P):
    """[k, W64] int64 (bit p % 64 of word p // 64 = pixel p) -> [k, P] bool."""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")
    return b[:, :P].astype(bool)


def _assert_tail_equal(got, want, dbg, score_rtol=1e-5, exact_masks=True, proof=None):
    """score_rtol: the mask-score sums run over Hm x Wm pixels in another
    order than the oracle's (1e-5 at 64x80; 200x336 = 67,200-term sums need 5e-5).
    exact_masks=False (the C5 geometry, 500 masks x 67,200 pixels): instead of
    bounds, a per-mismatch proof (``proof`` = (probs, row logits, Hm, Wm, OH,
    OW, kernel)):
      1. every top-k mask pixel whose GPU bit differs from the oracle's
         sigmoid(logit) > 0.5 has |logit| <= THRESH_AMBIGUOUS (the only
         place two correctly-rounded-to-1-ulp expf can disagree);
      2. the GPU mask sums are its bit counts, and the oracle's differ from
         them by exactly the flipped pixels of the row;
      3. given the GPU's masks, the rest of the tail IS the oracle's: the
         mask scores within the sum-order bar, Matrix NMS decays within
         2 * score_rtol, and the pasted masks bit-exact with boxes within
         max(1e-4, 2 ulp);
      4. rows with no flipped pixel match the oracle's own run exactly as in
         the exact case; classes and valid flags are exact throughout."""
    import oracle
    import solo
    from test_gpu_ops import assert_boxes_close
    masks, boxes, scores, classes, valid = [t.cpu().numpy() for t in got]
    nflip = 0
    for n, (im, bx, c, s, v, info) in enumerate(want):
        k = int(dbg["top_count"][n])
        assert k == len(info["top_scores"])
        np.testing.assert_array_equal(dbg["top_classes"][n, :k].cpu().numpy(), info["top_classes"])
        np.testing.assert_array_equal(valid[n], v)
        np.testing.assert_array_equal(classes[n], c)
        gts = dbg["top_scores"][n, :k].cpu().numpy()
        gsum = dbg["top_sum"][n, :k].cpu().numpy()
        gdec = dbg["decayed"][n, :k].cpu().numpy()
        if exact_masks:
            np.testing.assert_allclose(gts, info["top_scores"], rtol=score_rtol, atol=0)
            np.testing.assert_array_equal(gsum, info["top_sum_masks"])
            np.testing.assert_allclose(gdec, info["decayed"], rtol=2 * score_rtol, atol=1e-7)
            np.testing.assert_allclose(scores[n], s, rtol=2 * score_rtol, atol=0)
            np.testing.assert_array_equal(masks[n], im)
            assert_boxes_close(boxes[n], bx)
            continue
        probs, row_logits, Hm, Wm, OH, OW, kernel = proof
        cells = info["top_cells"]
        L = row_logits(n, cells)                                  # [k, P] GPU logits
        sig = oracle.sigmoid(L)
        obits = sig > np.float32(0.5)
        gbits = _unpack_bits(dbg["mask_bits"][n, :k].cpu().numpy(), Hm * Wm)
        flip = gbits != obits
        # 1. flips only at threshold-ambiguous logits
        assert np.all(np.abs(L[flip]) <= THRESH_AMBIGUOUS), np.abs(L[flip]).max()
        nflip += int(flip.sum())
        # 2. the sums are the bit counts; the oracle's differ by the flips
        np.testing.assert_array_equal(gsum, gbits.sum(1).astype(np.float32))
        np.testing.assert_array_equal(
            info["top_sum_masks"].astype(np.int64) - gsum.astype(np.int64),
            (obits & ~gbits).sum(1) - (gbits & ~obits).sum(1))
        # 3. the tail on the GPU's masks is the oracle's
        gm = gbits.astype(np.float32)
        mscore = ((sig * gm).sum(axis=1, dtype=np.float32) / gsum).astype(np.float32)
        cate = probs[n][cells, info["top_classes"]]
        np.testing.assert_allclose(gts, (cate * mscore).astype(np.float32), rtol=score_rtol, atol=0)
        dec = oracle.matrix_nms(gm, info["top_classes"], gts, gsum, kernel, 2.0)
        np.testing.assert_allclose(gdec, dec, rtol=2 * score_rtol, atol=1e-7)
        keep = np.nonzero(gdec > np.float32(0.05))[0][:valid.shape[1]]
        np.testing.assert_array_equal(keep.size, int(valid[n].sum()))
        pim, pbx = solo.masks_to_image(gm[keep], Hm, Wm, OH, OW)
        m = keep.size
        np.testing.assert_array_equal(masks[n][:m], pim)
        assert not masks[n][m:].any()
        assert_boxes_close(boxes[n][:m], pbx)
        # 4. unflipped rows: the oracle's own run, exactly as the exact case
        clean = ~flip.any(axis=1)
        np.testing.assert_allclose(gts[clean], info["top_scores"][clean], rtol=score_rtol, atol=0)
        np.testing.assert_array_equal(gsum[clean], info["top_sum_masks"][clean])
    return nflip


@pytest.fixture(params=[2, 0], ids=["mfma_lut", "popcount"])
def solo_mfma(request):
    """The Matrix-NMS intersections on the int8 MFMA (tuning "solo_mfma" 2:
    bits expanded by an LDS table, the default) or the AND + popcount tiles
    (0)."""
    from detectron2_tensorflow_amd.layers import ops
    old = ops.get_tuning("solo_mfma")
    ops.set_tuning("solo_mfma", request.param)
    yield request.param
    ops.set_tuning("solo_mfma", old)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["gaussian", "linear"])
def test_solo_tail_vs_oracle(dev, kernel, solo_mfma):
    """ops.solo_inference on random head outputs (2 images, the C5 grids
    40/36/24/16/12, K = 80, D = 256, masks 64x80 -> 256x320)."""
    import solo
    from detectron2_tensorflow_amd.layers import ops
    rng = np.random.default_rng(3)
    grids, K, D, Hm, Wm = [40, 36, 24, 16, 12], 80, 256, 64, 80
    strides = [8.0, 8.0, 16.0, 32.0, 32.0]
    cate, kern, feats = _random_head(rng, 2, grids, K, D, Hm, Wm)
    dbg = {}
    got = ops.solo_inference([torch.from_numpy(c).to(dev) for c in cate],
                             [torch.from_numpy(k).to(dev) for k in kern],
                             torch.from_numpy(feats).to(dev), strides, (256, 320),
                             nms_kernel=kernel, debug=dbg)
    # 1. sigmoid + point NMS: expf differs by an ulp (a few ulps of the sigmoid)
    import oracle
    want_p = np.concatenate([solo.point_nms(oracle.sigmoid(c)).reshape(2, -1, K) for c in cate], 1)
    gp = dbg["probs"].cpu().numpy()
    np.testing.assert_allclose(gp, want_p, rtol=1e-6, atol=0)
    assert ((gp > 0) == (want_p > 0)).all()
    # 2. dynamic conv logits vs float64 (split-bf16 products, f32 accumulate)
    kall = np.concatenate([k.reshape(2, -1, D) for k in kern], 1)
    for n in range(2):
        cells = dbg["live_cells"][n, :dbg["counts"][n]].cpu().numpy()
        want_l = kall[n][cells].astype(np.float64) @ feats[n].reshape(-1, D).astype(np.float64).T
        gl = dbg["logits"][dbg["row_off"][n]:dbg["row_off"][n] + len(cells)].cpu().numpy()
        assert np.abs(gl - want_l).max() <= 1e-4 * max(1.0, np.abs(want_l).max())
    # 3. the tail on identical probs / logits: bit-exact decisions
    want = _oracle_tail(gp, dbg, strides, grids, Hm, Wm, 256, 320, kernel=kernel)
    assert all(w[5]["num_candidates"] > 500 for w in want)  # the top-k(500) is exercised
    _assert_tail_equal(got, want, dbg)
    # 4. Matrix NMS's finite decays only (a linear kernel divides by 1 - comp)
    for n in range(2):
        d = dbg["decayed"][n].cpu().numpy()
        assert np.isfinite(d[:int(dbg["top_count"][n])]).all() or kernel == "linear"


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["gaussian", "linear"])
def test_solo_tail_vs_oracle_c5_geometry(dev, kernel, solo_mfma):
    """The tail at the C5 geometry (SOLOv2 R50-FPN at 1333x800 padded to
    800x1344): mask features 200x336 (67,200 pixels), D = 256, the five grids,
    more than 500 candidates per image (the top-k(500) and a 500 x 500 Matrix
    NMS), masks pasted onto 800x1344 — vs oracle/solo.py on the GPU's own
    probs / logits, every decision bit-exact; finite decays apart from the
    linear kernel's +inf columns."""
    from detectron2_tensorflow_amd.layers import ops
    rng = np.random.default_rng(33)
    grids, K, D, Hm, Wm = [40, 36, 24, 16, 12], 80, 256, 200, 336
    strides = [8.0, 8.0, 16.0, 32.0, 32.0]
    cate, kern, feats = _random_head(rng, 2, grids, K, D, Hm, Wm)
    dbg = {}
    got = ops.solo_inference([torch.from_numpy(c).to(dev) for c in cate],
                             [torch.from_numpy(k).to(dev) for k in kern],
                             torch.from_numpy(feats).to(dev), strides, (800, 1344),
                             nms_kernel=kernel, debug=dbg)
    probs = dbg["probs"].cpu().numpy()
    want = _oracle_tail(probs, dbg, strides, grids, Hm, Wm, 800, 1344, kernel=kernel)
    assert all(w[5]["num_candidates"] > 500 for w in want)
    assert all(len(w[5]["top_scores"]) == 500 for w in want)
    assert got[0].shape == (2, 100, 800, 1344)
    logits = dbg["logits"].cpu().numpy()
    live_row = dbg["live_row"].cpu().numpy()
    offs = dbg["row_off"]
    row_logits = lambda n, cells: logits[offs[n] + live_row[n][cells]]  # noqa: E731
    nflip = _assert_tail_equal(got, want, dbg, score_rtol=5e-5, exact_masks=False,
                               proof=(probs.reshape(2, -1, K), row_logits, Hm, Wm, 800, 1344,
                                      kernel))
    print(f"{kernel}: {nflip} threshold-ambiguous mask pixels flipped of {2 * 500 * Hm * Wm}")
    for n in range(2):
        d = dbg["decayed"][n, :500].cpu().numpy()
        fin = np.isfinite(d)
        assert fin.all() or kernel == "linear"
        assert fin.sum() > 250


@pytest.mark.gpu
def test_solo_tail_few_candidates_and_empty(dev, solo_mfma):
    """Fewer candidates than TOPK_CANDIDATES_TEST (top-k of the valid count,
    zero-mask padding rows in Matrix NMS), and an image with none at all."""
    from detectron2_tensorflow_amd.layers import ops
    rng = np.random.default_rng(4)
    grids, K, D, Hm, Wm = [12, 8], 16, 64, 32, 40
    strides = [8.0, 16.0]
    cate, kern, feats = _random_head(rng, 2, grids, K, D, Hm, Wm, cls_mean=-4.0)
    for c in cate:
        c[1] = -20.0  # image 1: no score above 0.1
    dbg = {}
    got = ops.solo_inference([torch.from_numpy(c).to(dev) for c in cate],
                             [torch.from_numpy(k).to(dev) for k in kern],
                             torch.from_numpy(feats).to(dev), strides, (128, 160), debug=dbg)
    assert dbg["counts"][1] == 0 and int(dbg["top_count"][1]) == 0
    want = _oracle_tail(dbg["probs"].cpu().numpy(), dbg, strides, grids, Hm, Wm, 128, 160)
    assert 0 < want[0][5]["num_candidates"] < 500
    _assert_tail_equal(got, want, dbg)
    assert not got[4][1].any() and not got[0][1].any()


def _solo_model(dev, batch):
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import calibrate_solo_head
    torch.manual_seed(0)
    model = build_model(_cfg()).to(dev).eval()
    with torch.no_grad():
        images = model.preprocess_image(batch)
        feats = model.neck(model.backbone(images.tensor))
        cls, ker = model.detector.mask_kernel_branch(feats)
        calibrate_solo_head(model.detector.mask_kernel_branch, cls, ker)
    return model


def _gpu_head(model, batch):
    images = model.preprocess_image(batch)
    feats = model.neck(model.backbone(images.tensor))
    cls, ker = model.detector.mask_kernel_branch(feats)
    mf = model.detector.mask_feature_branch(feats)
    return images, cls, ker, mf


@pytest.mark.gpu
def test_solo_r50_model_vs_cpu_restatement(dev):
    import cpu_pipeline as cp
    rng = np.random.default_rng(6)
    img = rng.uniform(0, 255, (2, 256, 320, 3)).astype(F32)
    batch = {"image": torch.from_numpy(img).to(dev),
             "image_shape": torch.tensor([[256, 320], [240, 300]], device=dev)}
    model = _solo_model(dev, batch)
    with torch.no_grad():
        images, cls, ker, mf = _gpu_head(model, batch)
        out = model(batch)["instances"]
        dbg = {}
        post = model.detector.inference(cls, ker, mf, images.tensor.shape[1:3], debug=dbg)
    # 1. the model's forward == its head + inference
    for k, f in (("boxes", post.boxes), ("scores", post.get_field("scores")),
                 ("classes", post.get_field("pred_classes")), ("is_valid", post.get_field("is_valid")),
                 ("masks", post.get_field("pred_masks"))):
        assert torch.equal(out[k], f), k
    assert out["masks"].shape == (2, 100, 256, 320) and out["masks"].dtype == torch.uint8
    # 2. head outputs vs the CPU restatement (backbone, FPN, grid resizes,
    #    GN towers, mask feature branch)
    ref = cp.CPUSOLOv2(model)
    with torch.no_grad():
        feats = ref.features(img)
        wcls, wker = ref.kernel_branch(feats)
        wmf = ref.feature_branch(feats)
    for g_, w_ in zip(list(cls) + list(ker) + [mf], list(wcls) + list(wker) + [wmf]):
        err = (g_.cpu() - w_).abs().max().item()
        assert err <= 1e-3 * max(w_.abs().max().item(), 1.0), err
    # 3. the tail on the GPU's own probs / logits: bit-exact decisions
    b = model.detector.mask_kernel_branch
    want = _oracle_tail(dbg["probs"].cpu().numpy(), dbg, b.strides, b.num_grids, mf.shape[1],
                        mf.shape[2], 256, 320)
    _assert_tail_equal([out["masks"], out["boxes"], out["scores"], out["classes"], out["is_valid"]],
                       want, dbg)
    # 4. end to end vs the whole CPU restatement: classes match on >= 90 % of
    #    the kept detections, masks agree on >= 99 % of pixels
    with torch.no_grad():
        w = ref(img)
    g = {k: v.cpu().numpy() for k, v in out.items()}
    for n in range(2):
        wv, gv = w["is_valid"][n], g["is_valid"][n]
        m = int(min(wv.sum(), gv.sum()))
        assert m > 0
        assert (w["classes"][n][:m] == g["classes"][n][:m]).mean() >= 0.9
        assert (w["masks"][n][:m] == g["masks"][n][:m]).mean() >= 0.99


@pytest.mark.gpu
def test_solo_r50_1333x800_geometry(dev):
    """C5 geometry: 800x1333 padded to 800x1344; mask features 200x336
    (67,200 pixels); determinism across two forwards; padded layout."""
    g = torch.Generator(device="cpu").manual_seed(11)
    img = torch.rand(2, 800, 1333, 3, generator=g) * 255
    batch = {"image": img.to(dev), "image_shape": torch.tensor([[800, 1333], [800, 1333]], device=dev)}
    model = _solo_model(dev, batch)
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            images, cls, ker, mf = _gpu_head(model, batch)
            a = model(batch)["instances"]
            b = model(batch)["instances"]
    finally:
        torch.backends.cudnn.deterministic = old
    assert tuple(mf.shape) == (2, 200, 336, 256)
    assert [tuple(c.shape[1:3]) for c in cls] == [(40, 40), (36, 36), (24, 24), (16, 16), (12, 12)]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["masks"].shape == (2, 100, 800, 1344)
    v = a["is_valid"].cpu().numpy()
    for n in range(2):
        m = int(v[n].sum())
        assert m > 0 and v[n][:m].all() and not v[n][m:].any()
        assert (a["scores"][n][m:] == 0).all() and (a["scores"][n][:m] > 0.05).all()
        assert not a["masks"][n][m:].any()
        bx = a["boxes"][n][:m]
        assert (bx[:, 0] <= bx[:, 2]).all() and (bx[:, 1] <= bx[:, 3]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
def test_group_norm_levels_equals_per_level(dev, relu):
    """d2mi_group_norm_nhwc_levels (one set of launches over the SOLOv2 grid
    levels) is bit-identical to d2mi_group_norm_nhwc per level."""
    from detectron2_tensorflow_amd.layers import ops
    rng = np.random.default_rng(7)
    C, G = 256, 32
    xs = [torch.from_numpy((rng.normal(size=(2, S, S, C)) * 2 + 0.5).astype(F32)).to(dev)
          for S in (40, 36, 24, 16, 12)]
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, size=C).astype(F32)).to(dev)
    beta = torch.from_numpy(rng.normal(size=C).astype(F32)).to(dev)
    got = ops.group_norm_levels(xs, G, gamma, beta, 1e-5, relu)
    for x, y in zip(xs, got):
        assert torch.equal(y, ops.group_norm(x, G, gamma, beta, 1e-5, relu))


@pytest.mark.gpu
@pytest.mark.parametrize("C,G,relu,up2,acc", [(128, 32, True, False, False), (512, 32, True, False, False),
                                              (128, 32, True, True, True), (256, 32, False, True, False),
                                              (128, 32, True, False, True)])
def test_group_norm_hip_vs_float64(dev, C, G, relu, up2, acc):
    """d2mi_group_norm_nhwc vs the GroupNorm.call formula in float64
    (normalization.py:235-260: moments over H, W and the group's channels,
    x * inv + (beta - mean * inv)), with the fused ReLU / nearest-x2 / sum."""
    from detectron2_tensorflow_amd.layers import ops
    rng = np.random.default_rng(C + G)
    N, H, W = 2, 25, 42
    x = (rng.normal(size=(N, H, W, C)) * 3 + 1).astype(F32)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(F32)
    beta = rng.normal(size=C).astype(F32)
    xr = x.astype(np.float64).reshape(N, H, W, G, C // G)
    mu = xr.mean(axis=(1, 2, 4), keepdims=True)
    var = ((xr - mu) ** 2).mean(axis=(1, 2, 4), keepdims=True)
    inv = 1 / np.sqrt(var + 1e-5) * gamma.reshape(1, 1, 1, G, C // G)
    want = (xr * inv + (beta.reshape(1, 1, 1, G, C // G) - mu * inv)).reshape(N, H, W, C)
    if relu:
        want = np.maximum(want, 0)
    if up2:
        want = want.repeat(2, 1).repeat(2, 2)
    base = rng.normal(size=want.shape).astype(F32) if acc else None
    if acc:
        want = want + base
    out = ops.group_norm(torch.from_numpy(x).to(dev), G, torch.from_numpy(gamma).to(dev),
                         torch.from_numpy(beta).to(dev), 1e-5, relu, up2,
                         torch.from_numpy(base).to(dev) if acc else None)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=2e-5, atol=2e-5)


@pytest.mark.gpu
def test_solo_training_steps(dev):
    """SOLOv2 R50-FPN training through the Trainer at 256x320
    (solo_v2.py:274-474: dice + focal losses, get_ground_truth): the losses
    of the first step equal the oracle's on the model's own head outputs,
    every trainable parameter gets a finite gradient, and over-fitting one
    batch lowers the loss."""
    import training as otrain
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg = _cfg()
    cfg.defrost()
    cfg.SOLVER.BASE_LR = 0.005
    cfg.SOLVER.WARMUP_ITERS = 0
    cfg.freeze()
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 5, dev, num_classes=80, sqrt_area=(24.0, 200.0),
                                  full_mask_hw=(256, 320))
    head = model.detector
    got = {}
    orig = head.mask_kernel_branch.losses

    def spy(pc, pk, mf, tg):
        got["args"] = ([t.detach().cpu().numpy() for t in pc], [t.detach().cpu().numpy() for t in pk],
                       mf.detach().cpu().numpy())
        return orig(pc, pk, mf, tg)
    head.mask_kernel_branch.losses = spy
    try:
        losses = model(batch)
    finally:
        del head.mask_kernel_branch.losses
    assert set(losses) == {"loss_ins", "loss_cls"}
    sum(losses.values()).backward()
    bad = [n for n, p in model.named_parameters()
           if p.requires_grad and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad[:5]
    inst = {k: v.cpu().numpy() for k, v in batch["instances"].items()}
    pc, pk, mf = got["args"]
    b = head.mask_kernel_branch
    tg = otrain.solov2_targets(inst["gt_boxes"], inst["gt_classes"], inst["is_valid"],
                               inst["gt_masks"], mf.shape[1:3], b.num_grids, b.scale_ranges,
                               b.sigma)
    assert sum(len(p) for _, p, _ in tg) > 5
    ins, cls = otrain.solov2_losses(pc, pk, mf, tg, b.num_classes, b.focal_loss_alpha,
                                    b.focal_loss_gamma, b.ins_loss_weight)
    assert float(losses["loss_ins"].detach()) == pytest.approx(ins, rel=1e-4)
    assert float(losses["loss_cls"].detach()) == pytest.approx(cls, rel=1e-4)
    model.zero_grad(set_to_none=True)
    tr = Trainer(cfg, model)
    hist = [float(tr.step(batch)["total_loss"]) for _ in range(10)]
    assert all(np.isfinite(hist)), hist
    # (measured: 3.32 -> 2.83 over the ten steps, falling at every step)
    assert np.mean(hist[-3:]) < 0.95 * np.mean(hist[:3]), hist
    assert (np.diff(hist) < 0).sum() >= 7, hist
    _C.raise_on_errors(dev)
