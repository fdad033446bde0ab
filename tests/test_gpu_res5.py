"""The C4 head on the GPU: the fused pool / gather kernels against float64,
Res5ROIHeads training and inference against the float64 restatement of the
reference (tests/res5_reference.py), the stride elision against the literal
path, and the settings that must take the literal path."""
import os

import numpy as np
import pytest
import torch

import res5_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
U = 2.0 ** -24  # float32 unit roundoff

# (R, P, C, M): dst = -1 rows mixed in and dst not monotone; the smallest shape;
# C below a wave's 16-byte span with no destination rows; a null dst; all rows taken
SHAPES = [(5, 49, 2048, 3), (1, 1, 4, 1), (7, 49, 12, 0), (64, 49, 2048, None), (33, 9, 516, 33)]


def _case(R, P, C, M, seed=0):
    g = torch.Generator().manual_seed(seed + R * 1000 + C)
    x = torch.randn(R, P, C, generator=g)
    dst = None
    if M is not None:
        dst = torch.full((R,), -1, dtype=torch.int32)
        rows = torch.randperm(R, generator=g)[:M]
        dst[rows] = torch.randperm(M, generator=g).to(torch.int32)  # (not monotone)
    gp = torch.randn(R, C, generator=g)
    gy = torch.randn(M, P, C, generator=g) if M else None
    return x, dst, gp, gy


def _ulp(v):
    """float32 spacing at the magnitude of float64 v (at least the smallest normal's)."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 23)


def _fwd(lib, _C, x, dst, M, dev):
    R, P, C = x.shape
    pooled = torch.full((R, C), float("nan"), device=dev)
    y = torch.full((M or 0, P, C), float("nan"), device=dev)
    rc = lib.d2mi_res5_pool_fwd(_C.ptr(x), R, P, C, _C.ptr(dst), M or 0, _C.ptr(pooled),
                                _C.ptr(y) if M else None, _C.stream_of(dev))
    _C.check(rc, "d2mi_res5_pool_fwd")
    return pooled, y


def _bwd(lib, _C, gp, gy, dst, shape, M, dev):
    R, P, C = shape
    dx = torch.full(shape, float("nan"), device=dev)  # every element must be written
    rc = lib.d2mi_res5_pool_bwd(_C.ptr(gp), _C.ptr(gy), _C.ptr(dst), R, P, C, M or 0, _C.ptr(dx),
                                _C.stream_of(dev))
    _C.check(rc, "d2mi_res5_pool_bwd")
    return dx


@pytest.mark.parametrize("R,P,C,M", SHAPES)
def test_pool_kernels_against_float64(dev, R, P, C, M):
    """Y bit-equal to the gathered rows; pooled within P * 2^-24 * mean_p |x| of
    float64 (the bound of a sequential f32 sum of P terms and one division);
    dX fully written (NaN pre-fill), bit-equal to the IEEE float32 evaluation
    of dpooled / P + dY (one division, one add, numpy) and within 2 ulp of
    float64.  The ulp is float32's at the element's own magnitude wherever
    dX is one term (rows without a destination) or two terms of one sign; where
    the terms cancel no float32 evaluation can be that close to float64 at
    the difference's magnitude, and the ulp is the larger term's.  Two runs
    are bitwise equal."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    x, dst, gp, gy = _case(R, P, C, M)
    xd, gpd = x.to(dev), gp.to(dev)
    dstd = dst.to(dev) if dst is not None else None
    gyd = gy.to(dev) if gy is not None else None
    _C.clear_errors(dev)
    pooled, y = _fwd(lib, _C, xd, dstd, M, dev)
    pooled2, y2 = _fwd(lib, _C, xd, dstd, M, dev)
    want_p, want_y = ref.pool_gather(x, dst, M or 0)
    assert torch.equal(pooled, pooled2) and torch.equal(y.cpu(), y2.cpu())
    if M:
        assert torch.equal(y.cpu().to(F64), want_y)
    bound = P * U * x.to(F64).abs().mean(1)
    err = (pooled.cpu().to(F64) - want_p).abs()
    print(f"pooled: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())

    dx = _bwd(lib, _C, gpd, gyd, dstd, (R, P, C), M, dev)
    dx2 = _bwd(lib, _C, gpd, gyd, dstd, (R, P, C), M, dev)
    assert torch.equal(dx, dx2) and not torch.isnan(dx).any()
    a32 = (gp.numpy() / np.float32(P))[:, None, :]
    b32 = np.zeros((R, P, C), np.float32)
    a64 = (gp.to(F64) / P)[:, None, :].expand(R, P, C)
    b64 = torch.zeros(R, P, C, dtype=F64)
    if M:
        taken = torch.nonzero(dst >= 0)[:, 0]
        b32[taken.numpy()] = gy.numpy()[dst[taken].long().numpy()]
        b64[taken] = gy.to(F64)[dst[taken].long()]
    got = dx.cpu()
    assert np.array_equal(got.numpy(), (a32 + b32).astype(np.float32))
    want = a64 + b64
    err = (got.to(F64) - want).abs()
    one_sign = (a64 * b64) >= 0
    scale = torch.where(one_sign, want.abs(), torch.maximum(a64.abs(), b64.abs()))
    ulps = err / _ulp(scale)
    print(f"dX: max ulps {float(ulps.max()):.3f} ({int(one_sign.sum())} of {want.numel()} "
          "elements at their own magnitude)")
    assert bool((ulps <= 2.0).all())
    assert _C.error_word(dev)[0] == 0


@pytest.mark.parametrize("R,P,C,M", SHAPES)
def test_autograd_through_the_fused_op_against_the_tensor_arm(dev, R, P, C, M):
    from detectron2_tensorflow_amd.layers import ops
    x, dst, gp, gy = _case(R, P, C, M, seed=1)
    dstd = dst.to(dev) if dst is not None else None
    outs = []
    for fn in (ops.res5_pool, ops.res5_pool_dense):
        xd = x.to(dev).requires_grad_(True)
        pooled, y = fn(xd, dstd, M or 0)
        loss = (pooled * gp.to(dev)).sum()
        if M:
            loss = loss + (y * gy.to(dev)).sum()
        loss.backward()
        outs.append((pooled.detach(), y.detach() if y is not None else None, xd.grad))
    (p0, y0, g0), (p1, y1, g1) = outs
    assert (y0 is None) == (y1 is None) == (dst is None)
    if y0 is not None:
        assert torch.equal(y0, y1)
    torch.testing.assert_close(p0, p1, rtol=0, atol=float(P * U * x.abs().mean(1).max()) * 2)
    # (the tensor arm adds dY into the broadcast: the same two f32 operations)
    torch.testing.assert_close(g0, g1, rtol=2.0 ** -22, atol=1e-7)


# ------------------------------------------------------------------ head level
def _gpu_train(head, feat, proposals, targets, shapes, dev):
    head.train()
    f = feat.detach().clone().to(dev).requires_grad_(True)
    for p in head.parameters():
        p.grad = None
    sampled, losses = head(ref.Images(shapes.to(dev)), {"res4": f}, ref.to_device(proposals, dev),
                           ref.to_device(targets, dev))
    sum(losses.values()).backward()
    grads = {n: p.grad.detach().cpu() for n, p in head.named_parameters() if p.grad is not None}
    return ({k: v.cpu() for k, v in sampled.items()}, {k: float(v.detach()) for k, v in losses.items()},
            f.grad.cpu(), grads)


def _reference_train(head_cpu, feat, sampled, targets):
    for p in head_cpu.parameters():
        p.grad = None
    f64 = feat.detach().to(F64).requires_grad_(True)
    want, pooled_in = ref.train_losses(head_cpu, f64, sampled, targets)
    sum(want.values()).backward()
    grads = {n: p.grad.detach().to(F64) for n, p in head_cpu.named_parameters()
             if p.grad is not None}
    return {k: float(v.detach()) for k, v in want.items()}, f64.grad, grads, pooled_in.detach()


def _close(got, want, what):
    """|got - want| <= 1e-4, the bound scaled by the reference's max-abs where
    that exceeds 1 (a gradient that is not O(1): sums over hundreds of rows)."""
    want = want.to(F64)
    tol = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got.to(F64) - want).abs().max())
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("fused", [True, False])
def test_head_training_against_the_float64_reference(dev, fused):
    from detectron2_tensorflow_amd.layers import ops
    _, head = ref.narrow_head(ROOT)
    feat, proposals, targets, shapes = ref.make_case()
    old = ops.res5.FUSED_POOL
    ops.res5.FUSED_POOL = fused
    try:
        sampled, losses, gfeat, grads = _gpu_train(head.to(dev), feat, proposals, targets, shapes, dev)
    finally:
        ops.res5.FUSED_POOL = old
    assert sampled["is_valid"].sum(1).tolist() == [12, 12] and head.last_mask_rows == 8
    want, wfeat, wgrads, _ = _reference_train(head.cpu(), feat, sampled, targets)
    assert set(losses) == set(want) == {"loss_cls", "loss_box_reg", "loss_mask"}
    for k in want:
        print(k, losses[k], want[k])
        assert abs(losses[k] - want[k]) <= 1e-4, (k, losses[k], want[k])
    _close(gfeat, wfeat, "feature map")
    assert set(grads) == set(wgrads)
    assert {n.split(".")[0] for n in grads} == {"res5", "box_predictor", "mask_head"}
    for n in wgrads:
        assert float(wgrads[n].abs().max()) > 0, n
        _close(grads[n], wgrads[n], n)


def _detect(head, feat, proposals, shapes, dev):
    head.eval()
    with torch.no_grad():
        res, _ = head(ref.Images(shapes.to(dev)), {"res4": feat.to(dev)},
                      ref.to_device(proposals, dev), None)
    return {"boxes": res.boxes.cpu(), "scores": res.get_field("scores").cpu(),
            "classes": res.get_field("pred_classes").cpu(),
            "valid": res.get_field("is_valid").cpu().bool(),
            "masks": res.get_field("pred_masks").cpu()}


def test_head_inference_against_the_float64_reference(dev):
    """Each valid detection is one (proposal, class) pair of the float64
    restatement: its box within 1e-4 px of that pair's decoded, clipped box
    and its score within 1e-4 of the pair's softmax score; its mask within
    1e-4 of the float64 mask head on the detection's own box.  Classes,
    validity and kept counts are those of the tensor arm exactly."""
    from detectron2_tensorflow_amd.layers import ops
    from detectron2_tensorflow_amd.structures import BoxList
    _, head = ref.narrow_head(ROOT, ["TEST.DETECTIONS_PER_IMAGE", 20])
    feat, _, _, shapes = ref.make_case()
    g = torch.Generator().manual_seed(5)
    N, P = 2, 48
    y, x = torch.rand(N, P, generator=g) * 50 + 2, torch.rand(N, P, generator=g) * 70 + 2
    hw = torch.rand(N, P, 2, generator=g) * 35 + 8
    props = torch.stack([y, x, y + hw[..., 0], x + hw[..., 1]], -1)
    pvalid = torch.rand(N, P, generator=g) < 0.9
    proposals = BoxList(props)
    proposals.add_field("is_valid", pvalid)
    head.to(dev)
    got = _detect(head, feat, proposals, shapes, dev)
    old = ops.res5.FUSED_POOL
    ops.res5.FUSED_POOL = False
    try:
        arm = _detect(head, feat, proposals, shapes, dev)
    finally:
        ops.res5.FUSED_POOL = old
    assert torch.equal(got["classes"], arm["classes"]) and torch.equal(got["valid"], arm["valid"])
    assert got["valid"].sum(1).tolist() == arm["valid"].sum(1).tolist()
    assert int(got["valid"].sum()) >= 10
    head.cpu()
    f64 = feat.to(F64)
    rows = torch.nonzero(pvalid.reshape(-1))[:, 0]
    img = torch.arange(N).repeat_interleave(P)[rows]
    pb = props.reshape(-1, 4).to(F64)[rows]
    with torch.no_grad():
        _, bf = ref.box_features(head, f64, pb, img)
        pooled = bf.mean((1, 2))
        prob = torch.softmax(ref.linear(pooled, head.box_predictor.cls_score), 1)
        deltas = ref.linear(pooled, head.box_predictor.bbox_pred).reshape(len(rows), -1, 4)
        for n in range(N):
            for d in torch.nonzero(got["valid"][n])[:, 0].tolist():
                c = int(got["classes"][n, d])
                cand = torch.nonzero(img == n)[:, 0]
                dec = ref.apply_deltas(deltas[cand, c if deltas.shape[1] > 1 else 0], pb[cand],
                                       head.box2box_transform.weights)
                h, w = shapes[n].tolist()
                dec = torch.stack([dec[:, 0].clamp(0, h), dec[:, 1].clamp(0, w),
                                   dec[:, 2].clamp(0, h), dec[:, 3].clamp(0, w)], 1)
                dist = (dec - got["boxes"][n, d].to(F64)).abs().amax(1)
                r = int(dist.argmin())
                assert float(dist[r]) <= 1e-4, (n, d, float(dist[r]))
                assert abs(float(prob[cand[r], c]) - float(got["scores"][n, d])) <= 1e-4, (n, d)
        db = got["boxes"].reshape(-1, 4).to(F64)
        D = got["boxes"].shape[1]
        _, mf = ref.box_features(head, f64, db, torch.arange(N).repeat_interleave(D))
        ml = ref.mask_head(head.mask_head, mf)
        want = torch.sigmoid(ml[torch.arange(N * D), :, :, got["classes"].reshape(-1).clamp(min=0)])
    v = got["valid"].reshape(-1)
    masks = got["masks"].reshape(N * D, *got["masks"].shape[2:])
    assert float((masks[v].to(F64) - want[v]).abs().max()) <= 1e-4
    assert float(masks[~v].abs().max() if (~v).any() else 0.0) == 0.0
    assert float((got["masks"] - arm["masks"]).abs().max()) <= 1e-4


@pytest.mark.parametrize("pooler", ["ROIAlignV2", "ROIAlign"])
def test_elision_on_against_off(dev, pooler):
    """Both arms within 1e-4 of the float64 restatement of the LITERAL
    formulation (the full 2n x 2n crop, block_1 at stride 2): the pooled res5
    input (the elided arm's n x n crop against the full crop's even grid), the
    losses and the feature-map gradient.  The boxes -- one of them reaching
    40 px past the image's top-left corner, so that out-of-range samples take
    part -- are constructed so that no sample coordinate of either arm lies
    within 1e-3 px of the padded map's borders 0 and H + 1 / W + 1, where the
    in-range test could flip between the arms; asserted from the float64
    coordinates, for the un-padded map's borders 0 and H - 1 / W - 1 as well."""
    _, head = ref.narrow_head(ROOT, ["MODEL.ROI_BOX_HEAD.POOLER_TYPE", pooler])
    feat, proposals, targets, shapes = ref.make_case(outside=True)
    Hf, Wf = feat.shape[1:3]
    results = {}
    for elide in (True, False):
        head.ELIDE_STRIDE = elide
        assert head.elides() == elide
        head.to(dev)
        sampled, losses, gfeat, _ = _gpu_train(head, feat, proposals, targets, shapes, dev)
        with torch.no_grad():
            b = sampled["boxes"].reshape(-1, 4).to(dev)
            n_img = torch.arange(2, dtype=torch.int32, device=dev).repeat_interleave(16)
            pooled_in, stride = head._pool([feat.to(dev)], b, n_img)
        assert stride == (1 if elide else None)
        assert pooled_in.shape[1:3] == ((7, 7) if elide else (14, 14))
        results[elide] = (sampled, losses, gfeat, pooled_in.cpu())
        head.cpu()
    sampled = results[True][0]
    assert all(torch.equal(sampled[k], results[False][0][k]) for k in sampled)
    # the border condition, from the CPU-computed float64 coordinates of both arms
    p = head.pooler
    boxes = sampled["boxes"].reshape(-1, 4)[sampled["is_valid"].reshape(-1)].to(F64)
    arms = [ref.sample_coords(boxes, (Hf, Wf), 14, p.scales[0], 0, p.aligned),
            ref.sample_coords(head._even_grid_boxes(boxes), (Hf, Wf), 7, p.scales[0], 0, p.aligned)]
    outside = 0
    for ys, xs in arms:
        for c, size in ((ys, Hf), (xs, Wf)):
            for border in (0.0, size + 1.0, 1.0, float(size)):  # padded map; un-padded map (+1)
                assert float((c - border).abs().min()) >= 1e-3, (pooler, border)
            outside += int(((c < 0) | (c > size + 1)).sum())
    assert outside > 0  # (the out-of-range branch takes part)
    want, wfeat, _, want_in = _reference_train(head, feat, sampled, targets)
    valid = sampled["is_valid"].reshape(-1)
    for elide, (_, losses, gfeat, pooled_in) in results.items():
        got_in = pooled_in[valid].to(F64)
        lit = want_in[:, ::2, ::2] if elide else want_in
        err = float((got_in - lit).abs().max())
        print(pooler, "elide" if elide else "literal", "pooled input err", err, losses, want)
        assert err <= 1e-4
        for k in want:
            assert abs(losses[k] - want[k]) <= 1e-4, (elide, k, losses[k], want[k])
        _close(gfeat, wfeat, f"feature map, elide={elide}")


@pytest.mark.parametrize("extra", [["MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2],
                                   ["MODEL.RESNETS.STRIDE_IN_1X1", False]],
                         ids=["sampling_ratio_2", "stride_in_3x3"])
def test_literal_path_settings(dev, extra):
    _, head = ref.narrow_head(ROOT, extra)
    assert head.ELIDE_STRIDE and not head.elides()
    feat, proposals, targets, shapes = ref.make_case()
    head.to(dev)
    sampled, losses, gfeat, _ = _gpu_train(head, feat, proposals, targets, shapes, dev)
    with torch.no_grad():
        x, stride = head._pool([feat.to(dev)], sampled["boxes"].reshape(-1, 4).to(dev),
                               torch.arange(2, dtype=torch.int32, device=dev).repeat_interleave(16))
    assert stride is None and x.shape[1:3] == (14, 14)
    want, wfeat, _, want_in = _reference_train(head.cpu(), feat, sampled, targets)
    assert float((x.cpu()[sampled["is_valid"].reshape(-1)].to(F64) - want_in).abs().max()) <= 1e-4
    for k in want:
        assert abs(losses[k] - want[k]) <= 1e-4, (k, losses[k], want[k])
    _close(gfeat, wfeat, "feature map")


def test_c4_model_trains_a_step_eagerly_and_infers(dev):
    """mask_rcnn_R_50_C4_1x end to end at 192 x 256: one Trainer step (finite
    losses, a gradient-fed update of the head) and one inference.  With one
    anchor size instead of the config's 5: the single-level RPN's 5 sizes x 3
    ratios are 15 anchors per cell, and the RPN kernels take at most 12
    (d2mi_grid_anchors, csrc/detect.h kMaxA) and, in the backward, 16 head
    outputs per cell = 3 anchors (d2mi_wgrad_skinny_levels) -- limits of the
    RPN kernels, not of the head."""
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import Res5ROIHeads, build_model
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/COCO-InstanceSegmentation/mask_rcnn_R_50_C4_1x.yaml"))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[128]]
    finalize(cfg, True, 1, ref.CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    assert type(model.roi_heads) is Res5ROIHeads and model.roi_heads.elides()
    batch = synthetic_train_batch(2, 192, 256, 0, dev)
    w = model.roi_heads.res5.blocks[2].conv3.weights
    before = w.detach().clone()
    losses = {k: float(v.detach()) for k, v in Trainer(cfg, model).step(batch).items()}
    _C.raise_on_errors(dev)
    print(losses)
    # (Trainer.step adds the sum of the model's five terms as total_loss)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc",
                           "total_loss"}
    assert all(np.isfinite(v) and v >= 0 for v in losses.values())
    assert not torch.equal(w.detach(), before)
    model.eval()
    with torch.no_grad():
        out = model.inference({"image": batch["image"], "image_shape": batch["image_shape"]})
    inst = out["instances"]
    D = cfg.TEST.DETECTIONS_PER_IMAGE
    assert inst["boxes"].shape == (2, D, 4) and inst["masks"].shape == (2, D, 14, 14)
    assert torch.isfinite(inst["boxes"]).all() and torch.isfinite(inst["masks"]).all()
    _C.raise_on_errors(dev)
