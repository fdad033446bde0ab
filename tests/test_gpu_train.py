"""GPU tests of the training path: the mask loss (HIP crop_and_resize targets)
against the oracle, the RPN loss on device against the per-image restatement,
and whole Mask R-CNN R50-FPN training steps (losses finite, every trainable
parameter receives a gradient, the loss falls when over-fitting one batch)."""
import os

import numpy as np
import pytest
import torch

import training as otrain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}


def _cfg(training, **solver):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-InstanceSegmentation",
                                     "mask_rcnn_R_50_FPN_1x.yaml"))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    for k, v in solver.items():
        setattr(cfg.SOLVER, k, v)
    finalize(cfg, training, 1, CATS)
    return cfg


def test_mask_rcnn_loss_matches_oracle(dev):
    from detectron2_tensorflow_amd.modeling.roi_heads.mask_head import mask_rcnn_loss
    rng = np.random.default_rng(0)
    B, G, K = 40, 6, 80
    gt = np.stack([rng.uniform(0, 100, G), rng.uniform(0, 100, G),
                   rng.uniform(120, 300, G), rng.uniform(120, 300, G)], 1).astype(np.float32)
    masks = (rng.random((G, 56, 56)) < 0.5).astype(np.uint8)
    gi = rng.integers(0, G, B)
    boxes = (gt[gi] + rng.normal(0, 15, (B, 4))).astype(np.float32)
    cls = rng.integers(0, K, B)
    fg = rng.random(B) < 0.7
    logits = rng.standard_normal((B, 28, 28, K)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = mask_rcnn_loss(t(logits), t(boxes), t(gt[gi]), t(cls), t(masks), t(gi), t(fg), True)
    want = otrain.mask_rcnn_loss(logits[fg], boxes[fg], gt[gi][fg], cls[fg], masks[gi][fg])
    assert got.item() == pytest.approx(want, rel=1e-5)


def test_rpn_losses_on_device_match_oracle(dev):
    """Same as the CPU test, but with the anchors from the HIP grid kernel and
    all the matching / loss glue on the GPU."""
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import RPN
    from detectron2_tensorflow_amd.structures import ImageList
    import oracle
    cfg = _cfg(False)
    cfg.defrost()
    cfg.MODEL.RPN.IN_FEATURES = ["p3"]
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[32, 64]]
    cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.5, 1.0]]
    rpn = RPN(cfg, {"p3": ShapeSpec(channels=8, stride=8)}).to(dev)
    rng = np.random.default_rng(3)
    N, H, W, G = 2, 6, 7, 4
    anchors = oracle.grid_anchors(H, W, 8, oracle.generate_cell_anchors([32, 64], [0.5, 1.0]))
    A = anchors.shape[0] // (H * W)
    feats = [torch.zeros(N, H, W, 8, device=dev)]
    np.testing.assert_array_equal(rpn._all_anchors(feats).cpu().numpy(), anchors)
    cy, cx = rng.uniform(0, 48, N * G), rng.uniform(0, 56, N * G)
    h, w = rng.uniform(16, 60, N * G), rng.uniform(16, 60, N * G)
    gt = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(np.float32)
    gt = gt.reshape(N, G, 4)
    valid = np.array([[1, 1, 1, 0], [1, 0, 1, 1]], bool)
    crowd = np.array([[0, 0, 1, 0], [0, 0, 0, 0]], bool)
    lg = rng.standard_normal((N, H, W, A)).astype(np.float32)
    dl = (rng.standard_normal((N, H, W, 4 * A)) * 0.1).astype(np.float32)
    images = ImageList(torch.zeros(N, 48, 56, 3, device=dev),
                       torch.tensor([[48, 56]] * N, dtype=torch.int32, device=dev))
    t = lambda a: torch.from_numpy(a).to(dev)
    losses = rpn.losses(images, feats, [t(lg)], [t(dl)],
                        {"gt_boxes": t(gt), "is_valid": t(valid), "gt_is_crowd": t(crowd)})
    labs, dels = zip(*[otrain.rpn_targets(anchors, gt[i], valid[i], crowd[i], (1, 1, 1, 1),
                                          [0.3, 0.7], [0, -1, 1]) for i in range(N)])
    cls, loc = otrain.rpn_losses(np.concatenate(labs), np.concatenate(dels), lg.reshape(-1),
                                 dl.reshape(-1, 4), N, 256)
    assert losses["loss_rpn_cls"].item() == pytest.approx(cls, rel=1e-5)
    assert losses["loss_rpn_loc"].item() == pytest.approx(loc, rel=1e-5)


def _train_model(dev, **solver):
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = _cfg(True, **solver)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    model.train()
    return cfg, model


def test_training_step_gradients_reach_every_trainable_parameter(dev):
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg, model = _train_model(dev)
    batch = synthetic_train_batch(2, 256, 320, 0, dev)
    losses = model(batch)
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask"}
    for k, v in losses.items():
        assert torch.isfinite(v).item(), (k, v)
    sum(losses.values()).backward()
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    # FREEZE_AT = 2: stem + res2 frozen
    assert frozen and all(".stem." in n or ".stages.0." in n for n in frozen), frozen[:5]
    assert any(".stages.1." in n for n, _ in trainable)
    missing = [n for n, p in trainable if p.grad is None]
    assert not missing, missing[:10]
    bad = [n for n, p in trainable if not torch.isfinite(p.grad).all()]
    assert not bad, bad[:10]
    from detectron2_tensorflow_amd import _C
    _C.raise_on_errors(dev)


def test_trainer_overfits_one_batch(dev):
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg, model = _train_model(dev, BASE_LR=0.01, WARMUP_ITERS=0, IMS_PER_BATCH_BASE=2)
    trainer = Trainer(cfg, model)
    batch = synthetic_train_batch(2, 256, 320, 1, dev)
    hist = []
    for _ in range(25):
        losses = trainer.step(batch)
        hist.append({k: float(v) for k, v in losses.items()})
    assert all(np.isfinite(h["total_loss"]) for h in hist)
    first = np.mean([h["total_loss"] for h in hist[:3]])
    last = np.mean([h["total_loss"] for h in hist[-3:]])
    assert last < 0.8 * first, (first, last, hist[-1])


def test_mask_head_on_foreground_rows_matches_fixed_layout(dev):
    """The compacted mask branch (foreground rows only, as the reference's
    select_foreground_proposals) gives the fixed-slot layout's loss and
    mask-head gradients: the extra rows of the fixed layout are masked out."""
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg, model = _train_model(dev)
    batch = synthetic_train_batch(2, 256, 320, 2, dev)
    rh = model.roi_heads
    res = {}
    for compact in (False, True):
        model.zero_grad(set_to_none=True)
        rh.mask_compact_rows = compact
        torch.manual_seed(5)  # same subsampling draw
        losses = model(batch)
        # the other losses at weight 0: one backward must reach every
        # participant of the pooler / RPN gradient hand-offs (layers/handoff.py)
        others = sum(v for k, v in losses.items() if k != "loss_mask")
        (losses["loss_mask"] + 0.0 * others).backward()
        res[compact] = (losses["loss_mask"].item(),
                        {n: p.grad.clone() for n, p in rh.mask_head.named_parameters()
                         if p.grad is not None})
    assert rh.last_mask_rows is not None and rh.last_mask_rows % rh.MASK_ROW_BUCKET == 0
    assert res[True][0] == pytest.approx(res[False][0], rel=1e-5, abs=1e-7)
    assert res[True][1].keys() == res[False][1].keys() and res[True][1]
    for n, g in res[False][1].items():
        # summation order differs with the row count (split-K / wgrad partitions
        # of every dgrad and wgrad in the head): weight gradients are sums over
        # ~10^5 pixel terms with cancellation, so the bound is relative to the
        # tensor's largest entry (measured: up to 1.2e-3 of it on a handful of
        # the 262,144 deconv-weight entries; a wrong row or class would be O(1))
        torch.testing.assert_close(res[True][1][n], g, rtol=1e-4, atol=2e-3 * g.abs().max().item())
        bad = ((res[True][1][n] - g).abs() > 3e-4 * g.abs().max()).float().mean().item()
        assert bad < 1e-3, (n, bad)


def test_rpn_head_fused_1x1_matches_separate_convs(dev):
    """The fused 16-wide RPN-head 1x1 (one MFMA conv forward, one dgrad conv +
    one skinny X^T G pass backward) gives the separate objectness / delta
    convs' outputs and gradients (f64 reference of the same math)."""
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import StandardRPNHead
    cfg = _cfg(True)
    torch.manual_seed(0)
    head = StandardRPNHead(cfg, [ShapeSpec(channels=256, stride=s) for s in (4, 8, 16, 32, 64)]).to(dev)
    with torch.no_grad():  # non-trivial biases / weights
        for c in (head.objectness_logits, head.anchor_deltas):
            c.weights.normal_(0, 0.05)
            c.bias.normal_(0, 0.1)
    xs = [torch.randn(2, h, w, 256, device=dev) for h, w in ((40, 52), (20, 26))]
    for x in xs:
        x.requires_grad_(True)
    _, logits, deltas = head(xs)
    gl = [torch.randn_like(t) for t in logits]
    gd = [torch.randn_like(t) for t in deltas]
    torch.autograd.backward(logits + deltas, gl + gd)
    wo, bo = head.objectness_logits.weights, head.objectness_logits.bias
    wd, bd = head.anchor_deltas.weights, head.anchor_deltas.bias
    # float64 reference of the same graph
    share = [torch.relu(torch.nn.functional.conv2d(
        x.detach().double().permute(0, 3, 1, 2), head.conv.weights.detach().double().permute(3, 2, 0, 1),
        head.conv.bias.detach().double(), padding=1)).permute(0, 2, 3, 1) for x in xs]
    gwo = sum(s.reshape(-1, 256).t() @ g.double().reshape(-1, g.shape[-1]) for s, g in zip(share, gl))
    gwd = sum(s.reshape(-1, 256).t() @ g.double().reshape(-1, g.shape[-1]) for s, g in zip(share, gd))
    for s, lg, dl in zip(share, logits, deltas):
        torch.testing.assert_close(lg.double(), s @ wo.detach().double()[0, 0] + bo.detach().double(),
                                   rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(dl.double(), s @ wd.detach().double()[0, 0] + bd.detach().double(),
                                   rtol=1e-4, atol=1e-4)
    tol = lambda r: dict(rtol=1e-4, atol=1e-5 * r.abs().max().item())
    torch.testing.assert_close(wo.grad[0, 0].double(), gwo, **tol(gwo))
    torch.testing.assert_close(wd.grad[0, 0].double(), gwd, **tol(gwd))
    gbo = sum(g.double().reshape(-1, g.shape[-1]).sum(0) for g in gl)
    gbd = sum(g.double().reshape(-1, g.shape[-1]).sum(0) for g in gd)
    torch.testing.assert_close(bo.grad.double(), gbo, **tol(gbo))
    torch.testing.assert_close(bd.grad.double(), gbd, **tol(gbd))
    assert all(torch.isfinite(x.grad).all() for x in xs)


def test_rpn_head_relu_gate_in_1x1_dgrad_is_exact(dev):
    """The 3x3 share conv's ReLU backward applied in the fused 1x1 head's dgrad
    epilogue (share > 0 gate) gives bit-identical input and 3x3 weight / bias
    gradients to the unfused threshold_backward."""
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import StandardRPNHead, _RPNHead1x1Fn
    cfg = _cfg(True)
    torch.manual_seed(1)
    head = StandardRPNHead(cfg, [ShapeSpec(channels=256, stride=s) for s in (4, 8, 16, 32, 64)]).to(dev)
    xs0 = [torch.randn(2, h, w, 256, device=dev) for h, w in ((40, 52), (20, 26))]
    grads = []
    for gate in (False, True):
        _RPNHead1x1Fn.GATE = gate
        try:
            xs = [x.clone().requires_grad_(True) for x in xs0]
            for prm in head.parameters():
                prm.grad = None
            _, logits, deltas = head(xs)
            g = torch.Generator(device=dev).manual_seed(3)
            outs = logits + deltas
            torch.autograd.backward(outs, [torch.randn(t.shape, device=dev, generator=g) for t in outs])
            grads.append([x.grad.clone() for x in xs] +
                         [head.conv.weights.grad.clone(), head.conv.bias.grad.clone()])
        finally:
            _RPNHead1x1Fn.GATE = True
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_fused_momentum_sgd_matches_foreach_reference(dev):
    """d2mi_momentum_sgd (L2 gradient + per-tensor clip_by_norm + momentum in
    two launches) against the torch._foreach restatement on CPU: weight-decay
    groups, clipped and unclipped tensors, a tensor without gradient, tensors
    spanning several 64k chunks; three steps (momentum carried)."""
    from detectron2_tensorflow_amd.solver import MomentumSGD
    g = torch.Generator().manual_seed(0)
    shapes = [(3, 3, 64, 64), (256,), (1024, 300), (7,), (2, 2, 128, 520)]
    cpu = [torch.randn(s, generator=g) for s in shapes]
    gpu = [t.clone().to(dev) for t in cpu]
    groups = lambda ps: [{"params": ps[:2], "weight_decay": 0.0},
                         {"params": ps[2:4], "weight_decay": 1e-4},
                         {"params": ps[4:], "weight_decay": 0.5}]
    oc, og = MomentumSGD(groups(cpu), 0.9, 10.0), MomentumSGD(groups(gpu), 0.9, 10.0)
    for step in range(3):
        for i, (c, d) in enumerate(zip(cpu, gpu)):
            if i == 3:  # no gradient
                c.grad = d.grad = None
                continue
            gr = torch.randn(c.shape, generator=g) * (0.001 if i == 1 else 1.0)
            c.grad, d.grad = gr.clone(), gr.clone().to(dev)
        oc.step(0.02)
        og.step(0.02)
        for c, d in zip(cpu, gpu):
            torch.testing.assert_close(d.cpu(), c, rtol=2e-6, atol=2e-6)
    for a, b in zip(oc.accum, og.accum):
        torch.testing.assert_close(b.cpu(), a, rtol=1e-5, atol=1e-6)


def test_fused_momentum_sgd_unaligned_gradients_are_bit_identical(dev):
    """Gradients that are views into one flat buffer at offsets that are not
    16-B aligned (the all-reduce buckets of engine/reducer.py) give the same
    clipped update, bit for bit, as separate aligned gradients: the norm's
    scalar fallback sums in the float4 body's order (r6: the one-rank RCCL
    test drifted by 4e-9 once a third step clipped)."""
    from detectron2_tensorflow_amd.solver import MomentumSGD
    g = torch.Generator().manual_seed(3)
    shapes = [(7,), (3, 3, 64, 64), (1024, 300), (5,), (2, 2, 128, 520)]
    w0 = [torch.randn(s, generator=g).to(dev) for s in shapes]
    arms = {}
    for arm in ("aligned", "views"):
        ps = [w.clone() for w in w0]
        opt = MomentumSGD([{"params": ps[:3], "weight_decay": 1e-4},
                           {"params": ps[3:], "weight_decay": 0.0}], 0.9, 10.0)
        for step in range(3):
            gs = [torch.randn(s, generator=torch.Generator().manual_seed(10 * step + i)) * 3.0
                  for i, s in enumerate(shapes)]
            if arm == "aligned":
                for p, gr in zip(ps, gs):
                    p.grad = gr.to(dev)
            else:
                flat = torch.cat([gr.reshape(-1) for gr in gs]).to(dev)
                off = 0
                for p, gr in zip(ps, gs):
                    p.grad = flat[off: off + gr.numel()].view_as(p)
                    off += gr.numel()
                assert any(p.grad.data_ptr() % 16 for p in ps)
            opt.step(0.02)
        arms[arm] = (ps, opt.accum)
    for a, b in zip(arms["aligned"][0] + arms["aligned"][1], arms["views"][0] + arms["views"][1]):
        assert torch.equal(a, b)


def test_fused_momentum_sgd_bumps_parameter_versions(dev):
    """Weight caches (packed conv weights, the fused RPN 1x1) key on the
    parameters' version counters: the fused update must bump them."""
    from detectron2_tensorflow_amd.solver import MomentumSGD
    p = torch.randn(3, 3, 8, 8, device=dev)
    p.grad = torch.randn_like(p)
    v = p._version
    MomentumSGD([{"params": [p], "weight_decay": 0.0}]).step(0.1)
    assert p._version > v


def test_batched_frozen_bn_fold_matches_per_layer_fold(dev):
    """The backbone's FoldGroup (every trainable Conv2D + FrozenBN folded by
    one launch, one backward pair) gives the per-layer fold's losses and
    gradients exactly; a second forward with unchanged weights refolds (the
    first graph's results are taken once)."""
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    cfg, model = _train_model(dev)
    batch = synthetic_train_batch(2, 256, 320, 2, dev)
    convs = [m for m in model.backbone.modules() if getattr(m, "_fold_group", None) is not None]
    group = convs[0]._fold_group
    assert sum(m.fold_trainable() for m in convs) > 20
    res = {}
    for batched in (True, False, True):
        for m in convs:
            m._fold_group = group if batched else None
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        losses = model(batch)
        sum(losses.values()).backward()
        res.setdefault(batched, []).append(
            ({k: v.item() for k, v in losses.items()},
             {n: p.grad.clone() for n, p in model.backbone.named_parameters() if p.grad is not None}))
    assert any(s[3] for s in group.slots.values())
    (la, ga), (la2, ga2) = res[True]
    lb, gb = res[False][0]
    assert la == lb == la2 and ga.keys() == gb.keys() == ga2.keys() and ga
    for n in ga:
        assert torch.equal(ga[n], gb[n]) and torch.equal(ga[n], ga2[n]), n


def test_fused_rpn_loss_matches_tensor_formulation(dev):
    """ops.rpn_loss (targets + sigmoid CE + smooth-L1 in one HIP pass, analytic
    backward) equals the tensor formulation of RPNOutputs.losses in value and
    in the gradients of logits and deltas."""
    from detectron2_tensorflow_amd.layers import ops
    from detectron2_tensorflow_amd.layers.loss import smooth_l1_loss
    from detectron2_tensorflow_amd.modeling.box_regression import Box2BoxTransform
    g = torch.Generator().manual_seed(4)
    N, P, G, beta = 2, 5000, 6, 1.0 / 9
    cy, cx = torch.rand(P, generator=g) * 500, torch.rand(P, generator=g) * 700
    hh, ww = torch.rand(P, generator=g) * 100 + 8, torch.rand(P, generator=g) * 100 + 8
    anchors = torch.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2], 1)
    gt = anchors[torch.randint(0, P, (N * G,), generator=g)].reshape(N, G, 4) + \
        torch.randn(N, G, 4, generator=g) * 3
    matches = torch.randint(0, G, (N, P), generator=g)
    pos = torch.rand(N, P, generator=g) < 0.05
    sampled = pos | (torch.rand(N, P, generator=g) < 0.05)
    logits = torch.randn(N, P, generator=g) * 3
    deltas = torch.randn(N, P, 4, generator=g) * 0.3
    weights = (1.0, 1.0, 1.0, 1.0)
    t = lambda a: a.to(dev)
    lf, df = t(logits).requires_grad_(True), t(deltas).requires_grad_(True)
    cls, loc = ops.rpn_loss(lf, df, t(anchors), t(gt), t(matches), t(pos), t(sampled), weights,
                            beta)
    (cls * 0.7 + loc * 1.3).backward()
    lr, dr = t(logits).requires_grad_(True), t(deltas).requires_grad_(True)
    b2b = Box2BoxTransform(weights)
    matched = torch.gather(t(gt), 1, t(matches)[..., None].expand(-1, -1, 4))
    tgt = b2b.get_deltas(t(anchors)[None].expand(N, -1, -1).reshape(-1, 4),
                         matched.reshape(-1, 4)).reshape(N, P, 4)
    tgt = torch.where(t(pos)[..., None], tgt, torch.zeros_like(tgt))
    obj = torch.nn.functional.binary_cross_entropy_with_logits(lr, t(pos).float(), reduction="none")
    cls_r = torch.where(t(sampled), obj, torch.zeros_like(obj)).sum()
    l1 = smooth_l1_loss(labels=tgt, predictions=dr, beta=beta)
    loc_r = torch.where(t(pos)[..., None], l1, torch.zeros_like(l1)).sum()
    (cls_r * 0.7 + loc_r * 1.3).backward()
    assert cls.item() == pytest.approx(cls_r.item(), rel=1e-5)
    assert loc.item() == pytest.approx(loc_r.item(), rel=1e-5)
    torch.testing.assert_close(lf.grad, lr.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(df.grad, dr.grad, rtol=1e-5, atol=1e-6)
    # the normaliser folded into the op (d2mi_rpn_loss_bwd_ex): the sums times
    # scale, and the gradients of the scaled losses; only one loss used (the
    # other's gradient is a null pointer = zero)
    s = 1.0 / 512
    ls, ds = t(logits).requires_grad_(True), t(deltas).requires_grad_(True)
    cls_s, loc_s = ops.rpn_loss(ls, ds, t(anchors), t(gt), t(matches), t(pos), t(sampled),
                                weights, beta, scale=s)
    assert cls_s.item() == pytest.approx(cls.item() * s, rel=1e-6)
    assert loc_s.item() == pytest.approx(loc.item() * s, rel=1e-6)
    cls_s.backward()
    lr2 = t(logits).requires_grad_(True)
    obj2 = torch.nn.functional.binary_cross_entropy_with_logits(lr2, t(pos).float(),
                                                                reduction="none")
    (torch.where(t(sampled), obj2, torch.zeros_like(obj2)).sum() * s).backward()
    torch.testing.assert_close(ls.grad, lr2.grad, rtol=1e-5, atol=1e-9)
    assert ds.grad is not None and not ds.grad.any()


def _whole_step_vs_cpu(dev, height, width, post_topk, roi_batch, seed=3):
    """One HIP Trainer.step vs oracle/cpu_train.py at height x width (see the
    callers), every RPN anchor and ROI candidate sampled."""
    import cpu_train
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-InstanceSegmentation",
                                     "mask_rcnn_R_50_FPN_1x.yaml"))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    cfg.SOLVER.BASE_LR = 0.02
    cfg.SOLVER.WARMUP_ITERS = 0
    cfg.SOLVER.IMS_PER_BATCH_BASE = 2
    cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE = 1 << 20
    if post_topk is not None:
        cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = post_topk
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = roi_batch
    cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION = 1.0
    finalize(cfg, True, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    model.train()
    batch = synthetic_train_batch(2, height, width, seed, dev)
    calibrate_rcnn_scores(model, batch)               # BASELINE.md logit scales
    cpu = cpu_train.CPUTrainStep(model, cfg)          # deep copy of the same weights
    names = [n for n, p in model.named_parameters() if p.requires_grad
             and not n.startswith("backbone.")]
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters() if n in names}
    trainer = Trainer(cfg, model)
    g_losses = {k: float(v.detach()) for k, v in trainer.step(batch).items()}
    c_losses = cpu.step(batch["image"].cpu().numpy(), batch["image_shape"].cpu().numpy(),
                        {k: v.cpu() for k, v in batch["instances"].items()}, threads=16)
    for k, v in c_losses.items():
        assert abs(g_losses[k] - v) <= 1e-4 * max(abs(v), 1e-3), (k, g_losses[k], v)
    cparams = dict(cpu.m.named_parameters())
    checked, worst_w, worst_d = 0, 0.0, 0.0
    for n, p in model.named_parameters():
        if n not in before:
            continue
        g, c, w0 = p.detach().cpu(), cparams[n].detach(), before[n]
        dg, dc = g - w0, c - w0
        upd = dc.abs().max().item()
        diff = (g - c).abs().max().item()
        # weights to 1e-4 of their scale (zero-initialised biases: of the update)
        assert diff <= max(1e-4 * c.abs().max().item(), 5e-3 * upd, 1e-12), (n, diff)
        worst_w = max(worst_w, diff / max(c.abs().max().item(), 1e-12))
        # the update is stored rounded to the weight's ulp: allow 4 ulp of it
        ulp4 = 4 * torch.finfo(torch.float32).eps * w0.abs().max().item()
        if upd > 100 * ulp4:
            dd = (dg - dc).abs().max().item()
            assert dd <= 5e-3 * upd + ulp4, (n, dd, upd)
            worst_d = max(worst_d, dd / upd)
            checked += 1
    print(f"losses gpu {g_losses}\nlosses cpu {c_losses}\nworst weight rel diff {worst_w:.3g}, "
          f"worst update rel diff {worst_d:.3g} over {checked} tensors")
    assert checked > 25, checked
    return g_losses, c_losses, trainer




def test_whole_training_step_matches_cpu_restatement(dev):
    """One HIP Trainer.step vs oracle/cpu_train.py's CPUTrainStep.step on
    identical weights and batch (lib/engine/trainer.py:116-139,
    model_deploy.py:203-205), with EVERY candidate sampled: the RPN and ROI
    batch sizes exceed the candidate counts (2^20 anchors per image at
    positive fraction 0.5; 200 train proposals + GT per image under 512 at
    fraction 1.0), so the random subsampling is a permutation and every loss
    is order-invariant.  Pins A14 (RPN losses), A18 (label + sample), A19
    (box losses), A20 (mask loss) and A23 (clip_by_norm + Momentum-SGD)
    together: losses to 1e-4 relative, the updated FPN / RPN / ROI-head
    weights to 1e-4 of their scale, and their updates w1 - w0 to 5e-3 of the
    update's scale per tensor plus 4 ulp of the weight (an f32 weight of 0.03
    rounds its update to ~2e-9; ReLU units within f32 noise of zero pass or
    block their gradient differently: the box head's updates differ by
    ~1.5e-3), for the tensors whose update exceeds 100 such ulps."""
    _whole_step_vs_cpu(dev, 256, 320, post_topk=200, roi_batch=512)


def test_whole_training_step_1333x800_matches_cpu_restatement(dev):
    """The headline config itself (BASELINE C3: Mask R-CNN R50-FPN training,
    2 images at 1333x800 padded to 1344x800, the config's 1,000 post-NMS
    training proposals per image) against oracle/cpu_train.py with every
    candidate sampled: RPN batch 2^20 >= the 268,569 anchors per image, ROI
    batch 1,024 >= 1,000 proposals + 7 GT at fraction 1.0.  Same bars as the
    256x320 test (losses 1e-4 relative; weights and updates per tensor).
    Reference: lib/engine/trainer.py:116-139, lib/engine/model_deploy.py:203-205."""
    g, c, trainer = _whole_step_vs_cpu(dev, 800, 1333, post_topk=None, roi_batch=1024, seed=1000)
    rows = trainer.model.roi_heads.last_mask_rows
    print(f"1333x800: mask-branch rows {rows}")
    assert rows >= 32


@pytest.mark.parametrize("nreg", [80, 1])
def test_fused_fast_rcnn_loss_matches_tensor_formulation(dev, nreg):
    """ops.fast_rcnn_loss (csrc/roi_losses.hip: per-row CE + smooth-L1 with the
    targets formed in place, fixed-order reduction, analytic backward) equals
    FastRCNNOutputs.losses' tensor formulation (fast_rcnn_losses with
    FUSED_LOSSES off) in value and in the logits / deltas gradients; rows that
    are padding (valid False), background and foreground all present."""
    from detectron2_tensorflow_amd.modeling.box_regression import Box2BoxTransform
    from detectron2_tensorflow_amd.modeling.roi_heads import fast_rcnn as fr
    g = torch.Generator().manual_seed(5)
    B, K = 1024, 80
    cy, cx = torch.rand(B, generator=g) * 700, torch.rand(B, generator=g) * 1200
    hh, ww = torch.rand(B, generator=g) * 200 + 8, torch.rand(B, generator=g) * 200 + 8
    props = torch.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2], 1)
    gtb = props + torch.randn(B, 4, generator=g) * 6
    gtb[:, 2:] = torch.maximum(gtb[:, 2:], gtb[:, :2] + 2)
    cls = torch.randint(0, K + 1, (B,), generator=g)  # K = background
    valid = torch.rand(B, generator=g) < 0.85
    logits = torch.randn(B, K + 1, generator=g) * 3
    deltas = torch.randn(B, nreg * 4, generator=g) * 0.5
    b2b = Box2BoxTransform((10.0, 10.0, 5.0, 5.0))
    t = lambda a: a.to(dev)
    res = {}
    for fused in (True, False):
        fr.FUSED_LOSSES = fused
        try:
            lg, dl = t(logits).requires_grad_(True), t(deltas).requires_grad_(True)
            out = fr.fast_rcnn_losses(lg, dl, t(props), t(cls), t(gtb), t(valid), b2b, 0.5)
            (out["loss_cls"] * 0.7 + out["loss_box_reg"] * 1.3).backward()
            res[fused] = (out["loss_cls"].item(), out["loss_box_reg"].item(), lg.grad, dl.grad)
        finally:
            fr.FUSED_LOSSES = True
    a, b = res[True], res[False]
    assert a[0] == pytest.approx(b[0], rel=2e-6) and a[1] == pytest.approx(b[1], rel=2e-6)
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(a[3], b[3], rtol=1e-5, atol=1e-8)


def test_three_training_losses_evaluate_one_box_regression_formula(dev):
    """ops.rpn_loss, ops.fast_rcnn_loss (class-agnostic and class-specific) and
    ops.retina_loss, each fed the same (source box, GT box, predicted deltas,
    weights, beta) as its only positive row, give the same box loss and the
    same delta gradient to the bit: the three kernels evaluate the get_deltas
    and smooth-L1 of csrc/box_loss.h.  One positive row makes every reduction
    a sum with zeros, and max(1, #valid) = 1 makes the Fast R-CNN normaliser
    exact, so no tolerance is involved."""
    from detectron2_tensorflow_amd.layers import ops
    g = torch.Generator().manual_seed(11)
    A, K = 4, 4  # RPN anchors / RetinaNet anchors of the one cell; classes (K % 4 == 0)
    t = lambda a: a.to(dev)
    for case in range(32):
        weights = ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0))[case % 2]
        beta = (0.0, 1.0 / 9, 0.5, 1.0)[(case // 2) % 4]
        cy, cx = torch.rand(A, generator=g) * 500, torch.rand(A, generator=g) * 700
        hh, ww = torch.rand(A, generator=g) * 100 + 8, torch.rand(A, generator=g) * 100 + 8
        boxes = torch.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2], 1)
        j = case % A          # the positive anchor
        c = (case // A) % K   # its GT class
        src = boxes[j]
        gtb = src + torch.randn(4, generator=g) * 3
        gtb[2:] = torch.maximum(gtb[2:], gtb[:2] + 2)
        pred = torch.randn(4, generator=g) * 0.3
        onehot = torch.arange(A) == j
        losses, grads = {}, {}

        d = torch.randn(1, A, 4, generator=g) * 0.3
        d[0, j] = pred
        d = t(d).requires_grad_(True)
        _, loc = ops.rpn_loss(t(torch.zeros(1, A)), d, t(boxes), t(gtb.reshape(1, 1, 4)),
                              t(torch.zeros(1, A, dtype=torch.int64)), t(onehot[None]),
                              t(onehot[None]), weights, beta, scale=1.0)
        loc.backward()
        losses["rpn"], grads["rpn"] = loc.detach(), d.grad[0, j]

        for nreg in (1, K):
            col = 0 if nreg == 1 else c
            d = torch.randn(1, nreg * 4, generator=g) * 0.3
            d[0, col * 4:col * 4 + 4] = pred
            d = t(d).requires_grad_(True)
            _, box = ops.fast_rcnn_loss(t(torch.zeros(1, K + 1)), d, t(src[None]),
                                        t(torch.tensor([c])), t(gtb[None]),
                                        t(torch.tensor([True])), weights, beta)
            box.backward()
            losses[f"frcn{nreg}"] = box.detach()
            grads[f"frcn{nreg}"] = d.grad[0, col * 4:col * 4 + 4]

        d = torch.randn(1, 1, 1, A * 4, generator=g) * 0.3
        d[0, 0, 0, j * 4:j * 4 + 4] = pred
        d = t(d).requires_grad_(True)
        labels = torch.where(onehot, 1, -1)[None]
        _, box = ops.retina_loss([t(torch.zeros(1, 1, 1, A * K))], [d], t(boxes),
                                 t(gtb.reshape(1, 1, 4)), t(torch.tensor([[c]])),
                                 t(torch.zeros(1, A, dtype=torch.int64)), t(labels), K, A, 0.25,
                                 2.0, beta, weights)
        box.backward()
        losses["retina"], grads["retina"] = box.detach(), d.grad[0, 0, 0, j * 4:j * 4 + 4]

        for name in ("frcn1", f"frcn{K}", "retina"):
            where = (case, name, weights, beta, src.tolist(), gtb.tolist(), pred.tolist())
            assert torch.equal(losses[name], losses["rpn"]), (where, losses)
            assert torch.equal(grads[name], grads["rpn"]), (where, grads)
        assert losses["rpn"] > 0 and grads["rpn"].any()


@pytest.mark.parametrize("C", [80, 1])
def test_fused_mask_loss_matches_tensor_formulation(dev, C):
    """ops.mask_loss (csrc/roi_losses.hip) == mask_rcnn_loss's tensor
    formulation: value and the logits gradient (only each foreground row's
    class channel nonzero)."""
    from detectron2_tensorflow_amd.modeling.roi_heads import mask_head as mh
    rng = np.random.default_rng(3)
    B, G = 64, 6
    gt = np.stack([rng.uniform(0, 100, G), rng.uniform(0, 100, G),
                   rng.uniform(120, 300, G), rng.uniform(120, 300, G)], 1).astype(np.float32)
    masks = (rng.random((G, 56, 56)) < 0.5).astype(np.uint8)
    gi = rng.integers(0, G, B)
    boxes = (gt[gi] + rng.normal(0, 15, (B, 4))).astype(np.float32)
    cls = rng.integers(0, 80, B)
    fg = rng.random(B) < 0.6
    logits = rng.standard_normal((B, 28, 28, C)).astype(np.float32) * 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = {}
    for fused in (True, False):
        mh.FUSED_LOSSES = fused
        try:
            lg = t(logits).requires_grad_(True)
            loss = mh.mask_rcnn_loss(lg, t(boxes), t(gt[gi]), t(cls), t(masks), t(gi), t(fg), True)
            (loss * 1.7).backward()
            res[fused] = (loss.item(), lg.grad)
        finally:
            mh.FUSED_LOSSES = True
    assert res[True][0] == pytest.approx(res[False][0], rel=2e-6)
    torch.testing.assert_close(res[True][1], res[False][1], rtol=1e-5, atol=1e-9)


def test_fpn_join_engages_and_matches_plain_step(dev, monkeypatch):
    """In a real Mask R-CNN training step the stage-output join engages for
    C3 and C4 (the next stage's conv1 / shortcut pair + the FPN lateral: three
    members each; C2 is frozen) and the step's gradients equal those with the
    join off (FPN.JOIN_GRAD = False: autograd add + threshold_backward)."""
    from detectron2_tensorflow_amd.layers import handoff
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.modeling.necks.fpn import FPN
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 5, dev)
    calibrate_rcnn_scores(model, batch)
    calls = []

    def observe(label, event):
        # every arrival at a join deposits or completes it, exactly one of the two
        if label.startswith("join (") and event in ("deposit", "complete"):
            calls.append("lateral" if label == "join (lateral)" else "pair")

    monkeypatch.setattr(handoff, "OBSERVER", observe)
    # (no MIOpen conv on this path since the r3 MFMA stem; the flag keeps a
    # torch fallback conv -- strided 3x3 dgrad, grouped / dilated -- exact too)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    grads = {}
    for join in (True, False):
        monkeypatch.setattr(FPN, "JOIN_GRAD", join)
        model.zero_grad(set_to_none=True)
        calls.clear()
        torch.manual_seed(1)  # the same subsampling draws in both passes
        losses = model(batch)
        sum(losses.values()).backward()
        if join:
            assert sorted(calls) == ["lateral"] * 2 + ["pair"] * 4, calls
        else:
            assert calls == []
        grads[join] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads[True].keys() == grads[False].keys() and grads[True]
    for n in grads[True]:
        assert torch.equal(grads[True][n], grads[False][n]), n


def test_fpn_topdown_handoff_engages_and_matches_plain_step(dev, monkeypatch):
    """The FPN merged maps P5..P3 (inner) are read by their output conv and by
    the next finer lateral's fused top-down add: with FPN.TD_HANDOFF the two
    backwards hand the gradient over (the output conv adds it in its dgrad
    epilogue) -- engaged at three levels, and the step's gradients equal those
    of the autograd add (TD_HANDOFF False), bit for bit."""
    from detectron2_tensorflow_amd.layers import handoff
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.modeling.necks.fpn import FPN
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 5, dev)
    calibrate_rcnn_scores(model, batch)
    deposits = []
    monkeypatch.setattr(handoff, "OBSERVER",
                        lambda label, event: event == "deposit" and deposits.append(label))
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    grads = {}
    for td in (True, False):
        monkeypatch.setattr(FPN, "TD_HANDOFF", td)
        model.zero_grad(set_to_none=True)
        deposits.clear()
        torch.manual_seed(1)  # the same subsampling draws in both passes
        losses = model(batch)
        sum(losses.values()).backward()
        # (one deposit per hand-off level, by whichever of the two runs first)
        n_td = sum(1 for w in deposits if w in ("FPN top-down", "pair"))
        grads[td] = ({n: p.grad.clone() for n, p in model.named_parameters()
                      if p.grad is not None}, n_td)
    assert grads[True][1] - grads[False][1] == 3, (grads[True][1], grads[False][1])
    g1, g0 = grads[True][0], grads[False][0]
    assert g1.keys() == g0.keys() and g1
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n


@pytest.mark.parametrize("one_launch", [True, False])
def test_rpn_head_level_weight_grad_accumulator_is_exact(dev, monkeypatch, one_launch):
    """The RPN head's fused 1x1 and its shared 3x3 accumulate their weight /
    bias gradients over the FPN levels in one buffer each
    (d2mi_wgrad_skinny_levels -- one launch pair at the last level -- or
    d2mi_wgrad_skinny_ex accumulate per level; d2mi_conv2d_wgrad_ex bit 3,
    levels with one split included): the model's gradients equal those of
    per-level gradients summed by autograd, bit for bit."""
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import (StandardRPNHead,
                                                                           _RPNHead1x1Fn)
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 6, dev)
    calibrate_rcnn_scores(model, batch)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(_RPNHead1x1Fn, "LEVELS_ONE_LAUNCH", one_launch)
    grads = {}
    for acc in (True, False):
        monkeypatch.setattr(_RPNHead1x1Fn, "ACC_LEVELS", acc)
        monkeypatch.setattr(StandardRPNHead, "ACC_CONV_LEVELS", acc)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        losses = model(batch)
        sum(losses.values()).backward()
        grads[acc] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads[True].keys() == grads[False].keys()
    assert any("objectness_logits" in n for n in grads[True])
    for n in grads[True]:
        assert torch.equal(grads[True][n], grads[False][n]), n


def test_deferred_roi_pixel_passes_are_exact(dev, monkeypatch):
    """ops.roi.DEFER_PIXELS: the merged box / mask pooler backward prepares its
    contributions once (d2mi_roi_align_bwd2_ex phase 1) and each FPN level's
    pixel pass runs inside the RPN head conv's backward, into that conv's
    full dgrad map (phase 2, accumulate) -- no map clear, no epilogue add of
    a second full map.  Every level is deferred in a training step, and the
    model's gradients equal the full-map hand-off's bit for bit (old + new at
    each touched pixel is the same rounding as dgrad + pooled map)."""
    from detectron2_tensorflow_amd.layers import handoff, ops
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 8, dev)
    calibrate_rcnn_scores(model, batch)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    applied = []

    def observe(label, event):
        if label == "deferred pixels":  # "apply level <l>"
            applied.append(int(event.rsplit(" ", 1)[1]))

    monkeypatch.setattr(handoff, "OBSERVER", observe)
    grads = {}
    for defer in (True, False):
        monkeypatch.setattr(ops.roi, "DEFER_PIXELS", defer)
        model.zero_grad(set_to_none=True)
        applied.clear()
        torch.manual_seed(1)
        losses = model(batch)
        sum(losses.values()).backward()
        assert sorted(applied) == ([0, 1, 2, 3] if defer else []), applied
        grads[defer] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads[True].keys() == grads[False].keys() and grads[True]
    for n in grads[True]:
        assert torch.equal(grads[True][n], grads[False][n]), n


def test_training_step_1333x800_grads_finite_and_deterministic(dev):
    """The bench workload itself (Mask R-CNN R50-FPN, 2 images at 1333x800
    padded to 1344x800, BASELINE config C3 on one GPU): after one Trainer.step
    every trainable parameter holds a finite gradient that is not all zero
    (the FPN / RPN / ROI-head gradient hand-offs all completed), the losses are
    finite, and a second step from the same weights, momentum and RNG state is
    bit-identical (losses, gradients and updated weights)."""
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 800, 1333, 1000, dev)
    calibrate_rcnn_scores(model, batch)
    trainer = Trainer(cfg, model)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    w0 = [p.detach().clone() for _, p in named]
    acc0 = [a.clone() for a in trainer.optimizer.accum]
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True  # (any torch fallback conv: MIOpen)
    try:
        runs = []
        for _ in range(2):
            with torch.no_grad():
                for (_, p), w in zip(named, w0):
                    p.copy_(w)
                for a, a0 in zip(trainer.optimizer.accum, acc0):
                    a.copy_(a0)
            trainer.iter = 0
            torch.cuda.manual_seed(1234)
            losses = {k: v.detach().clone() for k, v in trainer.step(batch).items()}
            grads = [p.grad.detach().clone() if p.grad is not None else None for _, p in named]
            runs.append((losses, grads, [p.detach().clone() for _, p in named]))
    finally:
        torch.backends.cudnn.deterministic = old
    (l1, g1, p1), (l2, g2, p2) = runs
    for k, v in l1.items():
        assert torch.isfinite(v).all(), (k, v)
        assert torch.equal(v, l2[k]), (k, v, l2[k])
    # (calibrated mask logits ~ N(0, 1): a BCE near 0.8, not a saturated one)
    assert 0 < float(l1["loss_mask"]) < 3
    zero = []
    for (n, _), a, b in zip(named, g1, g2):
        assert a is not None, f"{n}: no gradient"
        assert torch.isfinite(a).all(), n
        assert torch.equal(a, b), f"{n}: gradient differs between identical steps"
        if not bool((a != 0).any()):
            zero.append(n)
    # only parameters that cannot receive a gradient from one random-init
    # step may come back all-zero (none expected)
    assert not zero, zero
    for (n, _), a, b in zip(named, p1, p2):
        assert torch.equal(a, b), n


def test_partial_backward_through_gradient_handoffs_raises(dev):
    """A backward that reaches only some participants of a gradient hand-off
    (here: the RPN losses alone, so the ROI poolers' share of the FPN levels
    and the RPN head's pair never completes) raises instead of dropping the
    deposited gradient; the state is cleared, and a full backward afterwards
    gives every trainable parameter a gradient."""
    from detectron2_tensorflow_amd.layers.handoff import HandoffError
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = _cfg(True)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 5, dev)
    calibrate_rcnn_scores(model, batch)
    model.train()
    losses = model(batch)
    with pytest.raises(HandoffError):
        (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    model.zero_grad(set_to_none=True)
    losses = model(batch)
    sum(losses.values()).backward()
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
