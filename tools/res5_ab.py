#!/usr/bin/env python
"""The C4 head's two toggles, each arm against the other in one process:

  * ops.res5.FUSED_POOL: the fused pool / gather (csrc/res5_pool.hip) against
    the tensor formulation (ops.res5_pool_dense: mean, index_select, and in the
    backward the broadcast and the index_add), forward + backward, at R = 1024,
    P = 49, C = 2048 with 128 mask rows;
  * Res5ROIHeads.ELIDE_STRIDE: the head of mask_rcnn_R_50_C4_1x on a 50 x 84 x
    1024 res4 map (an 800 x 1333 image) with and without the stride elision:
    inference at 1000 proposals of one image, training (forward + backward)
    at 2 x 512 sampled rows.

Outputs are compared first; then the arms are timed with device events as
medians of interleaved rounds after a warm-up of each, with the GPU's clocks
sampled over the timed rounds, and the peak allocated bytes of one call of
each arm recorded.  One JSON line per measurement, also written to --out.

    python tools/res5_ab.py [--iters 10] [--rounds 7] [--out profiles/res5_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectron2_tensorflow_amd import _C  # noqa: E402
from detectron2_tensorflow_amd.config import finalize, get_cfg  # noqa: E402
from detectron2_tensorflow_amd.layers import ShapeSpec, ops  # noqa: E402
from detectron2_tensorflow_amd.modeling.roi_heads import build_roi_heads  # noqa: E402
from detectron2_tensorflow_amd.structures import BoxList  # noqa: E402

CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}


class Images:
    def __init__(self, shapes):
        self.image_shapes = shapes


def peak_bytes(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del res
    return int(peak)


def time_arms(arms, iters, rounds):
    """{arm: per-call us of each round}, the arms interleaved, and the clock summary."""
    clocks = {"error": "not sampled"}
    sampler = None
    try:
        from bench import GpuSampler
        sampler = GpuSampler(torch.device("cuda:0"))
        sampler.start()
    except Exception as e:  # (informative only)
        clocks = {"error": f"{type(e).__name__}: {e}"}
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters * 1e3)
    if sampler is not None:
        sampler.stop()
        clocks = sampler.summary()
    return times, clocks


def record(rec, arms, a, names):
    x, y = names
    peak = {k: peak_bytes(f) for k, f in arms.items()}
    times, clocks = time_arms(arms, a.iters, a.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    rec.update({f"{x}_us": round(med[x], 1), f"{y}_us": round(med[y], 1),
                "ratio": round(med[y] / med[x], 3),
                f"{x}_peak_bytes": peak[x], f"{y}_peak_bytes": peak[y],
                f"{x}_rounds_us": [round(v, 1) for v in times[x]],
                f"{y}_rounds_us": [round(v, 1) for v in times[y]],
                "iters": a.iters, "clocks": clocks, "device": torch.cuda.get_device_name(0)})
    print(json.dumps(rec), flush=True)
    return rec


def pool_ab(dev, a, R=1024, P=49, C=2048, M=128):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(R, P, C, generator=g).to(dev)
    dst = torch.full((R,), -1, dtype=torch.int32)
    dst[torch.randperm(R, generator=g)[:M]] = torch.arange(M, dtype=torch.int32)
    dst = dst.to(dev)
    gp, gy = torch.randn(R, C, generator=g).to(dev), torch.randn(M, P, C, generator=g).to(dev)

    def make(fn):
        leaf = x.detach().clone().requires_grad_(True)

        def run():
            pooled, y = fn(leaf, dst, M)
            (dx,) = torch.autograd.grad([pooled, y], [leaf], [gp, gy])
            return pooled.detach(), y.detach(), dx
        return run

    arms = {"fused": make(ops.res5_pool), "dense": make(ops.res5_pool_dense)}
    outs = {k: [t.clone() for t in f()] for k, f in arms.items()}  # (also the warm-up)
    names = ("pooled", "y", "dx")
    diff = {n: float((p - q).abs().max()) for n, p, q in zip(names, outs["fused"], outs["dense"])}
    del outs
    xb = R * P * C * 4
    rec = {"op": "res5_pool", "pass": "forward+backward", "R": R, "P": P, "C": C, "M": M,
           "fused_vs_dense_max_abs": diff,
           # fused: X read, Y and pooled written; dY and dpooled read, dX written
           "fused_bytes": 2 * xb + 2 * (M * P * C * 4) + 2 * (R * C * 4)}
    return record(rec, arms, a, ("fused", "dense"))


def head_inputs(dev, N, P, seed=0):
    """A 50 x 84 x 1024 res4 map per image and P proposal-like boxes in 800 x 1333."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(N, 50, 84, 1024, generator=g).to(dev)
    y1 = torch.rand(N, P, generator=g) * 600
    x1 = torch.rand(N, P, generator=g) * 1100
    boxes = torch.stack([y1, x1, y1 + torch.rand(N, P, generator=g) * 180 + 16,
                         x1 + torch.rand(N, P, generator=g) * 220 + 16], -1).to(dev)
    props = BoxList(boxes)
    props.add_field("is_valid", torch.ones(N, P, dtype=torch.bool, device=dev))
    shapes = torch.tensor([[800, 1333]] * N, dtype=torch.int32, device=dev)
    return feat, props, shapes


def head_ab(dev, a):
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs/COCO-InstanceSegmentation/mask_rcnn_R_50_C4_1x.yaml"))
    finalize(cfg, False, 1, CATS)
    torch.manual_seed(0)
    head = build_roi_heads(cfg, {"res4": ShapeSpec(channels=1024, stride=16)},
                           scope="roi_heads").to(dev)
    with torch.no_grad():  # (a random-init res5 gives logits in the hundreds)
        head.box_predictor.cls_score.weights.mul_(0.01)

    def arm(elide, fn):
        def run():
            head.ELIDE_STRIDE = elide
            return fn()
        return run

    out = []
    # inference, one image, 1000 proposals
    feat, props, shapes = head_inputs(dev, 1, 1000)
    head.eval()

    def infer():
        with torch.no_grad():
            res, _ = head(Images(shapes), {"res4": feat}, props, None)
        return res.boxes, res.get_field("scores"), res.get_field("pred_masks")

    arms = {"elide": arm(True, infer), "literal": arm(False, infer)}
    outs = {k: [t.clone() for t in f()] for k, f in arms.items()}
    diff = {n: float((p - q).abs().max())
            for n, p, q in zip(("boxes", "scores", "masks"), outs["elide"], outs["literal"])}
    del outs
    rec = {"op": "Res5ROIHeads", "pass": "inference", "N": 1, "proposals": 1000,
           "elide_vs_literal_max_abs": diff}
    out.append(record(rec, arms, a, ("elide", "literal")))
    # training, 2 x 512 sampled rows, forward + backward
    feat, props, shapes = head_inputs(dev, 2, 1000, seed=1)
    gt = props.boxes[:, :8].clone()
    targets = {"gt_boxes": gt, "gt_classes": torch.arange(16, device=dev).reshape(2, 8) % 80,
               "is_valid": torch.ones(2, 8, dtype=torch.bool, device=dev),
               "gt_masks": (torch.rand(2, 8, 56, 56, device=dev) > 0.5).to(torch.uint8)}
    # (proposals near the ground truth, so that foreground rows exist)
    jitter = (torch.rand(2, 8, 12, 4, device=dev) - 0.5) * 20
    props.boxes[:, 8:104] = (gt[:, :, None, :] + jitter).reshape(2, 96, 4)
    head.train()
    leaf = feat.requires_grad_(True)
    params = [p for p in head.parameters() if p.requires_grad]

    def train():
        _, losses = head(Images(shapes), {"res4": leaf}, props, targets)
        grads = torch.autograd.grad(sum(losses.values()), [leaf] + params)
        return (torch.stack([v.detach() for v in losses.values()]), grads[0])

    arms = {"elide": arm(True, train), "literal": arm(False, train)}
    outs = {k: [t.clone() for t in f()] for k, f in arms.items()}
    diff = {n: float((p - q).abs().max())
            for n, p, q in zip(("losses", "dfeat"), outs["elide"], outs["literal"])}
    scale = {n: float(q.abs().max()) for n, q in zip(("losses", "dfeat"), outs["literal"])}
    del outs
    rec = {"op": "Res5ROIHeads", "pass": "training forward+backward", "N": 2, "rows": 1024,
           "mask_rows": head.last_mask_rows, "elide_vs_literal_max_abs": diff,
           "literal_max_abs": scale}
    out.append(record(rec, arms, a, ("elide", "literal")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res5_ab.json"))
    a = ap.parse_args()
    _C.load()
    if not torch.cuda.is_available():
        raise SystemExit("res5_ab.py times GPU kernels: no GPU found")
    dev = torch.device("cuda:0")
    results = [pool_ab(dev, a)] + head_ab(dev, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
