#!/usr/bin/env python
"""The fused relation attention (ops.relation_attention, csrc/relation.hip)
against the tensor formulation of the same math
(modeling.roi_heads.relation_module.relation_dense, which builds the
[N, R, R, E] embedding) in one process, at the head's default sizes (G = 16,
dk = 4, dv = 64, E = 64):

  * the training shape, N = 2, R = 512: forward + backward;
  * the inference shape, N = 2, R = 1000: forward only.

Outputs (and gradients) are compared first; then both arms are timed with
device events as medians of interleaved rounds after a warm-up of each, and
the peak allocated bytes of one call of each arm are recorded.  One JSON line
per shape, also written to --out.

    python tools/relation_ab.py [--iters 20] [--rounds 7] [--out profiles/relation_ab.json]
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
from detectron2_tensorflow_amd.layers import ops  # noqa: E402
from detectron2_tensorflow_amd.modeling.roi_heads import relation_dense  # noqa: E402

G, DK, DV, E = 16, 4, 64, 64


def inputs(dev, N, R, seed=0):
    """Proposal-like boxes in an 800 x 1333 image, every slot valid but the
    last 3 % of each image; q / k / v ~ N(0, 1); a small geometry conv with a
    positive bias."""
    g = torch.Generator().manual_seed(seed)
    y1 = torch.rand(N, R, generator=g) * 700
    x1 = torch.rand(N, R, generator=g) * 1200
    boxes = torch.stack([y1, x1, y1 + torch.rand(N, R, generator=g) * 99 + 1,
                         x1 + torch.rand(N, R, generator=g) * 132 + 1], -1)
    valid = torch.ones(N, R, dtype=torch.bool)
    valid[:, R - R * 3 // 100:] = False
    q = torch.randn(N, R, G * DK, generator=g)
    k = torch.randn(N, R, G * DK, generator=g)
    v = torch.randn(N, R, DV, generator=g)
    # (small: every pre-activation stays near the bias, away from the ReLU edge
    # and the 1e-6 clamp where the gradient jumps and the two arms' last bits
    # would decide the comparison; the time does not depend on the values)
    wg = torch.randn(E, G, generator=g) * 0.02
    bg = torch.full((G,), 0.5)
    d_out = torch.randn(N, R, G * DV, generator=g)
    return [t.to(dev) for t in (boxes, valid, q, k, v, wg, bg, d_out)]


def make_arm(fn, t, backward):
    boxes, valid, q, k, v, wg, bg, d_out = t
    if not backward:
        def run():
            with torch.no_grad():
                return (fn(boxes, valid, q, k, v, wg, bg, G),)
        return run
    leaves = [x.detach().clone().requires_grad_(True) for x in (q, k, v, wg, bg)]

    def run():
        out = fn(boxes, valid, *leaves, G)
        return (out.detach(),) + torch.autograd.grad(out, leaves, d_out)
    return run


def peak_bytes(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del res
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relation_ab.json"))
    a = ap.parse_args()
    _C.load()
    if not torch.cuda.is_available():
        raise SystemExit("relation_ab.py times GPU kernels: no GPU found")
    dev = torch.device("cuda:0")
    results = []
    for name, N, R, backward in (("train", 2, 512, True), ("inference", 2, 1000, False)):
        t = inputs(dev, N, R)
        arms = {"fused": make_arm(ops.relation_attention, t, backward),
                "dense": make_arm(relation_dense, t, backward)}
        outs = {k: [x.clone() for x in f()] for k, f in arms.items()}  # (also the warm-up)
        torch.cuda.synchronize()
        names = ("out", "dq", "dk", "dv", "dwg", "dbg")
        diff = {n: float((x - y).abs().max()) for n, x, y in zip(names, outs["fused"], outs["dense"])}
        scale = {n: float(y.abs().max()) for n, y in zip(names, outs["dense"])}
        del outs
        peak = {k: peak_bytes(f) for k, f in arms.items()}
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, f in arms.items():
                f()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"op": "relation_attention", "shape": name, "N": N, "R": R, "G": G, "dk": DK,
               "dv": DV, "E": E, "pass": "forward+backward" if backward else "forward",
               "fused_vs_dense_max_abs": diff, "dense_max_abs": scale,
               "fused_us": round(med["fused"], 1), "dense_us": round(med["dense"], 1),
               "ratio": round(med["dense"] / med["fused"], 2),
               "fused_peak_bytes": peak["fused"], "dense_peak_bytes": peak["dense"],
               "embedding_bytes": 4 * N * R * R * E,
               "fused_rounds_us": [round(v, 1) for v in times["fused"]],
               "dense_rounds_us": [round(v, 1) for v in times["dense"]],
               "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
