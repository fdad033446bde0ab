#!/usr/bin/env python
"""Per-shape time and TFLOP/s of the MFMA conv launches inside bench.py's step.

usage: python tools/conv_shapes.py [--mode train|infer] [--steps 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plan_of(key):
    """'family splits' of a KernelTimer conv / wgrad key, from the plan queries
    (ops.conv_plan / ops.wgrad_plan: what the launcher runs for aligned operands)."""
    import re
    from detectron2_tensorflow_amd.layers import ops
    w = key.split()
    N, H, W, Cin, Cout = map(int, re.match(r"(\d+)x(\d+)x(\d+)x(\d+)->(\d+)$", w[1]).groups())
    k, s = int(w[2][1:]), int(w[3][1:])
    if w[0] == "wgrad":
        p = ops.wgrad_plan(N, H, W, Cin, Cout, k, s, ((k - 1) // 2, k - 1 - (k - 1) // 2))
        return f"{ops.WGRAD_KERNELS[p['kernel']]} x{p['splits']}"
    tag = w[5] if len(w) > 5 else ""
    operands = (ops.OP_ALL_ALIGNED | ops.OP_WORKSPACE | (ops.OP_GATE if "g" in tag else 0)
                | (ops.OP_RESIDUAL if "r" in tag else 0))
    p = ops.conv_plan(N, H, W, Cin, Cout, k, s, (int(w[4][1]), int(w[4][2])), operands=operands)
    fam = ops.CONV_FAMILIES[p["family"]]
    if fam == "stream1x1":
        return f"{fam} tn{p['stream_tn']}"
    return f"{fam} x{p['main_splits']}" + (f" +tail x{p['tail_splits']}" if p["tail_tiles"] else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="train")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-handoff", action="store_true",
                    help="bottleneck residual-gradient hand-off off (A/B)")
    a = ap.parse_args()
    import bench
    sys.argv = [sys.argv[0], "--mode", a.mode]
    args = bench.parse()
    args.gpus = 1
    dev = torch.device("cuda", 0)
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers.ops import KernelTimer
    _C.load()
    cfg, model = bench.build(args, dev)
    if a.no_handoff:
        for m in model.modules():
            if hasattr(m, "grad_handoff"):
                m.grad_handoff = False
    batch = bench.synthetic_batch(args, dev, 0)
    bench.calibrate_scores(model, batch)
    if a.mode == "train":
        from detectron2_tensorflow_amd.engine import Trainer
        tr = Trainer(cfg, model)
        step = lambda: tr.step(batch)
        ctx = torch.enable_grad
    else:
        step = lambda: model.inference(batch)
        ctx = torch.no_grad
    with ctx():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        KernelTimer.reset(enabled=True, detail=True)
        for _ in range(a.steps):
            step()
        KernelTimer.enabled = False
    from detectron2_tensorflow_amd.layers.ops import SPLIT_RIDGE
    ex = KernelTimer.extras()
    rows = [(k, n, ms, w, ex.get(k, {}).get("bytes", 0.0))
            for k, (n, ms, w) in KernelTimer.summary().items()
            if k.startswith("conv ") or k.startswith("wgrad ")]
    rows.sort(key=lambda r: -r[2])
    tot = sum(r[2] for r in rows)
    # each shape against its own bound (verdict r4 weak #4): flop/B vs the
    # split ridge (416.7 TF/s / 8 TB/s); frac = TF/s / 416.7 (MFMA-bound) or
    # GB/s / 8000 (memory-bound, bytes = every operand once + the output once)
    print(f"{'shape':48s} {'kernel, splits':26s} {'calls/step':>10s} {'ms/step':>8s} {'TF/s':>7s} {'GB/s':>7s} "
          f"{'flop/B':>7s} {'bound':>5s} {'frac':>6s}")
    agg = {"mfma": [0.0, 0.0, 0.0], "hbm": [0.0, 0.0, 0.0]}
    for k, n, ms, w, b in rows:
        tf, gbs = w / ms / 1e9, b / ms / 1e6
        ai = w / max(b, 1.0)
        bound = "mfma" if ai >= SPLIT_RIDGE else "hbm"
        frac = tf / 416.7 if bound == "mfma" else gbs / 8000
        agg[bound][0] += ms
        agg[bound][1] += w
        agg[bound][2] += b
        print(f"{k:48s} {plan_of(k):26s} {n / a.steps:10.1f} {ms / a.steps:8.3f} {tf:7.1f} {gbs:7.1f} {ai:7.1f} "
              f"{bound:>5s} {frac:6.3f}")
    print(f"total {tot / a.steps:.3f} ms/step")
    for bound, (ms, w, b) in agg.items():
        if ms:
            f = (w / ms / 1e9 / 416.7) if bound == "mfma" else (b / ms / 1e6 / 8000)
            print(f"{bound}-bound shapes: {ms / a.steps:.3f} ms/step, frac {f:.3f} "
                  f"({'of the 416.7 TF/s split peak' if bound == 'mfma' else 'of 8 TB/s HBM'})")


if __name__ == "__main__":
    main()
