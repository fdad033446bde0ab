#!/usr/bin/env python
"""BatchNorm on batch statistics, three arms in one process:

  * "hip":    ops.norm.FUSED_BN_TRAIN = True, the kernels of csrc/batch_norm.hip;
  * "tensor": the toggle off, the tensor formulation of the same formulas;
  * "torch":  torch.nn.functional.batch_norm(training=True) on the permuted
              (NCHW) view of the NHWC tensor, then a separate add and ReLU.

forward + backward at the shapes of a training step on 1333 x 800 images, 2
per GPU (padded to 800 x 1344): a res3 / res4 / res5 conv3 output
(relu(bn + shortcut)), an FPN p2 output (bn alone) and the box head's
[1024, 7, 7, 256] (relu(bn)).  Outputs are compared first; then the arms are
timed with device events as medians of interleaved rounds after a warm-up of
each, with the GPU's clocks sampled over the timed rounds.  The HIP arm's
passes are then timed one by one (ops.KernelTimer) against the bytes each must
move, as a fraction of the HBM peak.

--host-enqueue also times what the HOST spends on one forward + backward of
the HIP arm at each shape: a host clock around --iters calls with no device
wait inside ("enqueue"), and the same window closed by a device synchronise
("drained").  Where the two agree the call is bound by the host.

--step also times the eager Trainer step of
configs/Misc/mask_rcnn_R_50_FPN_3x_syncbn.yaml, and of the same model built
with every BatchNorm in the inference form (moving statistics folded into the
convs), in img/s.  --tree DIR imports the package from another checkout of
the repository (the parent commit's, built there) and times only that step:
its lines carry "tree": DIR.

One JSON line per measurement, also written to --out.

    python tools/bn_train_ab.py [--iters 100] [--rounds 7] [--host-enqueue] [--step]
                                [--tree DIR] [--out profiles/bn_train_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = None
if "--tree" in sys.argv[1:-1]:  # (before the package import below)
    TREE = ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
from detectron2_tensorflow_amd import _C  # noqa: E402
from detectron2_tensorflow_amd.layers import ops  # noqa: E402
from detectron2_tensorflow_amd.layers.ops import KernelTimer, norm  # noqa: E402

HBM_PEAK = 8e12  # B/s (MI355X, the figure of ops.timing's ridge points)
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
SHAPES = [("res3 conv3", (2, 100, 168, 512), "relu_add"), ("res4 conv3", (2, 50, 84, 1024), "relu_add"),
          ("res5 conv3", (2, 25, 42, 2048), "relu_add"), ("fpn p2", (2, 200, 336, 256), "none"),
          ("box head", (1024, 7, 7, 256), "relu")]


def time_arms(arms, iters, rounds):
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


def layer_ab(dev, a, name, shape, variant):
    g = torch.Generator().manual_seed(0)
    C = shape[-1]
    x = (30 + 0.3 * torch.randn(shape, generator=g)).to(dev)
    res = torch.randn(shape, generator=g).to(dev) if variant == "relu_add" else None
    dy = torch.randn(shape, generator=g).to(dev)
    gamma = (0.5 + torch.rand(C, generator=g)).to(dev).requires_grad_(True)
    beta = torch.randn(C, generator=g).to(dev).requires_grad_(True)
    mode = {"none": norm.RELU_NONE, "relu": norm.RELU_BEFORE_ADD, "relu_add": norm.RELU_AFTER_ADD}[variant]
    leaf = x.clone().requires_grad_(True)
    rleaf = res.clone().requires_grad_(True) if res is not None else None
    leaves = [leaf, gamma, beta] + ([rleaf] if rleaf is not None else [])

    def ours(fused):
        def run():
            norm.FUSED_BN_TRAIN = fused
            try:
                mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
                y = ops.batch_norm_train(leaf, gamma, beta, mm, mv, 1e-5, 0.9, rleaf, mode)
                return (y.detach(),) + torch.autograd.grad(y, leaves, dy)
            finally:
                norm.FUSED_BN_TRAIN = True
        return run

    def stock():
        mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        perm = (0, 3, 1, 2) if len(shape) == 4 else (0, 1)
        back = (0, 2, 3, 1) if len(shape) == 4 else (0, 1)
        y = torch.nn.functional.batch_norm(leaf.permute(perm), mm, mv, gamma, beta, True, 0.1,
                                           1e-5).permute(back)
        if rleaf is not None:
            y = y + rleaf
        if variant != "none":
            y = torch.relu(y)
        return (y.detach(),) + torch.autograd.grad(y, leaves, dy)

    arms = {"hip": ours(True), "tensor": ours(False), "torch": stock}
    outs = {k: [t.clone() for t in f()] for k, f in arms.items()}  # (also the warm-up)
    names = ["y", "dx", "dgamma", "dbeta"] + (["dresidual"] if rleaf is not None else [])
    # y: max |hip - other| / max |other|.  The gradients: the fraction of
    # elements further apart than 1e-4 of the scale (an element whose
    # pre-activation is within rounding of zero takes either side of the ReLU
    # in two float32 evaluations: a max norm would report that one element)
    def apart(p, q):
        return float(((p - q).abs() > 1e-4 * q.abs().max()).float().mean())

    diff = {k: {n: (float((p - q).abs().max() / q.abs().max()) if n == "y" else apart(p, q))
                for n, p, q in zip(names, outs["hip"], outs[k])} for k in ("tensor", "torch")}
    del outs
    times, clocks = time_arms(arms, a.iters, a.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    # the HIP arm's passes, one by one
    KernelTimer.reset()
    for _ in range(a.iters):
        arms["hip"]()
    passes = {}
    for k, (n, ms, byts) in KernelTimer.summary().items():
        if k.startswith("bn_train"):
            passes[k] = {"us": round(ms / n * 1e3, 1), "bytes": int(byts / n),
                         "hbm_fraction": round(byts / (ms * 1e-3) / HBM_PEAK, 3)}
    KernelTimer.reset(enabled=False)
    rec = {"op": "batch_norm_train", "pass": "forward+backward", "layer": name, "shape": list(shape),
           "variant": variant, "hip_vs": diff,
           "us": {k: round(v, 1) for k, v in med.items()},
           "rounds_us": {k: [round(t, 1) for t in v] for k, v in times.items()},
           "hip_passes": passes, "iters": a.iters, "clocks": clocks,
           "device": torch.cuda.get_device_name(0)}
    if a.host_enqueue:
        run = arms["hip"]
        enq, drained = [], []
        for _ in range(a.rounds):
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                run()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enq.append((t1 - t0) / a.iters * 1e6)
            drained.append((t2 - t0) / a.iters * 1e6)
        rec["hip_host_us"] = {"enqueue": round(statistics.median(enq), 1),
                              "drained": round(statistics.median(drained), 1),
                              "enqueue_rounds": [round(v, 1) for v in enq]}
    print(json.dumps(rec), flush=True)
    return rec


def step_ab(dev, a):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils import training
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    batch = synthetic_train_batch(2, 800, 1333, 1000, dev)
    out = []
    for arm in ("batch statistics", "inference form"):
        cfg = get_cfg()
        cfg.merge_from_file(os.path.join(ROOT, "configs/Misc/mask_rcnn_R_50_FPN_3x_syncbn.yaml"))
        cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
        finalize(cfg, True, 1, CATS)
        if arm == "inference form":  # the builders read the phase: every layer frozen-form
            training.set_training_phase(False)
        torch.manual_seed(0)
        model = build_model(cfg).to(dev).train()
        training.set_training_phase(True)
        live = sum(1 for m in model.modules() if getattr(m, "batch_stats", False))
        trainer = Trainer(cfg, model)
        for _ in range(a.step_warmup):
            losses = trainer.step(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            losses = trainer.step(batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        _C.raise_on_errors(dev)
        rec = {"op": "Trainer.step", "config": "Misc/mask_rcnn_R_50_FPN_3x_syncbn", "arm": arm,
               "batch_stats_layers": live, "images": 2, "size": [800, 1333], "steps": a.steps,
               "img_per_s": round(2 * a.steps / dt, 2), "ms_per_step": round(dt / a.steps * 1e3, 1),
               "total_loss": float(losses["total_loss"]),
               "device": torch.cuda.get_device_name(0)}
        if TREE is not None:
            rec["tree"] = a.tree
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del trainer, model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-enqueue", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_train_ab.jsonl"))
    a = ap.parse_args()
    _C.load()
    if not torch.cuda.is_available():
        raise SystemExit("bn_train_ab.py times GPU kernels: no GPU found")
    dev = torch.device("cuda:0")
    results = [] if TREE is not None else [layer_ab(dev, a, *s) for s in SHAPES]
    if a.step or TREE is not None:
        results += step_ab(dev, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
