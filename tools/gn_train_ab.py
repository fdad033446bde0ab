#!/usr/bin/env python
"""GroupNorm with a gradient, two arms in one process:

  * "hip":   ops.norm.FUSED_GN_TRAIN = True, d2mi_group_norm_train_fwd / _bwd
             (csrc/group_norm.hip), the ReLU fused;
  * "torch": the toggle off: torch.nn.functional.group_norm on the permuted
             (NCHW) view of the NHWC tensor, then torch.relu.

forward + backward at the shapes of a training step on 1333 x 800 images, 2
per GPU: an FPN p2 output, a semantic-head 128-channel map, the box head's
[1024, 7, 7, 256], the mask head's [128, 14, 14, 256], and the SOLOv2 kernel
towers' level shapes (read from the shipped config's model by hooks on its
GroupNorm layers in one forward).  Each arm's outputs are compared with float64
first (a tensor beyond the 1e-4 bar is reported on stderr and in the line); then the arms
are timed with device events as medians of interleaved rounds after a warm-up
of each, with the GPU's clocks sampled over the timed rounds.  The HIP arm's
two calls are then timed one by one (ops.KernelTimer) against the bytes each
must move, as a fraction of the HBM peak.

--host-enqueue also times what the HOST spends on one forward + backward of
the HIP arm at each shape: a host clock around --iters calls with no device
wait inside ("enqueue"), and the same window closed by a device synchronise
("drained").  Where the two agree the call is bound by the host.

--step also times, in img/s and --repeats times each, the eager Trainer step
of configs/Misc/mask_rcnn_R_50_FPN_3x_gn.yaml, of solo_v2_R_50_FPN and of
Panoptic FPN R50 with the toggle on and off.  --tree DIR imports the package
from another checkout of the repository (the parent commit's, built there) and
times only those steps: its lines carry "tree": DIR.

One JSON line per measurement, also written to --out.

    python tools/gn_train_ab.py [--iters 100] [--rounds 7] [--host-enqueue] [--step]
                                [--skip-layers] [--tree DIR] [--out profiles/gn_train_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = None
if "--tree" in sys.argv[1:-1]:  # (before the package import below)
    TREE = ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
from detectron2_tensorflow_amd import _C  # noqa: E402
from detectron2_tensorflow_amd.layers import ops  # noqa: E402
from detectron2_tensorflow_amd.layers.ops import KernelTimer, norm  # noqa: E402

BAR = 1e-4  # the project's bar: |got - want| <= 1e-4 * max |want| per tensor
HBM_PEAK = 8e12  # B/s (MI355X, the figure of ops.timing's ridge points)
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
SHAPES = [("fpn p2", (2, 200, 336, 256), 32, False), ("sem-seg head", (2, 200, 336, 128), 32, True),
          ("box head", (1024, 7, 7, 256), 32, True), ("mask head", (128, 14, 14, 256), 32, True)]
STEPS = [("Misc/mask_rcnn_R_50_FPN_3x_gn", "configs/Misc/mask_rcnn_R_50_FPN_3x_gn.yaml"),
         ("solo_v2_R_50_FPN", "configs/COCO-InstanceSegmentation/solo_v2_R_50_FPN_1x.yaml"),
         ("panoptic_fpn_R_50", "configs/COCO-PanopticSegmentation/panoptic_fpn_R_50_1x.yaml")]


def set_toggle(on):
    if hasattr(norm, "FUSED_GN_TRAIN"):  # (the parent commit's tree has none)
        norm.FUSED_GN_TRAIN = on


def build(path, dev):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, path))
    if "mask_rcnn" in path:  # (training never pastes; Panoptic FPN keeps its image-size masks)
        cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    finalize(cfg, True, 1, CATS)
    torch.manual_seed(0)
    return cfg, build_model(cfg).to(dev).train()


def train_batch(name, dev):
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    full = (800, 1344) if name.startswith("solo") else None
    batch = synthetic_train_batch(2, 800, 1333, 1000, dev, full_mask_hw=full)
    if name.startswith("panoptic"):
        g = torch.Generator().manual_seed(3)
        batch["sem_seg"] = torch.randint(0, 54, (2, 800, 1333), generator=g,
                                         dtype=torch.int32).to(dev)
    return batch


def solo_tower_shapes(dev):
    """(layer, shape, groups, relu) of every distinct GroupNorm input in the
    SOLOv2 kernel towers of the shipped config at 1333 x 800, 2 images."""
    from detectron2_tensorflow_amd.layers import GroupNorm
    name, path = STEPS[1]
    _, model = build(path, dev)
    seen, hooks = {}, []

    def pre(mod, args, kwargs):
        key = (tuple(args[0].shape), mod.num_groups, bool(kwargs.get("relu", False)))
        seen.setdefault(key, len(seen))

    for n, m in model.named_modules():
        if isinstance(m, GroupNorm) and "mask_kernel" in n:
            hooks.append(m.register_forward_pre_hook(pre, with_kwargs=True))
    model(train_batch(name, dev))
    for h in hooks:
        h.remove()
    del model
    torch.cuda.empty_cache()
    return [(f"solo tower {s[1]}x{s[2]}x{s[3]}", s, g, r) for (s, g, r) in seen]


def float64_errors(x, gamma, beta, dy, G, relu, outs):
    """max |got - want| / max |want| of (y, dx, dgamma, dbeta) against the
    float64 formulas on the same float32 inputs, the ReLU mask being the
    checked arm's own y > 0."""
    y, dx, dgamma, dbeta = outs
    N, H, W, C = x.shape
    grp = lambda t: t.reshape(N, H * W, G, C // G)
    per = lambda t: t[:, None, :, None]
    xd, gm = x.detach().double(), gamma.detach().double()
    mean = grp(xd).mean(dim=(1, 3))
    r = 1.0 / torch.sqrt(((grp(xd) - per(mean)) ** 2).mean(dim=(1, 3)) + 1e-5)
    xh = ((grp(xd) - per(mean)) * per(r)).reshape(x.shape)
    z = xh * gm + beta.detach().double()
    dz = dy.double() * (y > 0) if relu else dy.double()
    m = H * W * (C // G)
    dzg = dz * gm
    S1, S2 = grp(dzg).sum(dim=(1, 3)), grp(dzg * xh).sum(dim=(1, 3))
    want = (torch.relu(z) if relu else z,
            ((grp(dzg) - per(S1 / m) - grp(xh) * per(S2 / m)) * per(r)).reshape(x.shape),
            (dz * xh).reshape(-1, C).sum(0), dz.reshape(-1, C).sum(0))
    return [float((g.double() - w).abs().max() / w.abs().max()) for g, w in zip(outs, want)]


def time_arms(arms, iters, rounds):
    clocks = {"error": "not sampled"}
    sampler = None
    try:
        sys.path.insert(0, HERE)
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


def layer_ab(dev, a, name, shape, G, relu):
    g = torch.Generator().manual_seed(0)
    C = shape[-1]
    leaf = (30 + 0.3 * torch.randn(shape, generator=g)).to(dev).requires_grad_(True)
    dy = torch.randn(shape, generator=g).to(dev)
    gamma = (0.5 + torch.rand(C, generator=g)).to(dev).requires_grad_(True)
    beta = torch.randn(C, generator=g).to(dev).requires_grad_(True)
    leaves = [leaf, gamma, beta]

    def arm(fused):
        def run():
            old = norm.FUSED_GN_TRAIN
            norm.FUSED_GN_TRAIN = fused
            try:
                y = ops.group_norm_train(leaf, G, gamma, beta, 1e-5, relu)
                return (y.detach(),) + torch.autograd.grad(y, leaves, dy)
            finally:
                norm.FUSED_GN_TRAIN = old
        return run

    arms = {"hip": arm(True), "torch": arm(False)}
    outs = {k: [t.clone() for t in f()] for k, f in arms.items()}  # (also the warm-up)
    names = ["y", "dx", "dgamma", "dbeta"]
    # each arm against float64 (on the GPU) under its own ReLU mask, as max
    # |got - want| / max |want| per tensor; the masks' differences counted
    # (an element whose z is within rounding of zero takes either side)
    vs64 = {k: dict(zip(names, float64_errors(leaf, gamma, beta, dy, G, relu, o)))
            for k, o in outs.items()}
    flips = int(((outs["hip"][0] > 0) != (outs["torch"][0] > 0)).sum()) if relu else 0
    y_gap = float((outs["hip"][0] - outs["torch"][0]).abs().max() / outs["torch"][0].abs().max())
    flagged = [f"{k} {n} {e:.1e}" for k, d in vs64.items() for n, e in d.items() if e > BAR]
    if flagged:
        print(f"WARNING {name} {shape}: beyond {BAR:g} of float64: " + ", ".join(flagged),
              file=sys.stderr, flush=True)
    del outs
    # windows of at least 50 ms: a shorter one times the clock and the scheduler
    arms["hip"]()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        arms["hip"]()
    torch.cuda.synchronize()
    iters = max(a.iters, int(0.05 / ((time.perf_counter() - t0) / 20)) + 1)
    times, clocks = time_arms(arms, iters, a.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    KernelTimer.reset()
    for _ in range(iters):
        arms["hip"]()
    passes = {}
    for k, (n, ms, byts) in KernelTimer.summary().items():
        if k.startswith("gn_train"):
            passes[k] = {"us": round(ms / n * 1e3, 1), "bytes": int(byts / n),
                         "hbm_fraction": round(byts / (ms * 1e-3) / HBM_PEAK, 3)}
    KernelTimer.reset(enabled=False)
    rec = {"op": "group_norm_train", "pass": "forward+backward", "layer": name,
           "shape": list(shape), "groups": G, "relu": relu, "vs_float64": vs64,
           "y_hip_vs_torch": y_gap, "relu_mask_flips": flips, "beyond_bar": flagged,
           "us": {k: round(v, 1) for k, v in med.items()},
           "rounds_us": {k: [round(t, 1) for t in v] for k, v in times.items()},
           "hip_passes": passes, "iters": iters, "clocks": clocks,
           "device": torch.cuda.get_device_name(0)}
    if a.host_enqueue:
        run = arms["hip"]
        enq, drained = [], []
        for _ in range(a.rounds):
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enq.append((t1 - t0) / iters * 1e6)
            drained.append((t2 - t0) / iters * 1e6)
        rec["hip_host_us"] = {"enqueue": round(statistics.median(enq), 1),
                              "drained": round(statistics.median(drained), 1),
                              "enqueue_rounds": [round(v, 1) for v in enq]}
    print(json.dumps(rec), flush=True)
    return rec


def step_ab(dev, a):
    from detectron2_tensorflow_amd.engine import Trainer
    out = []
    for name, path in STEPS:
        batch = train_batch(name, dev)
        for arm in (("parent",) if TREE is not None else ("hip", "torch")):
            set_toggle(arm == "hip")
            try:
                cfg, model = build(path, dev)
                # bench.py's score injection: a random-init model's raw logits
                # leave the samplers nothing sensible to train on
                sys.path.insert(0, HERE)
                from bench import calibrate_scores
                calibrate_scores(model, batch)
                trainer = Trainer(cfg, model)
                for _ in range(a.step_warmup):
                    losses = trainer.step(batch)
                runs = []
                for _ in range(a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        losses = trainer.step(batch)
                    torch.cuda.synchronize()
                    runs.append(2 * a.steps / (time.perf_counter() - t0))
                _C.raise_on_errors(dev)
                rec = {"img_per_s": round(statistics.median(runs), 2),
                       "runs_img_per_s": [round(r, 2) for r in runs],
                       "spread_img_per_s": round(max(runs) - min(runs), 2),
                       "total_loss": float(losses["total_loss"])}
            except Exception as e:  # (an arm that cannot train is a result, not the tool's end)
                rec = {"error": f"{type(e).__name__}: {e}"[:300]}
            finally:
                set_toggle(True)
            rec = dict({"op": "Trainer.step", "config": name, "arm": arm, "images": 2,
                        "size": [800, 1333], "steps": a.steps}, **rec,
                       device=torch.cuda.get_device_name(0))
            if TREE is not None:
                rec["tree"] = a.tree
            print(json.dumps(rec), flush=True)
            out.append(rec)
            trainer = model = None
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-enqueue", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--skip-layers", action="store_true", help="only the --step workloads")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gn_train_ab.jsonl"))
    a = ap.parse_args()
    _C.load()
    if not torch.cuda.is_available():
        raise SystemExit("gn_train_ab.py times GPU kernels: no GPU found")
    dev = torch.device("cuda:0")
    results = []
    if TREE is None and not a.skip_layers:
        results = [layer_ab(dev, a, *s) for s in SHAPES + solo_tower_shapes(dev)]
    if a.step or TREE is not None:
        results += step_ab(dev, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if TREE is not None else "w") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
