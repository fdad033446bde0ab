#!/usr/bin/env python
"""YOLOv4 training loss, forward + backward, both arms of
yolov4_outputs.FUSED_YOLO_LOSS in one process at the training shape: 4 images
of 608 x 608 (levels 76 / 38 / 19, A = 3, P = 22,743 predictions per image),
K = 80, G = 64 padded GT rows with about 10 valid ones per image.

  fused    ops.yolov4_loss: d2mi_yolov4_assign, d2mi_yolov4_loss_fwd, _bwd
  tensor   yolov4_outputs.yolov4_losses_dense in float32 on the GPU

The arms' outputs are compared first (states and counts exactly), then both
are timed as medians of interleaved rounds after a warm-up of each: the
three losses, their sum's backward to every level's logits.  The byte model
of the fused arm: the logits once forward (the five leading terms of every
row touch most of its cache lines) and the gradient written once backward,
4 * N * P * (5 + K) bytes each.  A second record times the eager Trainer step
of the shipped config built in the training phase at the same shape.

    python tools/yolo_loss_ab.py [--iters 2000] [--rounds 7] [--out profiles/yolo_loss_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectron2_tensorflow_amd import _C  # noqa: E402
from detectron2_tensorflow_amd.layers import ops  # noqa: E402
from detectron2_tensorflow_amd.modeling.single_stage_heads import yolov4_outputs as Y  # noqa: E402

CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
STRIDES = [8, 16, 32]
SIZES = [[[12, 16], [19, 36], [40, 28]], [[36, 75], [76, 55], [72, 146]],
         [[142, 110], [192, 243], [459, 410]]]
SCALE_YX = [1.2, 1.1, 1.05]
K, THRESH, CLS_NORM, IOU_NORM = 80, 0.5, 1.0, 0.07
HBM_BYTES_PER_S = 8.0e12  # the datasheet's HBM3E rate of the MI355X


def cell_anchors():
    return [torch.tensor([[0.0, 0.0, h, w] for w, h in level]) for level in SIZES]


def make_inputs(dev, N, size, G, valid_per_image):
    g = torch.Generator().manual_seed(0)
    logits = []
    for s in STRIDES:
        x = torch.randn(N, size // s, size // s, 3, 5 + K, generator=g)
        x[..., 2:4] = (x[..., 2:4] * 0.5).clamp(-2, 2)
        x[..., 4] = x[..., 4] * 2 - 3
        logits.append(x.reshape(N, size // s, size // s, 3 * (5 + K)).to(dev))
    rng = np.random.default_rng(0)
    boxes = np.zeros((N, G, 4), np.float32)
    valid = np.zeros((N, G), bool)
    for n in range(N):
        m = valid_per_image
        side = np.exp(rng.uniform(np.log(16), np.log(size / 2), (m, 2)))
        c = rng.uniform(0, size, (m, 2))
        boxes[n, :m] = np.concatenate([c - side / 2, c + side / 2], 1)
        valid[n, :m] = True
    classes = rng.integers(0, K, (N, G))
    return logits, torch.from_numpy(boxes).to(dev), torch.from_numpy(classes).to(dev), \
        torch.from_numpy(valid).to(dev)


def time_loss(a, dev):
    logits, boxes, classes, valid = make_inputs(dev, a.batch, a.size, a.gt, a.valid)
    cells = cell_anchors()
    leaves = [x.clone().requires_grad_(True) for x in logits]

    def run(fn, debug=None):
        conf, cls, box, npos, nneg = fn(leaves, STRIDES, cells, SCALE_YX, K, boxes, classes, valid,
                                        (a.size, a.size), THRESH, CLS_NORM, IOU_NORM, debug=debug)
        grads = torch.autograd.grad(conf + cls + box, leaves)
        return (conf, cls, box, npos, nneg), grads

    arms = {"fused": lambda d=None: run(ops.yolov4_loss, d),
            "tensor": lambda d=None: run(Y.yolov4_losses_dense, d)}
    outs, dbg = {}, {}
    for k, f in arms.items():  # (also the warm-up)
        dbg[k] = {}
        outs[k] = f(dbg[k])
    torch.cuda.synchronize()
    (fo, fg), (to, tg) = outs["fused"], outs["tensor"]
    same = {"state": bool(torch.equal(dbg["fused"]["state"], dbg["tensor"]["state"])),
            "num_pos": [int(fo[3]), int(to[3])], "num_neg": [int(fo[4]), int(to[4])],
            "loss_rel": [abs(x.item() - y.item()) / abs(y.item()) for x, y in zip(fo[:3], to[:3])],
            "grad_rel_to_max": [float((x - y).abs().max() / y.abs().max()) for x, y in zip(fg, tg)]}
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, f in arms.items():
            f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            iters = a.iters if k == "fused" else a.tensor_iters
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    P = sum(t.shape[1] * t.shape[2] * 3 for t in logits)
    nbytes = 4 * sum(t.numel() for t in logits)
    ideal_us = 2 * nbytes / HBM_BYTES_PER_S * 1e6
    return {"op": "yolov4_loss fwd+bwd", "batch": a.batch, "size": a.size, "P": P, "K": K,
            "G": a.gt, "valid_per_image": a.valid, "outputs_fused_vs_tensor": same,
            "fused_us": round(med["fused"], 1), "tensor_us": round(med["tensor"], 1),
            "ratio": round(med["tensor"] / med["fused"], 2),
            "logit_bytes": nbytes, "ciou_evaluations": a.batch * P * a.valid,
            "ideal_us_read_plus_write": round(ideal_us, 2),
            "share_of_ideal": round(ideal_us / med["fused"], 4),
            "fused_rounds_us": [round(v, 1) for v in times["fused"]],
            "tensor_rounds_us": [round(v, 1) for v in times["tensor"]],
            "iters": a.iters, "tensor_iters": a.tensor_iters, "device": torch.cuda.get_device_name(0)}


def time_step(a, dev):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
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
    model = model.to(dev).train()
    batch = synthetic_train_batch(a.batch, a.size, a.size, 0, dev, num_gt=a.valid)
    trainer = Trainer(cfg, model)
    rec = {"op": "yolov4 eager Trainer.step", "batch": a.batch, "size": a.size}
    for arm in (True, False):
        Y.FUSED_YOLO_LOSS = arm
        for _ in range(a.step_warmup):
            losses = trainer.step(batch)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            losses = trainer.step(batch)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        key = "fused" if arm else "tensor"
        rec[f"{key}_step_ms"] = round(statistics.median(ms), 2)
        rec[f"{key}_steps_ms"] = [round(v, 2) for v in ms]
        rec[f"{key}_finite"] = bool(all(torch.isfinite(v).all() for v in losses.values()))
    Y.FUSED_YOLO_LOSS = True
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="fused calls per timed window")
    ap.add_argument("--tensor-iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--gt", type=int, default=64)
    ap.add_argument("--valid", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_loss_ab.jsonl"))
    a = ap.parse_args()
    _C.load()
    dev = torch.device("cuda:0")
    results = [time_loss(a, dev)]
    print(json.dumps(results[-1]), flush=True)
    if not a.no_step:
        results.append(time_step(a, dev))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
