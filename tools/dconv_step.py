"""Eager training step of the deformable Mask R-CNN config against the plain
one on the same box (bench.py's geometry: batch 2, 800x1333, synthetic batch,
calibrated random-init weights), with the per-group HIP-event times of the
deformable sampler.

    python tools/dconv_step.py [--steps 10] [--warmup 3] [--height 800] [--width 1333]

The dconv model's offsets are perturbed (offset_bias ~ normal(0, 1)): a fresh
layer's are all 0, which would time the sampler on the integer grid only.
Prints one JSON line per model and one with the ratio.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectron2_tensorflow_amd import _C  # noqa: E402
from detectron2_tensorflow_amd.layers import DeformConv2D, ops  # noqa: E402

CONFIGS = {"plain": "configs/COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_1x.yaml",
           "dconv": "configs/Misc/mask_rcnn_R_50_FPN_1x_dconv_c3-c5.yaml"}
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}


def run(name, a, dev):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, CONFIGS[name]))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    cfg.SOLVER.IMS_PER_GPU = a.batch
    finalize(cfg, training=True, world_size=1, category_map=CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, DeformConv2D):
                m.offset_bias.copy_(torch.randn(m.offset_bias.shape, generator=g))
    batch = synthetic_train_batch(a.batch, a.height, a.width, 1000, dev)
    calibrate_rcnn_scores(model, batch)
    trainer = Trainer(cfg, model)
    for _ in range(a.warmup):
        trainer.step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        losses = trainer.step(batch)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    ops.KernelTimer.reset(True)
    trainer.step(batch)
    groups = {k: {"launches": n, "ms": round(t, 3)}
              for k, (n, t, _) in ops.KernelTimer.summary().items() if k.startswith("deform")}
    ops.KernelTimer.reset(False)
    _C.raise_on_errors(dev)
    row = {"model": name, "eager_step_ms": round(ms, 2), "batch": a.batch,
           "image": [a.height, a.width], "steps": a.steps,
           "losses": {k: round(float(v), 4) for k, v in losses.items()}}
    if groups:
        row["deform_groups_one_step"] = groups
    print(json.dumps(row), flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    a = ap.parse_args()
    _C.load()
    dev = torch.device("cuda:0")
    plain = run("plain", a, dev)
    dconv = run("dconv", a, dev)
    print(json.dumps({"dconv_over_plain": round(dconv / plain, 3)}), flush=True)


if __name__ == "__main__":
    main()
