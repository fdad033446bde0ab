#!/usr/bin/env python
"""YOLOv4 inference post-processing (ops.yolov4_inference) at 608x608 -- 4
images, levels 76 / 38 / 19, A = 3, K = 80, P = 22,743 predictions per image
-- against the unfused torch composition of the reference's ops
(yolov4_outputs.py:236-264, :352-367) in one process: sigmoid, the decode,
multiply, max, nonzero, gather, ops.non_max_suppression per image.  Two
inputs: the head logits of the seeded YOLOv4 model on a seeded batch, and iid
logits.  Outputs are compared first (validity and classes exactly, scores and
boxes to a few ulp: torch's sigmoid / exp are not the kernel's), then both are
timed as medians of interleaved rounds after a warm-up of each.  One JSON
line per input, also written to --out.

    python tools/yolo_post_ab.py [--iters 400] [--rounds 7] [--out profiles/yolo_post_ab.json]
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

CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
STRIDES = [8, 16, 32]
SIZES = [[[12, 16], [19, 36], [40, 28]], [[36, 75], [76, 55], [72, 146]],
         [[142, 110], [192, 243], [459, 410]]]
SCALE_YX = [1.2, 1.1, 1.05]
K, THRESH, NMS, MAX_DET = 80, 0.05, 0.5, 100


def cell_anchors():
    return [torch.tensor([[0.0, 0.0, h, w] for w, h in level]) for level in SIZES]


def model_logits(dev, N, size):
    """Head logits of the YOLOv4 config built with seed 0 (BatchNorm statistics
    and the pred biases randomised with seed 1, as tests/test_gpu_yolo.py) on
    a seeded uniform batch."""
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.layers import BatchNorm
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-Detection", "yolov4_D_53_PAN_1x.yaml"))
    finalize(cfg, False, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, BatchNorm):
                m.gamma.copy_(torch.rand(m.gamma.shape, generator=g) + 0.5)
                m.beta.copy_(torch.randn(m.beta.shape, generator=g) * 0.1)
                m.moving_mean.copy_(torch.randn(m.moving_mean.shape, generator=g) * 0.1)
                m.moving_variance.copy_(torch.rand(m.moving_variance.shape, generator=g) + 0.5)
        for pred in model.detector.head.preds:
            pred.bias.copy_(torch.randn(pred.bias.shape, generator=g) * 2 - 2)
        model = model.to(dev).eval()
        img = (torch.rand((N, size, size, 3), generator=g) * 255).to(dev)
        inp = {"image": img, "image_shape": torch.tensor([[size, size]] * N, device=dev)}
        feats = model.neck(model.backbone(model.preprocess_image(inp).tensor))
        det = model.detector
        return [t.contiguous() for t in det.head([feats[f] for f in det.in_features])]


def iid_logits(dev, N, size):
    """conf ~ N(-5, 2) (about 2 % of the predictions pass sigmoid(conf) > 0.05,
    as a trained model's objectness does), the rest N(0, 1)."""
    g = torch.Generator().manual_seed(0)
    out = []
    for s in STRIDES:
        x = torch.randn(N, size // s, size // s, 3, 5 + K, generator=g)
        x[..., 4] = x[..., 4] * 2 - 5
        out.append(x.reshape(N, size // s, size // s, 3 * (5 + K)).to(dev))
    return out


def unfused(logits, cells):
    """The reference's ops, one torch call each (_get_predictions, then
    inference_single_image per image with ops.non_max_suppression)."""
    boxes_all, probs_all = [], []
    for x, stride, cell, s in zip(logits, STRIDES, cells, SCALE_YX):
        N, H, W, _ = x.shape
        x = x.reshape(N, H, W, 3, 5 + K)
        ys = torch.arange(H, dtype=torch.float32, device=x.device)
        xs = torch.arange(W, dtype=torch.float32, device=x.device)
        grid = torch.stack(torch.meshgrid(ys, xs, indexing="ij"), -1)[None, :, :, None, :]
        dydx = s * torch.sigmoid(x[..., 0:2]) - 0.5 * (s - 1)
        yx = (grid + dydx) * stride
        hw = torch.exp(x[..., 2:4]) * cell.to(x.device)[:, 2:]
        boxes_all.append(torch.cat([yx - 0.5 * hw, yx + 0.5 * hw], -1).reshape(N, -1, 4))
        probs_all.append((torch.sigmoid(x[..., 4:5]) * torch.sigmoid(x[..., 5:])).reshape(N, -1, K))
    boxes, probs = torch.cat(boxes_all, 1), torch.cat(probs_all, 1)
    N = boxes.shape[0]
    ob = torch.zeros((N, MAX_DET, 4), device=boxes.device)
    os_ = torch.zeros((N, MAX_DET), device=boxes.device)
    oc = torch.zeros((N, MAX_DET), dtype=torch.int32, device=boxes.device)
    ov = torch.zeros((N, MAX_DET), dtype=torch.bool, device=boxes.device)
    for n in range(N):
        score_max, cls = probs[n].max(-1)
        idx = torch.nonzero(score_max > THRESH)[:, 0]
        b, sc, c = boxes[n][idx], score_max[idx], cls[idx]
        keep = ops.non_max_suppression(b, sc, MAX_DET, NMS).to(torch.int64)
        k = keep.shape[0]
        ob[n, :k], os_[n, :k], oc[n, :k], ov[n, :k] = b[keep], sc[keep], c[keep].to(torch.int32), True
    return ob, os_, oc, ov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_post_ab.json"))
    a = ap.parse_args()
    _C.load()
    dev = torch.device("cuda:0")
    cells = cell_anchors()
    results = []
    for name, make in (("model", model_logits), ("iid", iid_logits)):
        logits = make(dev, a.batch, a.size)
        P = sum(t.shape[1] * t.shape[2] * 3 for t in logits)
        arms = {
            "fused": lambda: ops.yolov4_inference(logits, STRIDES, cells, SCALE_YX, K, THRESH, NMS,
                                                  MAX_DET),
            "unfused": lambda: unfused(logits, cells),
        }
        outs = {k: [t.clone() for t in f()] for k, f in arms.items()}  # (also the warm-up)
        torch.cuda.synchronize()
        fb, fs, fc, fv = outs["fused"]
        ub, us, uc, uv = outs["unfused"]
        same = {"is_valid": bool(torch.equal(fv, uv)), "classes": bool(torch.equal(fc, uc)),
                "scores_max_abs": float((fs - us).abs().max()),
                "boxes_max_abs": float((fb - ub).abs().max())}
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
        nbytes = 4 * sum(t.numel() for t in logits)
        rec = {"op": "yolov4_inference", "input": name, "batch": a.batch, "size": a.size, "P": P,
               "K": K, "detections_per_image": [int(v) for v in fv.sum(1).tolist()],
               "outputs_vs_unfused": same,
               "fused_us": round(med["fused"], 1), "unfused_us": round(med["unfused"], 1),
               "ratio": round(med["unfused"] / med["fused"], 2),
               "dense_logit_bytes": nbytes,
               "fused_rounds_us": [round(v, 1) for v in times["fused"]],
               "unfused_rounds_us": [round(v, 1) for v in times["unfused"]],
               "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
