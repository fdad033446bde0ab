"""ops.sem_seg_loss forward + backward against the unfused composition already
in the tree (ops.resize_bilinear_grad + torch cross_entropy), same process,
alternating windows, device-synchronised host clock, at the workload's
2 x 200 x 336 x 54 -> 800 x 1344; also ops.sem_seg_argmax against
ops.resize_bilinear + zero pad + torch.argmax and ops.panoptic_combine at
D = 100.  Writes the JSON kept as profiles/sem_seg_loss_timing.json.

    python tools/bench_sem_seg.py [out.json]
"""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectron2_tensorflow_amd import _C  # noqa: E402
from detectron2_tensorflow_amd.layers import ops  # noqa: E402

assert torch.cuda.is_available(), "needs the GPU"
_C.load()
dev = torch.device("cuda:0")
N, h, w, C, LDC, S, IGN, WGT = 2, 200, 336, 54, 56, 4, 255, 0.5
H, W = h * S, w * S
g = torch.Generator().manual_seed(0)
logits = torch.randn(N, h, w, LDC, generator=g) * 3.0
logits[..., C:] = 0.0
labels = torch.randint(0, C, (N, H, W), generator=g, dtype=torch.int32)
labels[torch.rand(N, H, W, generator=g) < 0.2] = IGN
shapes = torch.tensor([[H, W], [H - 37, W - 11]], dtype=torch.int32)
x = logits.to(dev).requires_grad_(True)
lab, shp = labels.to(dev), shapes.to(dev)
# the unfused path's padded label copy, made once outside the timed window
ys, xs = torch.arange(H, device=dev)[None, :, None], torch.arange(W, device=dev)[None, None, :]
inside = (ys < shp[:, 0, None, None]) & (xs < shp[:, 1, None, None])
lab64 = torch.where(inside, lab.long(), torch.full_like(lab, IGN, dtype=torch.int64))


def fused():
    x.grad = None
    loss = ops.sem_seg_loss(x, lab, shp, IGN, S, WGT, num_classes=C)
    loss.backward()
    return loss.detach(), x.grad


def unfused():
    x.grad = None
    up = ops.resize_bilinear_grad(x[..., :C].contiguous(), (H, W))
    loss = F.cross_entropy(up.reshape(-1, C), lab64.reshape(-1), ignore_index=IGN) * WGT
    loss.backward()
    return loss.detach(), x.grad


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


lf, gf = fused()
lu, gu = unfused()
torch.cuda.synchronize()
diff = {"loss_fused": float(lf), "loss_unfused": float(lu),
        "grad_max_abs_diff": float((gf - gu).abs().max()), "grad_max_abs": float(gu.abs().max())}
for fn in (fused, unfused):  # warm-up of every shape in the timed windows
    window(fn, 10)
rounds = {"fused_ms": [], "unfused_ms": []}
for _ in range(5):  # alternating windows
    rounds["fused_ms"].append(window(fused, 200))
    rounds["unfused_ms"].append(window(unfused, 40))
mf, mu = sorted(rounds["fused_ms"])[2], sorted(rounds["unfused_ms"])[2]
xd = x.detach()
extra = {}
with torch.no_grad():
    extra["fused_forward_only_ms"] = window(
        lambda: ops.sem_seg_loss(xd, lab, shp, IGN, S, WGT, num_classes=C), 200)
    extra["argmax_fused_ms"] = window(lambda: ops.sem_seg_argmax(xd, shp, S, num_classes=C), 200)

    def argmax_unfused():
        full = ops.resize_bilinear(xd[..., :C].contiguous(), (H, W))
        full = torch.where(inside[..., None], full, torch.zeros_like(full))
        return torch.argmax(full, -1)

    extra["argmax_unfused_ms"] = window(argmax_unfused, 40)
    assert torch.equal(ops.sem_seg_argmax(xd, shp, S, num_classes=C), argmax_unfused())
    D = 100
    gm = torch.Generator().manual_seed(1)
    masks = torch.zeros(N, D, H, W, dtype=torch.uint8)
    for n in range(N):
        for d in range(D):
            y0, x0 = int(torch.randint(0, H - 200, (1,), generator=gm)), int(torch.randint(0, W - 200, (1,), generator=gm))
            masks[n, d, y0:y0 + 150, x0:x0 + 180] = 1
    sem = ops.sem_seg_argmax(xd, shp, S, num_classes=C)
    args = (masks.to(dev), torch.rand(N, D, generator=gm).to(dev),
            torch.randint(0, 80, (N, D), generator=gm).to(dev), torch.rand(N, D, 4, generator=gm).to(dev),
            torch.ones(N, D, dtype=torch.bool, device=dev), sem)
    extra["panoptic_combine_ms"] = window(
        lambda: ops.panoptic_combine(*args, 0.5, 4096, 0.5, 54), 20)
full = N * H * W * C * 4
low = N * h * w * LDC * 4
out = {"shape": [N, h, w, C, H, W], "protocol": "5 alternating windows (200 fused / 40 unfused "
       "iterations each), host clock around device synchronise, median window",
       "measured": dict(rounds, fused_median_ms=mf, unfused_median_ms=mu, ratio=mu / mf, **diff, **extra),
       "modelled_bytes": {
           "full_resolution_logits": full, "low_resolution_logits_ldc56": low,
           "labels_int32": N * H * W * 4,
           "fused_fwd_bwd_minimum": 2 * low + 2 * N * H * W * 4 + low,
           "unfused_fwd_bwd_minimum": 4 * full + 3 * low}}
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out["measured"]))
