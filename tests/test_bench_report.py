"""bench.py's roofline objects from a synthetic KernelTimer summary (CPU):
every fraction is a fraction of its peak, and the ROIAlign backward's counter
bytes (one PMC "launch" = the whole backward) are divided by the backward's
summed launch time, not by one launch's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_kernel_report_fractions_and_roi_backward_accounting():
    import bench
    summary = {"conv2d_split": (10, 0.8, 10 * 11.7e9), "roi_align_bwd": (5, 0.255, 5.0e8)}
    extras = {"roi_align_bwd": {"unique_bytes": 2.7e7}}
    rep = bench.kernel_report(summary, mode="train", extras=extras)
    conv, roi = rep["conv2d_split"], rep["roi_align_bwd"]
    assert 0 < conv["frac"] < 1 and conv["unit"] == "TFLOP/s"
    assert roi["bytes_model"] == "unique" and 0 < roi["frac"] < 1
    if roi.get("traffic"):  # the committed PMC summary is present
        assert roi["traffic_per"].startswith("backward op")
        want = roi["traffic"] / 0.255e-3 / 1e9
        assert abs(roi["achieved_counter"] - want) < 0.2
        assert roi["frac_counter"] < 1


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    """--dump-outputs: every tensor of a step's nested output becomes
    <name>.npy in float32 (float64 for 64-bit values); an array over its share
    of the byte limit is stored as the same seeded sample on every call."""
    import numpy as np
    import torch
    import bench
    masks = (torch.arange(2 * 3 * 40 * 50) % 251).to(torch.uint8).reshape(2, 3, 40, 50)
    out = {"instances": {"masks": masks, "boxes": torch.rand(2, 3, 4),
                         "classes": torch.arange(6).reshape(2, 3)},
           "total_loss": torch.tensor(1.25, dtype=torch.float64)}
    limit = 4096
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(out, str(a), limit=limit)
    bench.dump_outputs(out, str(b), limit=limit)
    names = sorted(p.name for p in a.iterdir())
    assert names == ["instances.boxes.npy", "instances.classes.npy", "instances.masks.npy",
                     "total_loss.npy"]
    got = {n: np.load(a / n) for n in names}
    assert sum(v.nbytes for v in got.values()) <= limit
    assert got["instances.boxes.npy"].dtype == np.float32
    assert np.array_equal(got["instances.boxes.npy"], out["instances"]["boxes"].numpy())
    assert got["instances.classes.npy"].dtype == np.float64
    assert got["total_loss.npy"].dtype == np.float64 and got["total_loss.npy"] == 1.25
    m = got["instances.masks.npy"]
    assert m.dtype == np.float32 and m.shape == (limit // 4 // 4,)
    assert info["instances.masks"] == {"shape": [2, 3, 40, 50], "stored": m.size}
    assert set(m.tolist()) <= set(range(251)) and len(set(m.tolist())) > 1
    for n in names:
        assert np.array_equal(got[n], np.load(b / n))


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.full, args.dump_outputs, args.steps, args.warmup) == (False, None, 7, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"
