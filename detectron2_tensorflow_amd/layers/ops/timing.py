"""The benchmark's instrumentation of the op bindings: per-launch HIP-event
timing (KernelTimer) and the conv roofline's byte model and ridge points.
Imports no sibling module."""
import torch


class KernelTimer:
    """Opt-in per-launch HIP-event timing of the hot kernels (bench.py's live
    roofline).  Events are recorded on the launching stream around each call;
    ``work`` is the op's ALGORITHMIC flops (conv) or bytes (ROIAlign)."""

    enabled = False
    detail = False   # also key records by shape (tools/conv_shapes.py)
    records = []

    @classmethod
    def reset(cls, enabled=True, detail=False):
        cls.enabled = enabled
        cls.detail = detail
        cls.records = []

    @classmethod
    def start(cls):
        if not cls.enabled:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    @classmethod
    def stop(cls, ev0, name, work, extra=None):
        """extra: None or a zero-argument callable returning {key: amount} of
        further work models for this launch (evaluated after the timed region,
        by extras())."""
        if ev0 is None:
            return
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(torch.cuda.current_stream())
        cls.records.append((name, ev0, ev1, float(work), extra))

    @classmethod
    def summary(cls):
        """{name: (launches, total_ms, total_work)} (synchronises)."""
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, w, _ in cls.records:
            n, t, tw = out.get(name, (0, 0.0, 0.0))
            out[name] = (n + 1, t + e0.elapsed_time(e1), tw + w)
        return out

    @classmethod
    def extras(cls):
        """{name: {key: total}} of the launches' extra work models."""
        out = {}
        for name, _, _, _, ex in cls.records:
            if ex is None:
                continue
            d = out.setdefault(name, {})
            for k, v in ex().items():
                d[k] = d.get(k, 0.0) + float(v)
        return out


# ridge points of the two product forms: peak flops / HBM bandwidth
SPLIT_RIDGE = 2.5e15 / 6 / 8e12     # 52.1 flop/B (bf16 dense / 6 products)
F32_RIDGE = 157.3e12 / 8e12          # 19.7 flop/B (FP32 matrix)


def conv_bytes(x, w_packed, y, bias=None, topdown=None, residual=None, gate=None):
    """Least HBM bytes of one conv launch: every operand read once, the output
    written once."""
    n = x.numel() + w_packed.numel() + y.numel()
    for t in (bias, topdown, residual, gate):
        if t is not None:
            n += t.numel()
    return 4.0 * n


def bound_of(flops, byts, math_mode="split"):
    ridge = SPLIT_RIDGE if math_mode == "split" else F32_RIDGE
    return "mfma" if flops >= ridge * byts else "hbm"
