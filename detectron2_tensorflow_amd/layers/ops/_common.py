"""What every family module shares: tensor coercions, the box-regression and
box-mode constants, and the tuning knobs with the workspace-size caches a
knob change invalidates, and the host tables that launches read from device
memory (_HostTable).  Imports no sibling module."""
import math

import numpy as np
import torch

from ... import _C
from ...utils import capture

_DEFAULT_SCALE_CLAMP = math.log(1000.0 / 16)  # lib/modeling/box_regression.py:10

BOX_MODE_RAW, BOX_MODE_ALIGNED, BOX_MODE_UNALIGNED = 0, 1, 2


def _f32c(t):
    if t.dtype is torch.float32 and t.is_contiguous():
        return t
    return t.to(torch.float32).contiguous()


def _i32c(t):
    if t.dtype is torch.int32 and t.is_contiguous():
        return t
    return t.to(torch.int32).contiguous()


def _mask_u8(m):
    """A [N, G] bool / integer mask as contiguous bytes (bool: a free view)."""
    if m is None:
        return None
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)


# workspace sizes per conv / wgrad shape (pure functions of the shape and the
# device's CU count: one ctypes query per distinct shape); filled by
# conv.conv2d_nhwc / conv2d_wgrad, kept beside set_tuning, which clears them
_CONV_WS, _WGRAD_WS = {}, {}


def get_tuning(key):
    """d2mi_get_tuning: the knob's current value."""
    v = _C.lib().d2mi_get_tuning(key.encode())
    if v == -2 ** 31:
        raise KeyError(f"unknown tuning key {key!r}")
    return v


def set_tuning(key, value):
    """d2mi_set_tuning (in-process A/B of kernel variants, tools/); clears the
    conv workspace-size cache, whose plans may depend on the knob."""
    _C.check(_C.lib().d2mi_set_tuning(key.encode(), int(value)), "d2mi_set_tuning")
    _CONV_WS.clear()
    _WGRAD_WS.clear()


class _HostTable:
    """A device copy of a host table uploaded through a small ring of pinned
    buffers (each slot reused once its previous copy has left, by event)."""
    RING = 4

    def __init__(self, nbytes, device, what="table"):
        self.what = what
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.ring = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        self.events = [None] * self.RING
        self.i = 0

    def upload(self, arr):
        if capture.capturing():  # a per-graph table, filled after the capture
            return capture.table(arr, self.dev.device, self.what)
        k = self.i
        self.i = (k + 1) % self.RING
        if self.events[k] is not None:
            self.events[k].synchronize()
        self.ring[k].numpy()[:] = arr.view(np.uint8)
        self.dev.copy_(self.ring[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        self.events[k] = ev
        return self.dev
