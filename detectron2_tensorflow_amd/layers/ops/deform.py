"""Deformable-conv sampling, forward and backward (csrc/deform_conv.hip)."""
import torch

from ... import _C
from ._common import _f32c
from .timing import KernelTimer


def _deform_geometry(x, offsets, k, stride, rate, pads, groups):
    N, H, W, C = x.shape
    pb, pe = pads
    k_eff = k + (k - 1) * (rate - 1)
    OH = (H + pb + pe - k_eff) // stride + 1
    OW = (W + pb + pe - k_eff) // stride + 1
    oc = 2 * groups * k * k
    if offsets.dim() != 4 or tuple(offsets.shape[:3]) != (N, OH, OW) or offsets.shape[3] < oc:
        raise ValueError(f"deform_sample: offsets {tuple(offsets.shape)} do not match "
                         f"{(N, OH, OW)} x >= {oc} channels")
    return N, H, W, C, OH, OW


def _deform_sample_fwd(x, offsets, k, stride, rate, pads, groups):
    N, H, W, C, OH, OW = _deform_geometry(x, offsets, k, stride, rate, pads, groups)
    cols = torch.empty((N, OH, OW, k * k * C), dtype=torch.float32, device=x.device)
    ev = KernelTimer.start()
    rc = _C.lib().d2mi_deform_sample_fwd(_C.ptr(x), _C.ptr(offsets), N, H, W, C, int(groups),
                                         int(k), int(stride), int(rate), int(pads[0]),
                                         int(pads[1]), int(offsets.shape[3]), _C.ptr(cols),
                                         _C.stream_of(x.device))
    # least bytes: x and the offsets read once, the columns written once
    KernelTimer.stop(ev, "deform_sample", 4.0 * (x.numel() + offsets.numel() + cols.numel()))
    _C.check(rc, "d2mi_deform_sample_fwd")
    return cols


def deform_sample_bwd(x, offsets, gcols, k, stride, rate, pads, groups, want_x=True,
                      want_offsets=True):
    """(gx [N,H,W,C], goffsets shaped like ``offsets``) of deform_sample
    (d2mi_deform_sample_bwd); None where not wanted.  gx is a deterministic
    sorted-key scatter sum (no float atomics, every element written);
    channels of ``offsets`` past 2*groups*k*k get a zero gradient."""
    x, offsets, gcols = _f32c(x), _f32c(offsets), _f32c(gcols)
    _C.require_device(x, offsets, gcols)
    N, H, W, C, OH, OW = _deform_geometry(x, offsets, k, stride, rate, pads, groups)
    if gcols.numel() != N * OH * OW * k * k * C:
        raise ValueError(f"deform_sample_bwd: gcols {tuple(gcols.shape)} != "
                         f"{(N, OH, OW, k * k * C)}")
    gx = torch.empty_like(x) if want_x else None
    goff = torch.empty_like(offsets) if want_offsets else None
    if gx is None and goff is None:
        return None, None
    lib = _C.lib()
    args = (N, H, W, C, int(groups), int(k), int(stride), int(rate), int(pads[0]), int(pads[1]))
    wsb = lib.d2mi_deform_sample_bwd_workspace_size(*args) if want_x else 0
    ws = _C.scratch(wsb, x.device) if wsb else None
    ev = KernelTimer.start()
    rc = lib.d2mi_deform_sample_bwd(_C.ptr(x), _C.ptr(offsets), _C.ptr(gcols), *args,
                                    int(offsets.shape[3]), int(offsets.shape[3]), _C.ptr(gx),
                                    _C.ptr(goff), _C.ptr(ws), wsb, _C.stream_of(x.device))
    # least bytes: gcols, x (for goffsets) and the offsets read once, both
    # gradients written once
    KernelTimer.stop(ev, "deform_sample_bwd",
                     4.0 * (gcols.numel() + offsets.numel() + (x.numel() if want_x else 0)
                            + (x.numel() + offsets.numel() if want_offsets else 0)))
    _C.check(rc, "d2mi_deform_sample_bwd")
    return gx, goff


class _DeformSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offsets, k, stride, rate, pads, groups):
        x, offsets = _f32c(x), _f32c(offsets)
        _C.require_device(x, offsets)
        ctx.save_for_backward(x, offsets)
        ctx.conf = (k, stride, rate, pads, groups)
        return _deform_sample_fwd(x, offsets, k, stride, rate, pads, groups)

    @staticmethod
    def backward(ctx, gcols):
        x, offsets = ctx.saved_tensors
        gx, goff = deform_sample_bwd(x, offsets, gcols, *ctx.conf,
                                     want_x=ctx.needs_input_grad[0],
                                     want_offsets=ctx.needs_input_grad[1])
        return gx, goff, None, None, None, None, None


def deform_sample(x, offsets, k, stride=1, rate=1, pads=(0, 0), groups=1):
    """Deformable-conv column matrix (d2mi_deform_sample_fwd, replacing
    lib/layers/convolutional.py:410-452): x [N,H,W,C] unpadded, pads (pb, pe)
    the implied zero ring, offsets [N,OH,OW,>= 2*groups*k*k] (extra channels
    ignored) -> cols [N,OH,OW,k*k*C], tap-major.  Differentiable in x and
    offsets."""
    return _DeformSampleFn.apply(x, offsets, int(k), int(stride), int(rate),
                                 (int(pads[0]), int(pads[1])), int(groups))
