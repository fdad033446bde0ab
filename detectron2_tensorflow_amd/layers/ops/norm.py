"""GroupNorm and bilinear resize on NHWC (csrc/group_norm.hip; the resize
kernel lives in solo.hip)."""
import torch

from ... import _C
from ._common import _f32c


# ---------------------------------------------------------------- GroupNorm
def group_norm(x, num_groups, gamma, beta, eps, relu=False, up2=False, accumulate_into=None):
    """GroupNorm (+ ReLU) on NHWC with the SOLOv2 feature-branch tail fused
    (d2mi_group_norm_nhwc): up2 writes the nearest x2 upsample; accumulate_into
    adds the result into that tensor (returned).  Inference only (no grad)."""
    x = _f32c(x)
    gamma, beta = _f32c(gamma), _f32c(beta)
    _C.require_device(x, gamma, beta)
    N, H, W, C = x.shape
    oshape = (N, 2 * H, 2 * W, C) if up2 else (N, H, W, C)
    if accumulate_into is not None:
        y = accumulate_into
        if tuple(y.shape) != oshape or not y.is_contiguous() or y.dtype != torch.float32:
            raise ValueError(f"accumulate_into must be a contiguous f32 {oshape} tensor")
    else:
        y = torch.empty(oshape, dtype=torch.float32, device=x.device)
    lib = _C.lib()
    wsb = lib.d2mi_group_norm_workspace_size(N, H, W, C, int(num_groups))
    ws = _C.workspace(wsb, x.device)
    rc = lib.d2mi_group_norm_nhwc(_C.ptr(x), N, H, W, C, int(num_groups), _C.ptr(gamma),
                                  _C.ptr(beta), float(eps), int(bool(relu)), int(bool(up2)),
                                  int(accumulate_into is not None), _C.ptr(y), _C.ptr(ws), wsb,
                                  _C.stream_of(x.device))
    _C.check(rc, "d2mi_group_norm_nhwc")
    return y


def group_norm_levels(xs, num_groups, gamma, beta, eps, relu=False):
    """The same GroupNorm (+ ReLU) over up to 6 feature levels in one set of
    launches (d2mi_group_norm_nhwc_levels): per level ops.group_norm's
    arithmetic.  Inference only (no grad)."""
    xs = [_f32c(x) for x in xs]
    gamma, beta = _f32c(gamma), _f32c(beta)
    _C.require_device(gamma, beta, *xs)
    if not 1 <= len(xs) <= 6:
        raise ValueError(f"group_norm_levels takes 1..6 levels, got {len(xs)}")
    C = xs[0].shape[-1]
    dims, ys = [], []
    for x in xs:
        if x.dim() != 4 or x.shape[-1] != C:
            raise ValueError(f"every level must be [N, H, W, {C}], got {tuple(x.shape)}")
        dims += [x.shape[0], x.shape[1], x.shape[2]]
        ys.append(torch.empty_like(x))
    dm = _C.host_array(_C.ctypes.c_int32, dims)
    lib = _C.lib()
    wsb = lib.d2mi_group_norm_levels_workspace_size(dm, len(xs), C, int(num_groups))
    ws = _C.scratch(wsb, xs[0].device) if wsb else None
    xp = _C.host_array(_C.c_void_p, [x.data_ptr() for x in xs])
    yp = _C.host_array(_C.c_void_p, [y.data_ptr() for y in ys])
    rc = lib.d2mi_group_norm_nhwc_levels(xp, dm, len(xs), C, int(num_groups), _C.ptr(gamma),
                                         _C.ptr(beta), float(eps), int(bool(relu)), yp,
                                         _C.ptr(ws), wsb, _C.stream_of(xs[0].device))
    _C.check(rc, "d2mi_group_norm_nhwc_levels")
    return ys


# ------------------------------------------------------------ resize / SOLOv2
class _ResizeBilinearFn(torch.autograd.Function):
    """The half-pixel ResizeBilinear with a gradient (SOLOv2 training: the
    head's grid resamples of the FPN maps): forward on the HIP kernel, the
    adjoint of the same bilinear weights (half-pixel centres, edge-clamped;
    PyTorch's align_corners=False sampling is that rule) for the backward."""

    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.in_shape = tuple(x.shape)
        return resize_bilinear(x.detach(), (oh, ow))

    @staticmethod
    def backward(ctx, g):
        N, H, W, C = ctx.in_shape
        gi = torch.ops.aten.upsample_bilinear2d_backward(
            g.permute(0, 3, 1, 2).contiguous(), [g.shape[1], g.shape[2]], [N, C, H, W], False,
            None, None)
        return gi.permute(0, 2, 3, 1), None, None


def resize_bilinear_grad(x, size):
    """resize_bilinear (half-pixel) that autograd can differentiate."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _ResizeBilinearFn.apply(x, int(size[0]), int(size[1]))
    return resize_bilinear(x, size)


def resize_bilinear(x, size, align_corners=False, half_pixel_centers=True):
    """TF ResizeBilinear on NHWC f32 (d2mi_resize_bilinear): x [N,H,W,C] ->
    [N, size[0], size[1], C]."""
    x = _f32c(x)
    _C.require_device(x)
    N, H, W, C = x.shape
    OH, OW = int(size[0]), int(size[1])
    y = torch.empty((N, OH, OW, C), dtype=torch.float32, device=x.device)
    rc = _C.lib().d2mi_resize_bilinear(_C.ptr(x), N, H, W, C, OH, OW, int(bool(align_corners)),
                                       int(bool(half_pixel_centers)), _C.ptr(y),
                                       _C.stream_of(x.device))
    _C.check(rc, "d2mi_resize_bilinear")
    return y
