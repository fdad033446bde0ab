"""The C4 head's pool and gather (csrc/res5_pool.hip): the spatial mean of the
res5 output and the mask branch's row gather from one read of it, and their
backward as the one gradient of that output.  Owns the FUSED_POOL toggle."""
import torch

from ... import _C
from ._common import _f32c, _i32c

# True: Res5ROIHeads' mean + foreground gather run d2mi_res5_pool_fwd / _bwd on
# the GPU; False: the tensor formulation below (res5_pool_dense).  Tests and
# tools/res5_ab.py compare the two.  On by default: forward + backward at
# R = 1024, P = 49, C = 2048 with 128 mask rows take 212 us fused against 712 us
# (profiles/res5_ab.json, DESIGN.md section 5 "C4 head").
FUSED_POOL = True


def res5_pool_dense(x, dst=None, rows=0):
    """The same maths on tensors (any device / dtype): x [R, P, C] -> (pooled
    [R, C] = the mean over P, y [rows, P, C] with y[dst[r]] = x[r] for
    dst[r] >= 0, or None without dst).  Autograd forms the backward: the
    broadcast of dpooled / P plus an index_add of dy's rows."""
    pooled = x.mean(1)
    if dst is None:
        return pooled, None
    dst = dst.long()
    src = torch.nonzero(dst >= 0)[:, 0]
    y = x.new_zeros((int(rows),) + tuple(x.shape[1:]))
    return pooled, y.index_copy(0, dst[src], x.index_select(0, src))


class _Res5PoolFn(torch.autograd.Function):
    """(pooled, y) of d2mi_res5_pool_fwd; the backward is d2mi_res5_pool_bwd,
    which writes x's whole gradient from both outputs' gradients (no autograd
    add of two [R, P, C] tensors)."""

    @staticmethod
    def forward(ctx, x, dst, rows):
        R, P, C = x.shape
        dev = x.device
        pooled = torch.empty((R, C), dtype=torch.float32, device=dev)
        # (rows no dst names stay unwritten by the kernel: zero, as the dense arm's)
        y = (torch.zeros if dst is not None else torch.empty)(
            (rows if dst is not None else 0, P, C), dtype=torch.float32, device=dev)
        rc = _C.lib().d2mi_res5_pool_fwd(_C.ptr(x), R, P, C, _C.ptr(dst), rows, _C.ptr(pooled),
                                         _C.ptr(y) if rows else None, _C.stream_of(dev))
        _C.check(rc, "d2mi_res5_pool_fwd")
        ctx.dst, ctx.rows, ctx.shape = dst, rows, (R, P, C)
        ctx.set_materialize_grads(False)
        return pooled, y

    @staticmethod
    def backward(ctx, gp, gy):
        if gp is None and gy is None:
            return None, None, None
        R, P, C = ctx.shape
        dev = (gp if gp is not None else gy).device
        gp = _f32c(gp) if gp is not None else torch.zeros((R, C), dtype=torch.float32, device=dev)
        gy = _f32c(gy) if gy is not None and ctx.rows else None
        dx = torch.empty((R, P, C), dtype=torch.float32, device=dev)  # every element written
        rc = _C.lib().d2mi_res5_pool_bwd(_C.ptr(gp), _C.ptr(gy), _C.ptr(ctx.dst), R, P, C,
                                         ctx.rows, _C.ptr(dx), _C.stream_of(dev))
        _C.check(rc, "d2mi_res5_pool_bwd")
        return dx, None, None


def res5_pool(x, dst=None, rows=0):
    """x [R, P, C] f32 on the GPU -> (pooled [R, C], y [rows, P, C] or None):
    tf.reduce_mean(box_features, [1, 2]) and tf.gather(box_features, fg_inds)
    of lib/modeling/roi_heads/roi_heads.py:348, :371 in one launch.  dst [R]
    int32: the row of y that takes x[r], or -1; each value in [-1, rows), no
    destination named twice (a precondition: see d2mi_res5_pool_fwd)."""
    x = _f32c(x)
    if x.dim() != 3 or x.shape[2] % 4 or x.shape[1] < 1:
        raise ValueError(f"res5_pool: x {tuple(x.shape)} must be [R, P >= 1, C % 4 == 0]")
    if dst is not None:
        dst = _i32c(dst)
        if dst.shape != (x.shape[0],):
            raise ValueError(f"res5_pool: dst {tuple(dst.shape)} does not match x {tuple(x.shape)}")
    _C.require_device(x, dst)
    pooled, y = _Res5PoolFn.apply(x, dst, int(rows) if dst is not None else 0)
    return pooled, (y if dst is not None else None)
