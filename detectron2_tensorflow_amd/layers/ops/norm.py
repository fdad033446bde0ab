"""GroupNorm, BatchNorm on batch statistics and bilinear resize on NHWC
(csrc/group_norm.hip, csrc/batch_norm.hip; the resize kernel lives in
solo.hip).  Owns the FUSED_BN_TRAIN and FUSED_GN_TRAIN toggles."""
import torch
import torch.distributed as dist

from ... import _C
from ._common import _f32c
from .timing import KernelTimer


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


# ------------------------------------------------------ GroupNorm, training
# True: a GroupNorm that needs a gradient runs d2mi_group_norm_train_fwd /
# _bwd on a GPU float32 tensor whose sizes those kernels take; False: torch's
# group_norm on the permuted (NCHW) view, then torch.relu (the arm that also
# serves CPU tensors and refused sizes).  Tests and tools/gn_train_ab.py
# compare the two; DESIGN section 5 has the measurements behind the default.
FUSED_GN_TRAIN = True

# whether the kernels take (N, C, G): what the C entries' own size check says
# (a workspace query answers 0 for sizes they refuse), asked once per triple
_GN_SIZES = {}


def _gn_sizes_ok(N, C, G):
    key = (N, C, G)
    ok = _GN_SIZES.get(key)
    if ok is None:
        ok = _GN_SIZES[key] = _C.lib().d2mi_group_norm_train_bwd_workspace_size(
            max(N, 1), 1, 1, C, G) > 0
    return ok


def gn_train_fused(x, C, G):
    """Whether ops.group_norm_train runs the HIP kernels for x [N, H, W, C]
    with G groups: the toggle, a GPU float32 tensor, and sizes the kernels
    take (C / G a multiple of 4, C <= 2048, G <= 64)."""
    return (FUSED_GN_TRAIN and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and _gn_sizes_ok(int(x.shape[0]), int(C), int(G)))


def group_norm_torch(x, num_groups, gamma, beta, eps, relu=False):
    """GroupNorm (+ ReLU) of NHWC x on torch's group_norm over the permuted
    (NCHW) view: the arm of CPU tensors, refused sizes and the toggle off."""
    y = torch.nn.functional.group_norm(x.permute(0, 3, 1, 2), num_groups, gamma, beta,
                                       eps).permute(0, 2, 3, 1)
    if relu:
        y = torch.relu(y)
    return y


# workspace bytes per (entry, N, H, W, C, G): pure functions of the shape
_GN_WS = {}


def _gn_workspace(query, shape, G, device):
    key = (query,) + tuple(shape) + (G,)
    wsb = _GN_WS.get(key)
    if wsb is None:
        wsb = _GN_WS[key] = getattr(_C.lib(), query)(*shape, G)
    return _C.scratch(wsb, device), wsb


class _GroupNormTrainFn(torch.autograd.Function):
    """GroupNorm (+ ReLU) on NHWC with the explicit backward of
    d2mi_group_norm_train_bwd.  Saves x, mean, var, gamma and beta; the
    backward recomputes the ReLU's mask from them."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, relu):
        xc = _f32c(x.detach())
        g, b = _f32c(gamma.detach()), _f32c(beta.detach())
        _C.require_device(xc, g, b)
        N, H, W, C = xc.shape
        y = torch.empty_like(xc)
        mean, var = torch.empty((2, N, G), dtype=torch.float32, device=xc.device).unbind(0)
        if N:
            ws, wsb = _gn_workspace("d2mi_group_norm_train_fwd_workspace_size", xc.shape, G,
                                    xc.device)
            # x three times (two moment passes, the apply), y once
            _bn_timed("gn_train_fwd", 16.0 * xc.numel(),
                      lambda: _C.lib().d2mi_group_norm_train_fwd(
                          _C.ptr(xc), N, H, W, C, G, _C.ptr(g), _C.ptr(b), eps, relu, _C.ptr(y),
                          _C.ptr(mean), _C.ptr(var), _C.ptr(ws), wsb, _C.stream_of(xc.device)))
        ctx.save_for_backward(xc, mean, var, g, b)
        ctx.conf = (G, eps, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, mean, var, g, b = ctx.saved_tensors
        G, eps, relu = ctx.conf
        N, H, W, C = xc.shape
        want_x, want_g, want_b = ctx.needs_input_grad[:3]
        if N == 0:  # nothing to launch: an empty dx, zero sums
            return (torch.empty_like(xc) if want_x else None,
                    torch.zeros_like(g) if want_g else None,
                    torch.zeros_like(b) if want_b else None, None, None, None)
        dyc = _f32c(dy)
        dx = torch.empty_like(xc) if want_x else None
        dgamma = torch.empty_like(g) if want_g else None
        dbeta = torch.empty_like(b) if want_b else None
        ws, wsb = _gn_workspace("d2mi_group_norm_train_bwd_workspace_size", xc.shape, G, xc.device)
        # the reduce pass reads x and dy; the apply pass reads both again and writes dx
        nbytes = 4.0 * xc.numel() * (2 + (3 if want_x else 0))
        _bn_timed("gn_train_bwd", nbytes,
                  lambda: _C.lib().d2mi_group_norm_train_bwd(
                      _C.ptr(xc), _C.ptr(dyc), N, H, W, C, G, _C.ptr(mean), _C.ptr(var), _C.ptr(g),
                      _C.ptr(b), eps, relu, _C.ptr(dx), _C.ptr(dgamma), _C.ptr(dbeta), _C.ptr(ws),
                      wsb, _C.stream_of(xc.device)))
        return dx, dgamma, dbeta, None, None, None


def group_norm_train(x, num_groups, gamma, beta, eps, relu=False):
    """GroupNorm (+ ReLU) of x [N, H, W, C] that autograd can differentiate
    (lib/layers/normalization.py:174-260).  Where gn_train_fused holds: the
    HIP kernels (y has ops.group_norm's bits); else torch's group_norm on the
    NCHW view, then torch.relu."""
    G = int(num_groups)
    if gn_train_fused(x, x.shape[-1], G):
        return _GroupNormTrainFn.apply(x, gamma, beta, G, float(eps), int(bool(relu)))
    return group_norm_torch(x, G, gamma, beta, eps, relu)


# ------------------------------------------- BatchNorm on batch statistics
# True: the batch-statistics BatchNorm of a GPU tensor with C % 4 == 0 runs
# the kernels of csrc/batch_norm.hip; False: the tensor formulation below (the
# arm that also serves CPU tensors and C % 4 != 0).  Tests and
# tools/bn_train_ab.py compare the two.
FUSED_BN_TRAIN = True

RELU_NONE, RELU_BEFORE_ADD, RELU_AFTER_ADD = 0, 1, 2


def _bn_fused(t, C=None):
    """The HIP arm takes a GPU tensor whose channel count is a multiple of 4."""
    return FUSED_BN_TRAIN and t.is_cuda and (t.shape[-1] if C is None else C) % 4 == 0


# workspace bytes per (entry, M, C): pure functions of the shape (one ctypes
# query per distinct shape)
_BN_WS = {}


def _bn_workspace(query, M, C, device):
    key = (query, M, C)
    wsb = _BN_WS.get(key)
    if wsb is None:
        wsb = _BN_WS[key] = getattr(_C.lib(), query)(M, C)
    return _C.scratch(wsb, device), wsb


def _bn_timed(name, nbytes, call):
    ev = KernelTimer.start()
    rc = call()
    _C.check(rc, name)
    KernelTimer.stop(ev, name, nbytes)


def bn_train_stats(x):
    """x [M, C] -> this replica's (count, mean [C], M2 [C]) as one row
    [2C + 1], M2 = sum (x - mean)^2 (d2mi_bn_train_stats, or two passes over
    the tensor)."""
    M, C = x.shape
    if not _bn_fused(x):
        mean = x.mean(0)
        m2 = (x - mean).square().sum(0)
        return torch.cat([x.new_full((1,), float(M)), mean, m2])
    row = torch.empty(2 * C + 1, dtype=torch.float32, device=x.device)
    ws, wsb = _bn_workspace("d2mi_bn_train_stats_workspace_size", M, C, x.device)
    _bn_timed("bn_train_stats", 4.0 * x.numel(),
              lambda: _C.lib().d2mi_bn_train_stats(_C.ptr(x), M, C, _C.ptr(row), _C.ptr(ws), wsb,
                                                   _C.stream_of(x.device)))
    return row


def bn_all_rows(row, sync):
    """[P, L]: this replica's row alone, or under ``sync`` the rows of every
    rank in rank order.  Each rank writes its row into a zeroed [world, L]
    buffer and one all_reduce(SUM) on the default group delivers all of them:
    adding zeros is exact, so every rank holds the same bits."""
    if not sync:
        return row[None]
    buf = row.new_zeros((dist.get_world_size(), row.numel()))
    buf[dist.get_rank()] = row
    dist.all_reduce(buf)
    return buf


def bn_sync_active(sync):
    """Whether a sync=True layer has replicas to talk to (no collective at
    world size 1)."""
    return bool(sync) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def bn_train_finalize(rows, eps, decay, moving_mean, moving_var):
    """rows [P, 2C + 1] merged in row order, weighted by their counts ->
    (mean, var (biased), invstd), and the moving averages updated
    in place: moving * decay + batch * (1 - decay) (d2mi_bn_train_finalize)."""
    P, L = rows.shape
    C = (L - 1) // 2
    if not _bn_fused(rows, C):
        n = rows[:, :1]
        total = n.sum()
        mean = (n * rows[:, 1:1 + C]).sum(0) / total
        m2 = (rows[:, 1 + C:] + n * (rows[:, 1:1 + C] - mean).square()).sum(0)
        var = m2 / total
        invstd = 1.0 / torch.sqrt(var + eps)
        with torch.no_grad():
            moving_mean.mul_(decay).add_(mean * (1.0 - decay))
            moving_var.mul_(decay).add_(var * (1.0 - decay))
        return mean, var, invstd
    rows = _f32c(rows)
    _C.require_device(moving_mean, moving_var)
    mean, var, invstd = torch.empty((3, C), dtype=torch.float32, device=rows.device).unbind(0)
    rc = _C.lib().d2mi_bn_train_finalize(_C.ptr(rows), P, C, float(eps), float(decay),
                                         _C.ptr(moving_mean), _C.ptr(moving_var), _C.ptr(mean),
                                         _C.ptr(var), _C.ptr(invstd), _C.stream_of(rows.device))
    _C.check(rc, "d2mi_bn_train_finalize")
    return mean, var, invstd


def _relu_mask(dy, z_or_y):
    return torch.where(z_or_y > 0, dy, torch.zeros_like(dy))


def bn_train_apply(x, mean, invstd, gamma, beta, residual, relu_mode):
    """y = (x - mean) * invstd * gamma + beta, then relu_mode / residual as
    d2mi_bn_train_apply states them."""
    M, C = x.shape
    if not _bn_fused(x):
        y = (x - mean) * invstd
        if gamma is not None:
            y = y * gamma
        if beta is not None:
            y = y + beta
        if relu_mode == RELU_BEFORE_ADD:
            y = torch.relu(y)
        if residual is not None:
            y = y + residual
        if relu_mode == RELU_AFTER_ADD:
            y = torch.relu(y)
        return y
    y = torch.empty_like(x)
    n = 2 + (residual is not None)
    _bn_timed("bn_train_apply", 4.0 * n * x.numel(),
              lambda: _C.lib().d2mi_bn_train_apply(
                  _C.ptr(x), M, C, _C.ptr(mean), _C.ptr(invstd), _C.ptr(gamma), _C.ptr(beta),
                  _C.ptr(residual), int(relu_mode), _C.ptr(y), _C.stream_of(x.device)))
    return y


def _bn_dz(x, dy, y, mean, invstd, gamma, beta, relu_mode):
    """(dz, xh) of the tensor arm: dy through the fused ReLU's mask."""
    xh = (x - mean) * invstd
    if relu_mode == RELU_BEFORE_ADD:
        z = xh if gamma is None else xh * gamma
        dy = _relu_mask(dy, z if beta is None else z + beta)
    elif relu_mode == RELU_AFTER_ADD:
        dy = _relu_mask(dy, y)
    return dy, xh


def bn_train_bwd_reduce(x, dy, y, mean, invstd, gamma, beta, relu_mode):
    """sums [2C] = (sum dz, sum dz * xh) over this replica's rows: dbeta and
    dgamma (d2mi_bn_train_bwd_reduce)."""
    M, C = x.shape
    if not _bn_fused(x):
        dz, xh = _bn_dz(x, dy, y, mean, invstd, gamma, beta, relu_mode)
        return torch.cat([dz.sum(0), (dz * xh).sum(0)])
    sums = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    ws, wsb = _bn_workspace("d2mi_bn_train_bwd_reduce_workspace_size", M, C, x.device)
    n = 2 + (relu_mode == RELU_AFTER_ADD)
    _bn_timed("bn_train_bwd_reduce", 4.0 * n * x.numel(),
              lambda: _C.lib().d2mi_bn_train_bwd_reduce(
                  _C.ptr(x), _C.ptr(dy), _C.ptr(y), M, C, _C.ptr(mean), _C.ptr(invstd),
                  _C.ptr(gamma), _C.ptr(beta), int(relu_mode), _C.ptr(sums), _C.ptr(ws), wsb,
                  _C.stream_of(x.device)))
    return sums


def bn_train_bwd_apply(x, dy, y, mean, invstd, gamma, beta, relu_mode, sums, total, want_res):
    """(dx, dresidual or None): dx = gamma * invstd * (dz - sums[:C] / total -
    xh * sums[C:] / total), dresidual = dz (d2mi_bn_train_bwd_apply)."""
    M, C = x.shape
    if not _bn_fused(x):
        dz, xh = _bn_dz(x, dy, y, mean, invstd, gamma, beta, relu_mode)
        gi = invstd if gamma is None else gamma * invstd
        dx = gi * (dz - sums[:C] / total - xh * (sums[C:] / total))
        return dx, (dz if want_res else None)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_res else None
    n = 3 + (relu_mode == RELU_AFTER_ADD) + bool(want_res)
    _bn_timed("bn_train_bwd_apply", 4.0 * n * x.numel(),
              lambda: _C.lib().d2mi_bn_train_bwd_apply(
                  _C.ptr(x), _C.ptr(dy), _C.ptr(y), M, C, _C.ptr(mean), _C.ptr(invstd),
                  _C.ptr(gamma), _C.ptr(beta), int(relu_mode), _C.ptr(sums), float(total),
                  _C.ptr(dx), _C.ptr(dres), _C.stream_of(x.device)))
    return dx, dres


class _BatchNormTrainFn(torch.autograd.Function):
    """BatchNorm on batch statistics (lib/layers/normalization.py:97-165) with
    the explicit backward
        dbeta = sum dz, dgamma = sum dz * xh,
        dx = gamma * invstd * (dz - mean_M(dz) - xh * mean_M(dz * xh)),
    xh = (x - mean) * invstd and mean_M over every row the statistics were
    taken over.  Each step has the HIP arm and the tensor arm; the
    cross-replica exchange between the passes is shared by both."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, moving_mean, moving_var, eps, decay, relu_mode,
                sync, stats_out):
        shape = x.shape
        x2 = _f32c(x.detach()).reshape(-1, shape[-1])
        res2 = None if residual is None else _f32c(residual.detach()).reshape(x2.shape)
        g = None if gamma is None else _f32c(gamma.detach())
        b = None if beta is None else _f32c(beta.detach())
        rows = bn_all_rows(bn_train_stats(x2), sync)
        mean, var, invstd = bn_train_finalize(rows, eps, decay, moving_mean, moving_var)
        y = bn_train_apply(x2, mean, invstd, g, b, res2, relu_mode)
        # the rows of all replicas: known on the host locally; under sync read
        # back from the exchanged counts (the sync path's one host read per
        # layer and step)
        ctx.total = float(rows[:, 0].sum()) if sync else float(x2.shape[0])
        y = y.reshape(shape)
        ctx.save_for_backward(x2, mean, invstd, g, b, y if relu_mode == RELU_AFTER_ADD else None)
        ctx.conf = (shape, relu_mode, sync, residual is not None)
        if stats_out is not None:
            stats_out.update(mean=mean, var=var, invstd=invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, mean, invstd, g, b, y = ctx.saved_tensors
        shape, relu_mode, sync, has_res = ctx.conf
        dy2 = _f32c(dy).reshape(x2.shape)
        y = None if y is None else y.reshape(x2.shape)
        sums = bn_train_bwd_reduce(x2, dy2, y, mean, invstd, g, b, relu_mode)
        C = x2.shape[1]
        total = ctx.total
        allsums = sums
        if sync:
            allsums = bn_all_rows(sums, True).sum(0)  # (rank order: the same bits everywhere)
        want_res = has_res and ctx.needs_input_grad[3]
        dx, dres = bn_train_bwd_apply(x2, dy2, y, mean, invstd, g, b, relu_mode, allsums, total,
                                      want_res)
        dgamma = sums[C:] if g is not None and ctx.needs_input_grad[1] else None
        dbeta = sums[:C] if b is not None and ctx.needs_input_grad[2] else None
        return (dx.reshape(shape) if ctx.needs_input_grad[0] else None, dgamma, dbeta,
                dres.reshape(shape) if dres is not None else None,
                None, None, None, None, None, None, None)


def batch_norm_train(x, gamma, beta, moving_mean, moving_var, eps, decay, residual=None,
                     relu_mode=RELU_NONE, sync=False, stats_out=None):
    """BatchNorm of x [..., C] on the statistics of its own rows (with
    ``sync`` and more than one rank: of every replica's rows), moving averages
    updated in place; ``residual`` / ``relu_mode`` fuse the add and the ReLU
    that follow it.  stats_out: a dict that receives mean / var / invstd."""
    if x.dim() < 2:
        raise ValueError(f"batch_norm_train: x {tuple(x.shape)} must be [..., C]")
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"batch_norm_train: residual {tuple(residual.shape)} does not match x "
                         f"{tuple(x.shape)}")
    if relu_mode == RELU_AFTER_ADD and residual is None:
        relu_mode = RELU_BEFORE_ADD
    return _BatchNormTrainFn.apply(x, gamma, beta, residual, moving_mean, moving_var, float(eps),
                                   float(decay), int(relu_mode), bn_sync_active(sync), stats_out)


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
