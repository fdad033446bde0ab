"""Float64 restatement of BatchNorm on batch statistics
(lib/layers/normalization.py:97-165 as tf.layers.BatchNormalization computes
it in training): plain torch float64 on the same float32 inputs, for the
forward, the moving-average update and the explicit backward.

    mean = E[x], var = E[(x - mean)^2] (biased), xh = (x - mean) * rsqrt(var + eps)
    z = xh * gamma + beta
    y = z | relu(z) | relu(z) + residual | z + residual | relu(z + residual)
    moving = moving * decay + batch * (1 - decay)
    dbeta = sum dz, dgamma = sum dz * xh
    dx = gamma * invstd * (dz - mean_M(dz) - xh * mean_M(dz * xh)), dresidual = dz

The rows are those of the last axis' complement: [N, H, W, C] or [R, C].
"""
import torch

BAR = 1e-4  # the README's "within 1e-4": |got - want| <= BAR * max|want| per tensor


def d(t):
    return None if t is None else t.detach().double().cpu()


def forward(x, gamma, beta, eps, residual=None, relu=False, relu_after_add=False):
    """dict of float64 tensors: mean, var, invstd, xh, z (the BatchNorm
    output) and y (after the fused ReLU / add)."""
    x = d(x)
    C = x.shape[-1]
    rows = x.reshape(-1, C)
    mean = rows.mean(0)
    var = ((rows - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * invstd
    z = xh
    if gamma is not None:
        z = z * d(gamma)
    if beta is not None:
        z = z + d(beta)
    y = z
    after = relu and relu_after_add and residual is not None
    if relu and not after:
        y = torch.relu(y)
    if residual is not None:
        y = y + d(residual)
    if after:
        y = torch.relu(y)
    return {"mean": mean, "var": var, "invstd": invstd, "xh": xh, "z": z, "y": y}


def moving(moving_mean, moving_var, fwd, decay):
    """The moving averages after one update from ``fwd``'s batch moments."""
    return (d(moving_mean) * decay + fwd["mean"] * (1 - decay),
            d(moving_var) * decay + fwd["var"] * (1 - decay))


def backward(fwd, dy, gamma, mask=None):
    """dict dx, dgamma, dbeta, dresidual from the gradient dy at y.  mask:
    where the fused ReLU passed (a bool tensor of y's shape; None: no ReLU).
    A caller that checks a float32 implementation hands in THAT forward's
    y > 0, once its y has met the bar: an element within rounding of zero has
    no defined side."""
    dz = d(dy)
    if mask is not None:
        dz = torch.where(mask.cpu(), dz, torch.zeros_like(dz))
    C = dz.shape[-1]
    xh = fwd["xh"]
    M = dz.numel() // C
    dbeta = dz.reshape(-1, C).sum(0)
    dgamma = (dz * xh).reshape(-1, C).sum(0)
    gi = fwd["invstd"] if gamma is None else d(gamma) * fwd["invstd"]
    dx = gi * (dz - dbeta / M - xh * (dgamma / M))
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "dresidual": dz}


def relu_mask(fwd, residual=None, relu=False, relu_after_add=False):
    """The float64 forward's own ReLU mask (None without a ReLU) and the
    quantity it thresholds."""
    if not relu:
        return None, None
    t = fwd["z"] + d(residual) if (relu_after_add and residual is not None) else fwd["z"]
    return t > 0, t


def close(got, want, what=""):
    """|got - want| <= BAR * max|want| (float64 compare), with the figures in
    the failure message."""
    got, want = d(got), d(want)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max())
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= BAR * scale, f"{what}: max err {err:.3g} > {BAR:g} * {scale:.3g}"
    return err, scale
