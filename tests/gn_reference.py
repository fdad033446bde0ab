"""Float64 restatement of GroupNorm on NHWC with its gradient
(lib/layers/normalization.py:174-260: tf.nn.moments over (H, W, the group's
channels), then tf.nn.batch_normalization), plain torch float64 on the same
float32 inputs.  For x [N, H, W, C] with G groups, m = H * W * C / G:

    mean, var (biased) per (n, g); r = rsqrt(var + eps); xh = (x - mean) * r
    z = xh * gamma + beta; y = z | relu(z)
    dbeta_c = sum_{n,hw} dz, dgamma_c = sum_{n,hw} dz * xh
    S1 = sum_{hw, c in g} dz * gamma_c, S2 = sum_{hw, c in g} dz * gamma_c * xh
    dx = r * (dz * gamma_c - S1 / m - xh * S2 / m)

The bar and the compare are BatchNorm's (bn_reference.close / BAR).
"""
import torch

from bn_reference import BAR, close, d  # noqa: F401


def _per_group(t, G):
    """[N, H, W, C] -> [N, H*W, G, C/G]."""
    N, H, W, C = t.shape
    return t.reshape(N, H * W, G, C // G)


def forward(x, G, gamma, beta, eps, relu=False):
    """dict of float64 tensors: mean, var [N, G]; r [N, G]; xh, z, y [N, H, W, C]."""
    x = d(x)
    xg = _per_group(x, G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    r = 1.0 / torch.sqrt(var + eps)
    xh = ((xg - mean[:, None, :, None]) * r[:, None, :, None]).reshape(x.shape)
    z = xh * d(gamma) + d(beta)
    y = torch.relu(z) if relu else z
    return {"mean": mean, "var": var, "r": r, "xh": xh, "z": z, "y": y, "G": G}


def backward(fwd, dy, gamma, mask=None):
    """dict dx, dgamma, dbeta from the gradient dy at y.  mask: where the fused
    ReLU passed (bool, y's shape; None: no ReLU).  A caller that checks a
    float32 implementation hands in THAT forward's y > 0, once its y has met
    the bar: an element within rounding of zero has no defined side."""
    dz = d(dy)
    if mask is not None:
        dz = torch.where(mask.cpu(), dz, torch.zeros_like(dz))
    G, xh, r = fwd["G"], fwd["xh"], fwd["r"]
    N, H, W, C = dz.shape
    m = H * W * (C // G)
    dbeta = dz.reshape(-1, C).sum(0)
    dgamma = (dz * xh).reshape(-1, C).sum(0)
    dzg = dz * d(gamma)
    S1 = _per_group(dzg, G).sum(dim=(1, 3))
    S2 = _per_group(dzg * xh, G).sum(dim=(1, 3))
    inner = _per_group(dzg, G) - (S1 / m)[:, None, :, None] \
        - _per_group(xh, G) * (S2 / m)[:, None, :, None]
    dx = (inner * r[:, None, :, None]).reshape(dz.shape)
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}
