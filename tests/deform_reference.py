"""torch-on-CPU restatement of the reference's DeformConv2D
(lib/layers/convolutional.py:51-115 and :375-503), written from those lines
and independent of the package: what the HIP sampler and layers.DeformConv2D
are tested against.  Parity status: restatement + known-answer tests
(tests/test_deform_cpu.py), unpinned -- TensorFlow 1.x cannot run here, as
for ROIAlign.

Positions (the add, the clip, the floor, the corner clip) are always float32,
as in the reference graph; ``dtype`` is the precision of everything after
that.  float32 reproduces the reference arithmetic operation by operation
(the bit-exact forward); float64 with autograd gives the gradients TF
autodiff forms for the same graph: floor passes nothing, clip_by_value (like
torch.clamp) passes where the unclipped value lies in [0, Hp-1] inclusive,
the clipped corner floats are constants, the pad ring's gradient is dropped
by the pad's own gradient.
"""
import torch
import torch.nn.functional as F


def same_pads(k, rate=1):
    """fix_padding (convolutional.py:12-23): (pad_beg, pad_end) of SAME."""
    k_eff = k + (k - 1) * (rate - 1)
    total = k_eff - 1
    return total // 2, total - total // 2


def pads_of(k, rate, padding):
    return same_pads(k, rate) if (padding == "SAME" and k != 1) else (0, 0)


def out_size(size, k, stride, rate, pads):
    k_eff = k + (k - 1) * (rate - 1)
    return (size + pads[0] + pads[1] - k_eff) // stride + 1


def base_positions(OH, OW, k, stride, rate):
    """_get_sampling_indices (:51-67): integer (y, x) of tap t = kh*k + kw of
    output (oh, ow) on the padded grid, each [OH, OW, k*k]."""
    oh = torch.arange(OH).view(OH, 1, 1, 1)
    ow = torch.arange(OW).view(1, OW, 1, 1)
    kh = torch.arange(k).view(1, 1, k, 1)
    kw = torch.arange(k).view(1, 1, 1, k)
    y = (oh * stride + kh * rate).expand(OH, OW, k, k).reshape(OH, OW, k * k)
    x = (ow * stride + kw * rate).expand(OH, OW, k, k).reshape(OH, OW, k * k)
    return y, x


def deform_cols(x, offsets, k, stride=1, rate=1, padding="SAME", groups=1, dtype=torch.float32):
    """x [N,H,W,C], offsets [N,OH,OW,2*G*k*k] (channel (g*k*k + t)*2 + {dy, dx})
    -> cols [N,OH,OW,k*k*C], tap-major (:410-452 up to the last reshape, in the
    layout whose product with weights.reshape(k*k*C, Cout) is the k x k /
    stride-k VALID conv of :455-483)."""
    N, H, W, C = x.shape
    G, KK = groups, k * k
    Cg = C // G
    pb, pe = pads_of(k, rate, padding)
    Hp, Wp = H + pb + pe, W + pb + pe
    OH, OW = out_size(H, k, stride, rate, (pb, pe)), out_size(W, k, stride, rate, (pb, pe))
    assert offsets.shape == (N, OH, OW, 2 * G * KK), offsets.shape
    xp = F.pad(x.to(dtype), (0, 0, pb, pe, pb, pe)).reshape(N, Hp, Wp, G, Cg)
    off = offsets.reshape(N, OH, OW, G, KK, 2)
    by, bx = base_positions(OH, OW, k, stride, rate)
    by = by.view(1, OH, OW, 1, KK)
    bx = bx.view(1, OH, OW, 1, KK)
    # float32 positions decide the corners
    with torch.no_grad():
        o32 = off.detach().to(torch.float32)
        y32 = (by.to(torch.float32) + o32[..., 0]).clamp(0.0, float(Hp - 1))
        x32 = (bx.to(torch.float32) + o32[..., 1]).clamp(0.0, float(Wp - 1))
        y0 = torch.floor(y32).to(torch.int64)
        x0 = torch.floor(x32).to(torch.int64)
        y1, x1 = y0 + 1, x0 + 1
        y0, y1 = y0.clamp(0, Hp - 1), y1.clamp(0, Hp - 1)
        x0, x1 = x0.clamp(0, Wp - 1), x1.clamp(0, Wp - 1)
    # the same positions in the arithmetic dtype (identical values in float32)
    od = off.to(dtype)
    y = (by.to(dtype) + od[..., 0]).clamp(0.0, float(Hp - 1))
    xx = (bx.to(dtype) + od[..., 1]).clamp(0.0, float(Wp - 1))
    b = torch.arange(N).view(N, 1, 1, 1, 1).expand(N, OH, OW, G, KK)
    g = torch.arange(G).view(1, 1, 1, G, 1).expand(N, OH, OW, G, KK)
    p0, p1 = xp[b, y0, x0, g], xp[b, y0, x1, g]
    p2, p3 = xp[b, y1, x0, g], xp[b, y1, x1, g]
    fy0, fy1, fx0, fx1 = (t.to(dtype) for t in (y0, y1, x0, x1))
    w0 = ((fy1 - y) * (fx1 - xx)).unsqueeze(-1)
    w1 = ((fy1 - y) * (xx - fx0)).unsqueeze(-1)
    w2 = ((y - fy0) * (fx1 - xx)).unsqueeze(-1)
    w3 = ((y - fy0) * (xx - fx0)).unsqueeze(-1)
    pix = ((w0 * p0 + w1 * p1) + w2 * p2) + w3 * p3  # tf.add_n: left to right
    # [N,OH,OW,G,KK,Cg] -> [N,OH,OW,KK,G*Cg]
    return pix.permute(0, 1, 2, 4, 3, 5).reshape(N, OH, OW, KK * C)


def offset_conv(x, offset_weights, offset_bias, k, stride, rate, padding, dtype):
    """:376-406: VALID conv of the fix_padding'ed input, dilation = rate."""
    pb, pe = pads_of(k, rate, padding)
    xp = F.pad(x.to(dtype), (0, 0, pb, pe, pb, pe))
    y = F.conv2d(xp.permute(0, 3, 1, 2), offset_weights.to(dtype).permute(3, 2, 0, 1),
                 offset_bias.to(dtype), stride=stride, dilation=rate)
    return y.permute(0, 2, 3, 1)


def deform_conv(x, weights, bias, offset_weights, offset_bias, k, stride=1, rate=1,
                padding="SAME", groups=1, dtype=torch.float64):
    """The whole layer without normalizer / activation: [N,OH,OW,Cout]."""
    offsets = offset_conv(x, offset_weights, offset_bias, k, stride, rate, padding, dtype)
    cols = deform_cols(x, offsets, k, stride, rate, padding, groups, dtype)
    out = cols @ weights.to(dtype).reshape(-1, weights.shape[-1])
    return out if bias is None else out + bias.to(dtype)


def im2col(x, k, stride=1, rate=1, padding="SAME", shift=(0, 0)):
    """Plain im2col of the padded input in the same [N,OH,OW,k*k*C] layout by
    explicit slicing; ``shift`` moves every tap by whole pixels (dy, dx) and
    must keep every tap inside the padded grid."""
    N, H, W, C = x.shape
    pb, pe = pads_of(k, rate, padding)
    xp = F.pad(x, (0, 0, pb, pe, pb, pe))
    OH, OW = out_size(H, k, stride, rate, (pb, pe)), out_size(W, k, stride, rate, (pb, pe))
    taps = []
    for kh in range(k):
        for kw in range(k):
            ys = torch.arange(OH) * stride + kh * rate + shift[0]
            xs = torch.arange(OW) * stride + kw * rate + shift[1]
            assert 0 <= int(ys.min()) and int(ys.max()) < xp.shape[1]
            assert 0 <= int(xs.min()) and int(xs.max()) < xp.shape[2]
            taps.append(xp[:, ys][:, :, xs])
    return torch.stack(taps, 3).reshape(N, OH, OW, k * k * C)
