"""Tensor formulations of the C4 head's pieces, in the dtype and on the device
of their inputs: the crop (lib/layers/functional.py:100-166 on
tf.image.crop_and_resize), the res5 stage with its FrozenBN un-folded, and the
mask head.  Res5ROIHeads runs them for CPU tensors (tests, loss parity runs);
GPU tensors take the HIP kernels and never come here."""
import torch
import torch.nn.functional as F

from ...layers.convolutional import same_pads
from ...layers.ops import BOX_MODE_ALIGNED, BOX_MODE_RAW, BOX_MODE_UNALIGNED


def sample_positions(boxes, crop, size, scale=1.0, box_mode=BOX_MODE_ALIGNED, pad=True):
    """Sample coordinates (pos_y [R, ch], pos_x [R, cw]) of a crop on the map
    the taps index -- the 1-px SYMMETRIC-padded one with ``pad`` -- in the
    boxes' dtype, with the operations and their order of roi_geom / in_coord
    in csrc/roi_align.hip.  size: the un-padded (H, W)."""
    ch, cw = crop
    b = boxes if box_mode == BOX_MODE_RAW else boxes * scale
    Hp, Wp = (size[0] + 2, size[1] + 2) if pad else tuple(size)
    if pad:
        b = b + 1
    y1, x1, y2, x2 = b.unbind(1)
    if box_mode == BOX_MODE_ALIGNED:
        sh, sw = (y2 - y1) / ch, (x2 - x1) / cw
        y1, x1 = ((y1 + sh / 2) - 0.5) / (Hp - 1), ((x1 + sw / 2) - 0.5) / (Wp - 1)
        y2, x2 = y1 + (sh * (ch - 1)) / (Hp - 1), x1 + (sw * (cw - 1)) / (Wp - 1)
    elif box_mode == BOX_MODE_UNALIGNED:
        y1, y2, x1, x2 = y1 / Hp, y2 / Hp, x1 / Wp, x2 / Wp

    def axis(c1, c2, img, n):
        if n == 1:
            return (0.5 * (c1 + c2) * (img - 1))[:, None]
        step = ((c2 - c1) * (img - 1)) / (n - 1)
        i = torch.arange(n, dtype=boxes.dtype, device=boxes.device)
        return (c1 * (img - 1))[:, None] + i * step[:, None]

    return axis(y1, y2, Hp, ch), axis(x1, x2, Wp, cw)


def crop_and_resize_dense(feat, boxes, box_ind, crop, scale=1.0, box_mode=BOX_MODE_ALIGNED,
                          pad=True):
    """feat [N, H, W, C], boxes [R, 4] -> [R, ch, cw, C]: one bilinear sample
    per output element, 0 outside the (padded) map, differentiable w.r.t. feat
    (boxes carry no gradient, functional.py:120)."""
    N, H, W, C = feat.shape
    py, px = sample_positions(boxes.detach().to(feat.dtype), crop, (H, W), scale, box_mode, pad)
    d = 1 if pad else 0

    def taps(pos, img):
        ok = (pos >= 0) & (pos <= img + 2 * d - 1)
        lo = torch.floor(pos)
        r0 = (lo.long() - d).clamp(0, img - 1)
        r1 = (torch.ceil(pos).long() - d).clamp(0, img - 1)
        return ok, r0, r1, pos - lo

    oky, y0, y1, ly = taps(torch.nan_to_num(py), H)
    okx, x0, x1, lx = taps(torch.nan_to_num(px), W)
    n = box_ind.long()[:, None, None]
    g = lambda yy, xx: feat[n, yy[:, :, None], xx[:, None, :]]
    lx, ly = lx[:, None, :, None], ly[:, :, None, None]
    top = g(y0, x0) + (g(y0, x1) - g(y0, x0)) * lx
    bot = g(y1, x0) + (g(y1, x1) - g(y1, x0)) * lx
    out = top + (bot - top) * ly
    ok = (oky[:, :, None] & okx[:, None, :])[..., None]
    return torch.where(ok, out, torch.zeros_like(out))


def conv_dense(x, layer, stride=None):
    """Conv2D.call (lib/layers/convolutional.py:198-263): the explicit SAME
    pad, a VALID conv, the bias, the FrozenBN (x - mean) * gamma / sqrt(var +
    eps) + beta, the activation."""
    k, s = layer.kernel_size, layer.stride if stride is None else stride
    if layer.padding == "SAME" and k != 1:
        pb, pe = same_pads(k, layer.rate)
        x = F.pad(x, (0, 0, pb, pe, pb, pe))
    dt = x.dtype
    bias = layer.bias.to(dt) if layer.bias is not None else None
    y = F.conv2d(x.permute(0, 3, 1, 2), layer.weights.to(dt).permute(3, 2, 0, 1), bias, stride=s,
                 dilation=layer.rate, groups=layer.num_groups).permute(0, 2, 3, 1)
    bn = layer.normalizer_fn
    if bn is not None:
        if not hasattr(bn, "moving_variance"):
            raise NotImplementedError(f"{layer.scope}: only FrozenBN has a tensor formulation here")
        if getattr(bn, "batch_stats", False):
            raise NotImplementedError(f"{layer.scope}: a BatchNorm on batch statistics has no "
                                      "tensor formulation here (only the inference form)")
        y = ((y - bn.moving_mean.to(dt)) * (bn.gamma.to(dt) / torch.sqrt(
            bn.moving_variance.to(dt) + bn.epsilon)) + bn.beta.to(dt))
    return layer.act_fn(y) if layer.act_fn is not None else y


def stage_dense(stage, x, first_stride=None):
    """Stage of BottleneckBlocks (lib/modeling/backbone/resnet.py): relu(conv3(
    conv2(conv1(x))) + shortcut(x)).  first_stride: the stride the first
    block's strided convs run at instead of their own."""
    for i, blk in enumerate(stage.blocks):
        over = lambda c: first_stride if (i == 0 and first_stride is not None
                                          and c.stride > 1) else None
        sc = conv_dense(x, blk.shortcut, over(blk.shortcut)) if blk.shortcut is not None else x
        h = conv_dense(x, blk.conv1, over(blk.conv1))
        h = conv_dense(h, blk.conv2, over(blk.conv2))
        x = torch.relu(conv_dense(h, blk.conv3) + sc)
    return x


def mask_head_dense(head, x):
    """MaskRCNNConvUpsampleHead.call: (deconv features, mask logits)."""
    for c in head.convs:
        x = conv_dense(x, c)
    dc = head.deconv
    dt = x.dtype
    y = F.conv_transpose2d(x.permute(0, 3, 1, 2), dc.weights.to(dt).permute(3, 2, 0, 1),
                           dc.bias.to(dt) if dc.bias is not None else None, stride=dc.stride)
    if dc.kernel_size != dc.stride or dc.normalizer_fn is not None:
        raise NotImplementedError("mask_head_dense: the 2x2 / stride-2 deconv without a normalizer")
    y = y.permute(0, 2, 3, 1)
    y = dc.act_fn(y) if dc.act_fn is not None else y
    return y, conv_dense(y, head.predictor)
