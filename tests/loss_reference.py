"""Float64 restatement of the RPN, Fast R-CNN, mask and RetinaNet training
losses, written from the reference's formulas (lib/layers/loss.py,
lib/modeling/box_regression.py:38-74, rpn_outputs.py:306-401,
fast_rcnn.py:269-357, mask_head.py:17-68, retinanet.py:147-210) in plain
torch on the CPU, differentiable, with ``dtype`` a parameter so that the same
text runs in float32 (its error against float64 is the float32 error of the
formulas themselves: tests/test_gpu_losses.py sizes its bounds from it).

Rows that do not count are REMOVED by boolean indexing, as the reference's
boolean_mask / SparseBoxList removes them -- never masked with ``where`` --
so whatever an excluded row holds (NaN, a zero-area box) cannot reach a loss
or a gradient.  No GPU code is imported here.

gamma in (0, 1) is out of scope for the focal loss: gamma q^(gamma - 1) * 0
is NaN once q = 1 - p_t rounds to 0, in TF's autodiff, in torch's and in the
kernel alike, and no shipped config uses such a gamma.

The case builders (``CASES``) are seeded and deterministic and return
float32 tensors; tests/test_loss_reference_cpu.py checks that each case has
the property it is named for.
"""
import math

import torch

UPSTREAM = (0.7, 1.3)  # distinct upstream gradients, neither 1
F32 = torch.float32
F64 = torch.float64


class Losses(tuple):
    """The losses of one call (0-d tensors) and the input leaves they were
    computed from (``leaves``, in ``dtype``, at the full input shapes)."""

    def __new__(cls, losses, leaves):
        self = super().__new__(cls, losses)
        self.leaves = tuple(leaves)
        return self


def _leaf(x, dtype):
    return x.detach().to(dtype).requires_grad_(True)


# ------------------------------------------------------------ element formulas
def get_deltas(src, tgt, weights):
    """Box2BoxTransform.get_deltas (box_regression.py:38-74); boxes (y0, x0,
    y1, x1), result (dy, dx, dh, dw) times the weights."""
    sh, sw = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scy, scx = src[:, 0] + 0.5 * sh, src[:, 1] + 0.5 * sw
    th, tw = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tcy, tcx = tgt[:, 0] + 0.5 * th, tgt[:, 1] + 0.5 * tw
    wy, wx, wh, ww = weights
    return torch.stack([wy * (tcy - scy) / sh, wx * (tcx - scx) / sw,
                        wh * torch.log(th / sh), ww * torch.log(tw / sw)], 1)


def smooth_l1(labels, predictions, beta):
    """smooth_l1_loss (loss.py:9-58), reduction 'none'."""
    n = (labels - predictions).abs()
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def sigmoid_ce(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log(1 + exp(-|x|))."""
    return x.clamp(min=0) - x * z + torch.log1p(torch.exp(-x.abs()))


def focal(x, t, alpha, gamma):
    """sigmoid_focal_loss (loss.py:59-101), reduction 'none'."""
    p = torch.sigmoid(x)
    ce = sigmoid_ce(x, t)
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * (1 - p_t) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


# ------------------------------------------------------------------ the losses
def rpn(logits, deltas, anchors, gt, matches, pos, sampled, weights, beta, dtype=F64):
    """(cls_sum, loc_sum) of RPNOutputs.losses before the normaliser
    (rpn_outputs.py:135-185, :306-401): sigmoid CE of the sampled anchors
    against [anchor is positive], smooth-L1 of the positive anchors' deltas
    against get_deltas(anchor, matched GT).  logits [N, P], deltas [N, P, 4],
    anchors [P, 4], gt [N, G, 4], matches [N, P], pos / sampled [N, P]."""
    lg, dl = _leaf(logits, dtype), _leaf(deltas, dtype)
    pos, sampled = pos.bool(), sampled.bool()
    cls = sigmoid_ce(lg[sampled], pos[sampled].to(dtype)).sum()
    n_idx, p_idx = torch.nonzero(pos, as_tuple=True)
    src = anchors.to(dtype)[p_idx]
    tgt = gt.to(dtype)[n_idx, matches.long()[n_idx, p_idx]]
    loc = smooth_l1(get_deltas(src, tgt, weights), dl[n_idx, p_idx], beta).sum()
    return Losses((cls, loc), (lg, dl))


def fast_rcnn(logits, deltas, proposals, gt_classes, gt_boxes, valid, weights, beta, dtype=F64):
    """(loss_cls, loss_box_reg) of FastRCNNOutputs.losses (fast_rcnn.py:269-357)
    over the valid rows, both / max(1, #valid): softmax CE against the GT class
    (K = background), smooth-L1 of the foreground rows' GT-class deltas (column
    0 when class-agnostic).  logits [B, K + 1], deltas [B, nreg * 4]."""
    B, K1 = logits.shape
    K, nreg = K1 - 1, deltas.shape[1] // 4
    lg, dl = _leaf(logits, dtype), _leaf(deltas, dtype)
    valid = valid.bool()
    rows = torch.nonzero(valid)[:, 0]
    c = gt_classes.long()[rows]
    R = max(1, int(rows.numel()))
    x = lg[rows]
    ce = torch.logsumexp(x, 1) - x[torch.arange(rows.numel()), c]
    loss_cls = ce.sum() / R
    keep = (c >= 0) & (c < K)
    fr, fc = rows[keep], c[keep]
    col = torch.zeros_like(fc) if nreg == 1 else fc
    pred = dl.reshape(B, nreg, 4)[fr, col]
    tgt = get_deltas(proposals.to(dtype)[fr], gt_boxes.to(dtype)[fr], weights)
    loss_box = smooth_l1(tgt, pred, beta).sum() / R
    return Losses((loss_cls, loss_box), (lg, dl))


def mask(logits, target, classes, fg, dtype=F64):
    """mask_rcnn_loss (mask_head.py:17-68) given the rounded targets: the mean
    sigmoid CE of each foreground row's class channel (clamped to [0, C - 1];
    channel 0 when C == 1) over fg x Hm x Wm; 0 with no foreground.  logits
    [B, Hm, Wm, C], target [B, Hm, Wm]."""
    C = logits.shape[3]
    lg = _leaf(logits, dtype)
    rows = torch.nonzero(fg.bool())[:, 0]
    if rows.numel() == 0:
        return Losses((lg.sum() * 0,), (lg,))
    c = torch.zeros_like(rows) if C == 1 else classes.long()[rows].clamp(0, C - 1)
    x = lg[rows, :, :, c]
    return Losses((sigmoid_ce(x, target.to(dtype)[rows]).mean(),), (lg,))


def retina(cls_levels, box_levels, anchors, gt, gt_classes, matches, labels, K, A, alpha, gamma,
           beta, weights, dtype=F64):
    """(focal sum, smooth-L1 sum) of RetinaNet.losses before the normaliser
    (retinanet.py:147-210): the levels reshaped to [N, HWA, K] / [N, HWA, 4]
    and concatenated in (level, h, w, a) order; focal loss "sum" over the
    anchors with label >= 0 against one_hot(class)[:K] (background: all zero),
    smooth-L1 "sum" over the label == 1 anchors against get_deltas(anchor,
    matched GT).  Leaves: every class level, then every box level."""
    N = cls_levels[0].shape[0]
    cl = [_leaf(c, dtype) for c in cls_levels]
    bl = [_leaf(b, dtype) for b in box_levels]
    x = torch.cat([c.reshape(N, -1, K) for c in cl], 1)
    d = torch.cat([b.reshape(N, -1, 4) for b in bl], 1)
    assert x.shape[1] == anchors.shape[0] == labels.shape[1] and A >= 1
    labels, matches = labels.long(), matches.long()
    vn, vr = torch.nonzero(labels >= 0, as_tuple=True)
    fn, fr = torch.nonzero(labels == 1, as_tuple=True)
    t = torch.zeros((vn.numel(), K), dtype=dtype)
    is_fg = labels[vn, vr] == 1
    t[torch.nonzero(is_fg)[:, 0], gt_classes.long()[fn, matches[fn, fr]]] = 1
    cls_sum = focal(x[vn, vr], t, alpha, gamma).sum()
    tgt = get_deltas(anchors.to(dtype)[fr], gt.to(dtype)[fn, matches[fn, fr]], weights)
    box_sum = smooth_l1(tgt, d[fn, fr], beta).sum()
    return Losses((cls_sum, box_sum), tuple(cl) + tuple(bl))


def gradients(outputs, upstream=UPSTREAM):
    """d(sum_i upstream[i] * outputs[i]) / d(every leaf), at the full input
    shapes: autograd scatters through the boolean indexing, so every element
    of a removed row is exactly 0."""
    total = sum(u * l for u, l in zip(upstream, outputs))
    grads = torch.autograd.grad(total, outputs.leaves, allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(grads, outputs.leaves)]


# ---------------------------------------------------------------- case builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _boxes(g, n, height, width, lo=8.0, hi=100.0):
    cy, cx = torch.rand(n, generator=g) * height, torch.rand(n, generator=g) * width
    hh = torch.rand(n, generator=g) * (hi - lo) + lo
    ww = torch.rand(n, generator=g) * (hi - lo) + lo
    return torch.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2], 1)


def _jitter(g, boxes, sigma):
    out = boxes + torch.randn(boxes.shape, generator=g) * sigma
    out[..., 2:] = torch.maximum(out[..., 2:], out[..., :2] + 2)
    return out


def case(kernel, args, conf, **extra):
    return dict(kernel=kernel, args=tuple(args), conf=tuple(conf), **extra)


W1, W10 = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
SAT = (90.0, -90.0, 104.0, -104.0)  # expf overflows past 88.7


# RPN ---------------------------------------------------------------------
def rpn_case(seed, N, P, G, beta=1.0 / 9, weights=W1, pos_frac=0.1, samp_frac=0.1, mode=None):
    g = _gen(seed)
    anchors = _boxes(g, P, 500, 700)
    gt = _jitter(g, anchors[torch.randint(0, P, (N * G,), generator=g)].reshape(N, G, 4), 3.0)
    matches = torch.randint(0, G, (N, P), generator=g)
    pos = torch.rand(N, P, generator=g) < pos_frac
    pos[:, 0] = True
    extra = torch.rand(N, P, generator=g) < samp_frac
    sampled = pos | extra
    logits = torch.randn(N, P, generator=g) * 3
    deltas = torch.randn(N, P, 4, generator=g) * 0.3
    if mode == "no_pos":
        pos[:] = False
        sampled = extra
    elif mode == "no_sampled":
        sampled = torch.zeros_like(pos)
    elif mode == "independent":
        sampled = extra
    elif mode == "saturated":
        i = torch.arange(P)
        logits = torch.tensor(SAT)[i % 4].repeat(N, 1)
        pos = ((i // 4) % 2 == 1).repeat(N, 1)
        sampled = torch.ones_like(pos)
    return case("rpn", (logits, deltas, anchors, gt, matches, pos, sampled), (weights, beta))


# Fast R-CNN ----------------------------------------------------------------
def frcn_case(seed, B, K1, nreg, beta=0.5, weights=W10, mode=None):
    g = _gen(seed)
    K = K1 - 1
    props = _boxes(g, B, 700, 1200, 8.0, 200.0)
    gtb = _jitter(g, props, 6.0)
    cls = torch.randint(0, K1, (B,), generator=g)
    valid = torch.rand(B, generator=g) < 0.85
    logits = torch.randn(B, K1, generator=g) * 3
    deltas = torch.randn(B, nreg * 4, generator=g) * 0.5
    if B <= 16:  # small cases: foreground, background and padding all present
        valid[:] = True
        cls[0] = min(2, K - 1)
        if B > 1:
            cls[1] = K
        if B > 2:
            valid[2] = False
    if mode == "no_valid":
        valid[:] = False
    elif mode == "no_fg":
        cls[:] = K
    elif mode == "saturated":
        valid[:] = True
        cls = torch.tensor([3, 3, 3, 3, 80, 80, 0, 79])
        for r in range(8):
            kind, c = r % 4, int(cls[r])
            if kind == 0:
                logits[r, c] = 1e4
            elif kind == 1:
                logits[r, (c + 7) % K1] = 1e4
            elif kind == 2:
                logits[r, c] = -1e4
            else:
                logits[r] = 1.25
    elif mode == "dirty":
        nan = float("nan")
        valid = torch.tensor([True, True, False, True] * 4)
        cls = torch.tensor([5, K, 7, 79] * 4)
        bad = ~valid
        logits[bad], deltas[bad], props[bad], gtb[bad] = nan, nan, nan, nan
        cls[bad] = -7
        bg = valid & (cls == K)
        props[bg, 2:] = props[bg, :2]   # zero-area proposals and GT boxes
        gtb[bg] = 0.0
    return case("frcn", (logits, deltas, props, cls, gtb, valid), (weights, beta))


def nextafter32(x, up):
    x = torch.tensor(x, dtype=F32)
    return float(torch.nextafter(x, torch.tensor(math.inf if up else -math.inf, dtype=F32)))


def frcn_kink(beta):
    """Proposal == GT box, so every target is exactly 0 and the prediction is
    t - p up to sign: the 48 foreground slots cycle through 0, +-beta,
    +-nextafter(beta) (both directions) and +-beta / 2, beta rounded to
    float32 as the kernel receives it."""
    B, K, nreg = 12, 4, 4
    c = frcn_case(31, B, K + 1, nreg, beta=beta)
    logits, deltas, props, cls, gtb, valid = c["args"]
    valid = torch.ones(B, dtype=torch.bool)
    cls = torch.arange(B) % K
    b32 = float(torch.tensor(beta, dtype=F32))
    up, dn = nextafter32(b32, True), nextafter32(b32, False)
    vals = torch.tensor([0.0, b32, -b32, up, -up, dn, -dn, b32 / 2, -b32 / 2], dtype=F32)
    d = deltas.reshape(B, nreg, 4).clone()
    d[torch.arange(B), cls] = vals[torch.arange(B * 4) % len(vals)].reshape(B, 4)
    return case("frcn", (logits, d.reshape(B, nreg * 4), props, cls, props.clone(), valid),
                (W10, beta))


# mask ------------------------------------------------------------------------
def mask_case(seed, B, Hm, Wm, C, mode=None):
    g = _gen(seed)
    logits = torch.randn(B, Hm, Wm, C, generator=g) * 2
    target = (torch.rand(B, Hm, Wm, generator=g) < 0.5).float()
    classes = torch.randint(0, C, (B,), generator=g)
    fg = torch.rand(B, generator=g) < 0.6
    fg[0], fg[B - 1] = True, False
    if mode == "quad":          # every slot of one float4
        classes = torch.arange(B) % 4
        fg[:] = True
        fg[B - 1] = False
    elif mode == "ends":        # the first and the last channel
        classes = torch.where(torch.arange(B) % 2 == 0, 0, C - 1)
        fg[1] = True
    elif mode == "agnostic":    # C == 1: the class is ignored, in range or not
        classes = torch.tensor([0, 57, -3, 1, 80])[torch.arange(B) % 5]
        fg[:B - 1] = True
    elif mode == "no_fg":
        fg[:] = False
    elif mode == "all_fg":
        fg[:] = True
    elif mode == "saturated":
        fg[:] = True
        classes = torch.arange(B) % C
        i = torch.arange(Hm * Wm)
        logits[torch.arange(B), :, :, classes] = torch.tensor(SAT)[i % 4].reshape(Hm, Wm)
        target = ((i // 4) % 2 == 1).float().reshape(Hm, Wm).repeat(B, 1, 1)
    elif mode == "dirty":
        fg = torch.arange(B) % 2 == 0
        logits[~fg] = float("nan")
        classes[~fg] = -1
    return case("mask", (logits, target, classes, fg), ())


# RetinaNet -----------------------------------------------------------------
def retina_anchors(grids, strides, A):
    """(level, h, w, a) order; A of the 9 (scale, ratio) cell anchors."""
    out = []
    for (H, W), s in zip(grids, strides):
        ys = (torch.arange(H, dtype=F32) + 0.5) * s
        xs = (torch.arange(W, dtype=F32) + 0.5) * s
        cell = []
        for a in range(A):
            size = 4.0 * s * 2 ** ((a % 3) / 3.0)
            ratio = (0.5, 1.0, 2.0)[(a // 3) % 3]
            h, w = size * math.sqrt(ratio), size / math.sqrt(ratio)
            cell.append([-h / 2, -w / 2, h / 2, w / 2])
        cell = torch.tensor(cell, dtype=F32)
        ctr = torch.stack(torch.meshgrid(ys, xs, indexing="ij"), -1).reshape(-1, 1, 2)
        out.append((ctr.repeat(1, 1, 2) + cell[None]).reshape(-1, 4))
    return torch.cat(out)


def _iou(a, b):
    ih = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    iw = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = ih * iw
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])  # noqa: E731
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def retina_case(seed, grids, strides, A, K, N, G, alpha=0.25, gamma=2.0, beta=0.1, weights=W1,
                mode=None, classes=None):
    g = _gen(seed)
    H, W = grids[0][0] * strides[0], grids[0][1] * strides[0]
    anchors = retina_anchors(grids, strides, A)
    R = anchors.shape[0]
    gt = torch.stack([_boxes(g, G, H, W, 16.0, 0.8 * min(H, W)) for _ in range(N)])
    gcls = torch.randint(0, K, (N, G), generator=g)
    if classes is not None:
        gcls[0, :len(classes)] = torch.tensor(classes)
    matches = torch.zeros((N, R), dtype=torch.int64)
    labels = torch.zeros((N, R), dtype=torch.int64)
    for n in range(N):  # IoU >= 0.5 fg, < 0.4 bg, else ignored; each GT's best anchor fg
        iou = _iou(gt[n], anchors)
        best, matches[n] = iou.max(0)
        labels[n] = torch.where(best >= 0.5, 1, torch.where(best < 0.4, 0, -1))
        top = iou.argmax(1)
        labels[n, top] = 1
        matches[n, top] = torch.arange(G)
    cls = [torch.randn(N, h, w, A * K, generator=g) * 1.5 - 3 for h, w in grids]
    box = [torch.randn(N, h, w, A * 4, generator=g) * 0.3 for h, w in grids]
    if mode == "all_ignored":
        labels[:] = -1
    elif mode == "no_fg":
        labels[labels == 1] = -1
    elif mode == "saturated":
        assert len(grids) == 1
        sat = torch.tensor([30.0, -30.0, 90.0, -90.0, 104.0, -104.0])
        gcls[gcls == 1] = 0                     # class 1 is nobody's GT class
        x = cls[0].reshape(N, R, K)
        fn, fr = torch.nonzero(labels == 1, as_tuple=True)
        x[fn, fr, gcls[fn, matches[fn, fr]]] = sat[torch.arange(fn.numel()) % 6]
        r = torch.arange(0, R, 3)
        x[:, r, 1] = sat[(r // 3) % 6]          # a target-0 element of every third anchor
        cls = [x.reshape(cls[0].shape)]
    return case("retina", (cls, box, anchors, gt, gcls, matches, labels),
                (K, A, alpha, gamma, beta, weights))


_ONE_LEVEL = dict(grids=[(8, 10)], strides=[8], A=9, K=8, N=2, G=4)
_PYRAMID = dict(grids=[(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)], strides=[8, 16, 32, 64, 128],
                A=9, K=80, N=2, G=7)
_TINY_TOP = dict(grids=[(8, 8), (4, 4), (2, 2), (1, 1), (1, 1)], strides=[8, 16, 32, 64, 128],
                 A=9, K=8, N=2, G=4)


def _beta_id(b):
    return {0.0: "b0", 0.5: "b0.5", 0.1: "b0.1", 1.0: "b1", 1.0 / 9: "b1_9"}[b]


def _cases():
    c = {}
    # Fast R-CNN (beta 0 is the shipped heads' value)
    c["frcn/one_row"] = lambda: frcn_case(1, 1, 81, 80)
    c["frcn/ragged_rows"] = lambda: frcn_case(2, 5, 21, 20, beta=0.0)
    c["frcn/k1"] = lambda: frcn_case(3, 7, 2, 1)
    c["frcn/lane_edge-64"] = lambda: frcn_case(4, 7, 64, 63)
    c["frcn/lane_edge-65"] = lambda: frcn_case(5, 7, 65, 64, beta=0.0)
    c["frcn/three_passes"] = lambda: frcn_case(6, 6, 129, 1)
    c["frcn/coco-80"] = lambda: frcn_case(7, 1027, 81, 80, beta=0.0)
    c["frcn/coco-1"] = lambda: frcn_case(8, 1027, 81, 1)
    c["frcn/no_valid"] = lambda: frcn_case(9, 9, 81, 80, mode="no_valid")
    c["frcn/no_fg"] = lambda: frcn_case(10, 9, 81, 80, mode="no_fg")
    c["frcn/saturated"] = lambda: frcn_case(11, 8, 81, 80, mode="saturated")
    for b in (0.0, 0.5, 1.0 / 9):
        c[f"frcn/kink-{_beta_id(b)}"] = lambda b=b: frcn_kink(b)
    c["frcn/dirty_padding"] = lambda: frcn_case(12, 16, 81, 80, mode="dirty")
    # RPN
    c["rpn/tiny"] = lambda: rpn_case(1, 1, 1, 1)
    c["rpn/sub_wave"] = lambda: rpn_case(2, 1, 63, 3)
    c["rpn/block_edge"] = lambda: rpn_case(3, 2, 257, 3, beta=0.0)
    c["rpn/fwd_stride"] = lambda: rpn_case(4, 2, 65536 + 257, 6, pos_frac=0.02, samp_frac=0.05)
    c["rpn/bwd_stride"] = lambda: rpn_case(5, 1, 524288 + 301, 3, pos_frac=0.005, samp_frac=0.02)
    c["rpn/no_pos"] = lambda: rpn_case(6, 2, 300, 4, mode="no_pos")
    c["rpn/no_sampled"] = lambda: rpn_case(7, 2, 300, 4, mode="no_sampled")
    c["rpn/independent_masks"] = lambda: rpn_case(8, 2, 5000, 100, pos_frac=0.05, samp_frac=0.05,
                                                  mode="independent")
    c["rpn/saturated"] = lambda: rpn_case(9, 1, 512, 2, mode="saturated")
    for wn, w in (("w1", W1), ("w10", W10)):
        for b in (0.0, 1.0 / 9, 1.0):
            c[f"rpn/weights_beta-{wn}-{_beta_id(b)}"] = \
                lambda w=w, b=b: rpn_case(10, 2, 300, 4, beta=b, weights=w)
    # mask
    c["mask/small_map"] = lambda: mask_case(1, 5, 7, 7, 4, mode="quad")
    c["mask/wave_edge"] = lambda: mask_case(2, 3, 8, 8, 80)
    c["mask/scalar_c3"] = lambda: mask_case(3, 6, 14, 14, 3, mode="ends")
    c["mask/agnostic"] = lambda: mask_case(4, 5, 28, 28, 1, mode="agnostic")
    c["mask/cap_vec4"] = lambda: mask_case(5, 140, 28, 28, 80)
    c["mask/cap_scalar"] = lambda: mask_case(6, 900, 28, 28, 3)
    c["mask/no_fg"] = lambda: mask_case(7, 8, 28, 28, 80, mode="no_fg")
    c["mask/all_fg"] = lambda: mask_case(8, 8, 28, 28, 80, mode="all_fg")
    c["mask/saturated"] = lambda: mask_case(9, 4, 8, 8, 4, mode="saturated")
    c["mask/dirty_rows"] = lambda: mask_case(10, 8, 14, 14, 80, mode="dirty")
    # RetinaNet
    c["retina/one_cell"] = lambda: retina_case(1, [(1, 1)], [32], 1, 4, 1, 1, classes=[2])
    c["retina/single_level"] = lambda: retina_case(2, **_ONE_LEVEL)
    c["retina/pyramid"] = lambda: retina_case(3, **_PYRAMID, classes=[0, 3, 4, 79])
    c["retina/tiny_top_level"] = lambda: retina_case(4, **_TINY_TOP)
    c["retina/all_ignored"] = lambda: retina_case(2, **_ONE_LEVEL, mode="all_ignored")
    c["retina/no_fg"] = lambda: retina_case(2, **_ONE_LEVEL, mode="no_fg")
    for an, (a, gm) in (("a0.25-g2", (0.25, 2.0)), ("a-1-g2", (-1.0, 2.0)),
                        ("a0.25-g0", (0.25, 0.0)), ("a0.25-g1.5", (0.25, 1.5))):
        for b in (0.1, 0.0):
            c[f"retina/alpha_gamma-{an}-{_beta_id(b)}"] = \
                lambda a=a, gm=gm, b=b: retina_case(5, **_ONE_LEVEL, alpha=a, gamma=gm, beta=b)
    c["retina/saturated"] = lambda: retina_case(6, **_ONE_LEVEL, mode="saturated")
    return c


CASES = _cases()
FUNCS = {"rpn": rpn, "frcn": fast_rcnn, "mask": mask, "retina": retina}


def names(kernel):
    return [n for n in CASES if n.startswith(kernel + "/")]


def run(c, dtype=F64):
    """The restatement on a built case."""
    return FUNCS[c["kernel"]](*c["args"], *c["conf"], dtype=dtype)


def counted_deltas(c):
    """|t - p| in float64 of every element the smooth-L1 of a case counts."""
    k, a = c["kernel"], c["args"]
    if k == "rpn":
        logits, deltas, anchors, gt, matches, pos, _ = a
        n, p = torch.nonzero(pos.bool(), as_tuple=True)
        t = get_deltas(anchors.double()[p], gt.double()[n, matches[n, p]], c["conf"][0])
        return (t - deltas.double()[n, p]).abs()
    if k == "frcn":
        logits, deltas, props, cls, gtb, valid = a
        K, nreg = logits.shape[1] - 1, deltas.shape[1] // 4
        r = torch.nonzero(valid.bool() & (cls >= 0) & (cls < K))[:, 0]
        col = cls[r] if nreg > 1 else torch.zeros_like(r)
        t = get_deltas(props.double()[r], gtb.double()[r], c["conf"][0])
        return (t - deltas.double().reshape(-1, nreg, 4)[r, col]).abs()
    if k == "retina":
        cls, box, anchors, gt, gcls, matches, labels = a
        N = box[0].shape[0]
        d = torch.cat([b.double().reshape(N, -1, 4) for b in box], 1)
        n, r = torch.nonzero(labels == 1, as_tuple=True)
        t = get_deltas(anchors.double()[r], gt.double()[n, matches[n, r]], c["conf"][5])
        return (t - d[n, r]).abs()
    raise ValueError(k)


def counted_masks(c):
    """Per leaf, the elements a loss reaches."""
    k, a = c["kernel"], c["args"]
    if k == "rpn":
        pos, sampled = a[5].bool(), a[6].bool()
        return [sampled, pos[..., None].expand(-1, -1, 4)]
    if k == "frcn":
        logits, deltas, _, cls, _, valid = a
        B, K1 = logits.shape
        nreg = deltas.shape[1] // 4
        fg = valid.bool() & (cls >= 0) & (cls < K1 - 1)
        m = torch.zeros(B, nreg, 4, dtype=torch.bool)
        r = torch.nonzero(fg)[:, 0]
        m[r, cls[r] if nreg > 1 else torch.zeros_like(r)] = True
        return [valid.bool()[:, None].expand(B, K1), m.reshape(B, nreg * 4)]
    if k == "mask":
        logits, _, classes, fg = a
        B, Hm, Wm, C = logits.shape
        m = torch.zeros(B, Hm, Wm, C, dtype=torch.bool)
        r = torch.nonzero(fg.bool())[:, 0]
        m[r, :, :, classes[r].clamp(0, C - 1) if C > 1 else torch.zeros_like(r)] = True
        return [m]
    cls, box, _, _, _, _, labels = a
    K, A = c["conf"][:2]
    out, r0 = [], 0
    for x in cls:
        N, H, W, _ = x.shape
        n = H * W * A
        lab = labels[:, r0:r0 + n].reshape(N, H, W, A, 1)
        out.append((lab >= 0).expand(-1, -1, -1, -1, K).reshape(x.shape))
        r0 += n
    r0 = 0
    for x in box:
        N, H, W, _ = x.shape
        n = H * W * A
        lab = labels[:, r0:r0 + n].reshape(N, H, W, A, 1)
        out.append((lab == 1).expand(-1, -1, -1, -1, 4).reshape(x.shape))
        r0 += n
    return out


def cleaned(c):
    """A dirty case (frcn/dirty_padding, mask/dirty_rows) with what its
    excluded rows hold -- NaN, zero-area boxes, class -1 -- replaced by
    ordinary numbers, in the same layout: nothing that counts changes."""
    if c["kernel"] == "frcn":
        logits, deltas, props, cls, gtb, valid = (x.clone() for x in c["args"])
        bad = ~valid.bool()
        bg = valid.bool() & (cls == logits.shape[1] - 1)
        logits[bad], deltas[bad] = 1.0, 1.0
        cls[bad] = 0
        props[bad | bg] = torch.tensor([0.0, 0.0, 8.0, 8.0])
        gtb[bad | bg] = torch.tensor([1.0, 1.0, 9.0, 12.0])
        return dict(c, args=(logits, deltas, props, cls, gtb, valid))
    logits, target, classes, fg = (x.clone() for x in c["args"])
    logits[~fg.bool()] = 0.5
    classes[~fg.bool()] = 0
    return dict(c, args=(logits, target, classes, fg))


def case_beta(c):
    """The smooth-L1 beta of a case; None for the mask loss, which has none."""
    if c["kernel"] == "mask":
        return None
    return c["conf"][4] if c["kernel"] == "retina" else c["conf"][1]
