"""YOLOv4 inference restated from the oracle's pieces, numpy, float32
(lib/modeling/single_stage_heads/yolov4_outputs.py:208-264 _get_predictions,
:331-390 inference; lib/modeling/necks/yolov4.py:171-182 SPP):

  oracle.sigmoid -> the decode, term by term -> conf * prob -> max / argmax
  -> score > thresh in prediction order -> oracle.nms (class-agnostic) ->
  gather -> zero padding.

Python scalars enter as the reference's do: scale_yx and 0.5 * (scale_yx - 1)
are formed in double and rounded to float32 where they meet a tensor.
"""
import numpy as np

import oracle

F32 = np.float32


def predictions(logits, strides, cell_hw, scale_yx, num_classes):
    """logits[l] [N, H, W, A * (5 + K)]; cell_hw[l] [A, 2] the (h, w) of the
    [0, 0, h, w] cell anchors.  Returns boxes [N, P, 4], conf [N, P], score
    [N, P], cls [N, P] (int32, lowest index at the maximum) and prob
    [N, P, K], level-major."""
    K = int(num_classes)
    boxes, conf, prob = [], [], []
    for x, stride, cell, s in zip(logits, strides, cell_hw, scale_yx):
        x = np.asarray(x, F32)
        N, H, W, _ = x.shape
        cell = np.asarray(cell, F32).reshape(-1, 2)
        A = cell.shape[0]
        x = x.reshape(N, H, W, A, 5 + K)
        grid = np.stack(np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32),
                                    indexing="ij"), -1)[None, :, :, None, :]
        dydx = F32(s) * oracle.sigmoid(x[..., 0:2]).reshape(x[..., 0:2].shape) - F32(0.5 * (s - 1))
        yx = ((grid + dydx) * F32(stride)).astype(F32)
        hw = (np.exp(x[..., 2:4]) * cell[None, None, None]).astype(F32)
        half = (F32(0.5) * hw).astype(F32)
        boxes.append(np.concatenate([yx - half, yx + half], -1).astype(F32).reshape(N, -1, 4))
        c = oracle.sigmoid(x[..., 4]).reshape(N, H, W, A)
        p = oracle.sigmoid(x[..., 5:]).reshape(N, H, W, A, K)
        conf.append(c.reshape(N, -1))
        prob.append((c[..., None] * p).astype(F32).reshape(N, -1, K))
    boxes, conf, prob = np.concatenate(boxes, 1), np.concatenate(conf, 1), np.concatenate(prob, 1)
    return boxes, conf, prob.max(-1), prob.argmax(-1).astype(np.int32), prob


def select(boxes, scores, classes, thresh, nms_thresh, max_det):
    """Threshold, NMS and padding on given dense values: boxes [N, P, 4],
    scores / classes [N, P].  Returns boxes [N, D, 4], scores, classes
    (int32), is_valid (bool) [N, D]."""
    boxes, scores = np.asarray(boxes, F32), np.asarray(scores, F32)
    N = boxes.shape[0]
    ob = np.zeros((N, max_det, 4), F32)
    os_ = np.zeros((N, max_det), F32)
    oc = np.zeros((N, max_det), np.int32)
    ov = np.zeros((N, max_det), bool)
    for n in range(N):
        idx = np.nonzero(scores[n] > F32(thresh))[0]
        keep = idx[oracle.nms(boxes[n][idx], scores[n][idx], max_det, nms_thresh)]
        k = len(keep)
        ob[n, :k], os_[n, :k], oc[n, :k], ov[n, :k] = boxes[n][keep], scores[n][keep], \
            np.asarray(classes)[n][keep], True
    return ob, os_, oc, ov


def inference(logits, strides, cell_hw, scale_yx, num_classes, thresh, nms_thresh, max_det):
    boxes, _, score, cls, _ = predictions(logits, strides, cell_hw, scale_yx, num_classes)
    return select(boxes, score, cls, thresh, nms_thresh, max_det)


def spp(x):
    """x [N, H, W, C] -> [N, H, W, 4C] = [pool13, pool9, pool5, x]: zero pad
    (tf.pad), VALID stride-1 max pools, concat."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    outs = []
    for k in (13, 9, 5):
        r = k // 2
        p = np.zeros((N, H + 2 * r, W + 2 * r, C), F32)
        p[:, r:r + H, r:r + W] = x
        m = np.full((N, H, W, C), -np.inf, F32)
        for dy in range(k):
            for dx in range(k):
                m = np.maximum(m, p[:, dy:dy + H, dx:dx + W])
        outs.append(m)
    return np.concatenate(outs + [x], -1)


def hand_made_case():
    """N = 1, K = 3, A = 3, levels (2, 2), (1, 1), (1, 1): P = 18, strides
    8 / 16 / 32, scale_yx 1 (dydx = sigmoid(raw) exactly), every cell anchor
    8 x 8, threshold 0.25, NMS 0.5, max_det 5.  Logits are 0 (sigmoid exactly
    0.5), +40 (exactly 1 in float32) or -40 (4e-18, "0" below), so every
    score that matters is exactly 0.25, 0.5 or 1; raw box terms are 0 (exp =
    1: an 8 x 8 box centred half a cell in):

      p0, p1  cell (0, 0) of level 0, anchors 0 and 1: the same box
              [0, 0, 8, 8]; p0 scores 1.0 (class 2), p1 0.5 -> p1 suppressed
      p3, p6  cells (0, 1) and (1, 0), anchor 0: boxes [0, 8, 8, 16] and
              [8, 0, 16, 8], both 0.5 exactly -> a score tie, p3 before p6
      p12     level 1: conf 1, classes (0.5, 0.5, 0) -> class tie, class 0;
              box [4, 4, 12, 12] overlaps p0 with IoU 16 / 112: kept
      p15     level 2: conf 0.5, best class 0.5 -> 0.25 == threshold: dropped
      the rest have conf 0: score 0

    Order: p0 (1.0), then the 0.5 group by index: p1 (suppressed by p0), p3,
    p6, p12.  Returns (case dict, expected dict)."""
    K, A = 3, 3
    hw = [(2, 2), (1, 1), (1, 1)]
    BIG = F32(40.0)
    logits = [np.zeros((1, h, w, A, 5 + K), F32) for h, w in hw]
    for x in logits:
        x[..., 4] = -BIG  # conf 0
    l0, l1, l2 = logits

    def put(x, h, w, a, conf, cls):
        x[0, h, w, a, 4] = conf
        x[0, h, w, a, 5:] = cls

    put(l0, 0, 0, 0, BIG, [-BIG, -BIG, BIG])     # p0: 1.0, class 2
    put(l0, 0, 0, 1, BIG, [-BIG, 0.0, -BIG])     # p1: 0.5, class 1
    put(l0, 0, 1, 0, 0.0, [BIG, -BIG, -BIG])     # p3: 0.5, class 0
    put(l0, 1, 0, 0, BIG, [-BIG, -BIG, 0.0])     # p6: 0.5, class 2
    put(l1, 0, 0, 0, BIG, [0.0, 0.0, -BIG])      # p12: 0.5, classes 0 and 1 tie
    put(l2, 0, 0, 0, 0.0, [0.0, -BIG, -BIG])     # p15: 0.25 == threshold
    case = {
        "logits": [x.reshape(1, h, w, A * (5 + K)) for x, (h, w) in zip(logits, hw)],
        "strides": [8, 16, 32],
        "cell_hw": [np.full((A, 2), 8.0, F32)] * 3,
        "scale_yx": [1.0, 1.0, 1.0],
        "num_classes": K, "thresh": 0.25, "nms_thresh": 0.5, "max_det": 5,
    }
    boxes = np.zeros((1, 5, 4), F32)
    boxes[0, :4] = [[0, 0, 8, 8], [0, 8, 8, 16], [8, 0, 16, 8], [4, 4, 12, 12]]
    expected = {
        "boxes": boxes,
        "scores": np.array([[1.0, 0.5, 0.5, 0.5, 0.0]], F32),
        "classes": np.array([[2, 0, 2, 0, 0]], np.int32),
        "is_valid": np.array([[1, 1, 1, 1, 0]], bool),
    }
    return case, expected
