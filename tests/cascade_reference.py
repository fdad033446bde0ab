"""Cascade R-CNN stage hand-over restated from the oracle's pieces
(lib/modeling/roi_heads/cascade_rcnn.py:141-215 _match_and_label_boxes,
:244-273 _create_proposals_from_boxes), per image, numpy:

  oracle.apply_deltas -> oracle.clip_to_window([0, 0, h, w]) -> oracle.area > 0
  -> training.pairwise_iou of the valid, non-crowd, non-difficult GT (and of
  the crowd / difficult GT) -> training.matcher([thr], [0, 1], no low-quality
  matches) -> the matched class / index / box.

With the decisions of DESIGN.md section 9: the stage's own threshold, ignored
rows (-1) keep their box and leave the loss, gt_index into the full [G] list,
validity chained (valid_k = valid_{k-1} and area > 0; inference: unchanged).
"""
import numpy as np

import oracle
import training

F32 = np.float32


def refine(deltas, boxes, valid, image_hw, weights, gt=None, iou_thr=None, num_classes=None,
           decoded=None):
    """deltas [N*S, 4], boxes [N, S, 4], valid [N, S] bool, image_hw [N, 2].
    gt (training): dict of gt_boxes [N, G, 4], is_valid, gt_classes and optional
    gt_is_crowd / gt_difficult [N, G].  decoded [N, S, 4]: boxes to label instead
    of this function's own decode (a kernel's output: an expf ulp cannot flip
    a label then).  Returns a dict of numpy arrays like ops.cascade_refine."""
    boxes = np.asarray(boxes, F32)
    N, S = boxes.shape[:2]
    deltas = np.asarray(deltas, F32).reshape(N, S, 4)
    valid = np.asarray(valid, bool)
    out = np.zeros((N, S, 4), F32)
    for n in range(N):
        h, w = image_hw[n]
        dec = oracle.apply_deltas(deltas[n], boxes[n], weights)
        out[n] = oracle.clip_to_window(dec, [0, 0, h, w])
    if gt is None:
        return {"boxes": out, "is_valid": valid.copy()}
    lab_boxes = out if decoded is None else np.asarray(decoded, F32)
    G = gt["gt_boxes"].shape[1]
    zeros = np.zeros((N, G), bool)
    crowd = np.asarray(gt.get("gt_is_crowd", zeros), bool)
    diff = np.asarray(gt.get("gt_difficult", zeros), bool)
    res = {"boxes": out, "is_valid": np.zeros((N, S), bool),
           "gt_classes": np.zeros((N, S), np.int64), "gt_index": np.zeros((N, S), np.int64),
           "gt_boxes": np.zeros((N, S, 4), F32), "loss_valid": np.zeros((N, S), bool)}
    for n in range(N):
        b = lab_boxes[n]
        gb = np.asarray(gt["gt_boxes"][n], F32)
        ok = valid[n] & (oracle.area(b) > 0)
        matchable = np.asarray(gt["is_valid"][n], bool) & ~crowd[n] & ~diff[n]
        q = training.pairwise_iou(gb[matchable], b)
        m, lab = training.matcher(q, [iou_thr], [0, 1], False,
                                  crowd=training.pairwise_iou(gb[crowd[n]], b),
                                  difficult=training.pairwise_iou(gb[diff[n]], b))
        full = np.nonzero(matchable)[0]
        idx = full[m] if len(full) else np.zeros(S, np.int64)
        cls = np.where(lab == 1, np.asarray(gt["gt_classes"][n], np.int64)[idx],
                       np.where(lab == 0, num_classes, -1))
        cls = np.where(ok, cls, -1)
        res["is_valid"][n] = ok
        res["gt_classes"][n] = cls
        res["gt_index"][n] = idx
        res["gt_boxes"][n] = gb[idx]
        res["loss_valid"][n] = ok & (cls >= 0)
    return res


def hand_made_case():
    """N = 2, S = 70, G = 5 with the rows that decide the semantics (image 0
    is 100 x 120; zero deltas keep a box as it is):
      row 0  decoded fully outside the image -> clipped to area 0 -> invalid
      row 1  on two identical GT (0 and 1)    -> the first wins
      row 2  [0, 0, 10, 20] vs GT 2 [0, 0, 10, 10]: IoU exactly 0.5
             (foreground at thr 0.5, background at thr 0.6)
      row 3  inside the crowd GT 3 only       -> ignored (-1): loss_valid 0, is_valid 1
      row 4  an already-invalid input slot
      rows 5..69 seeded random boxes and deltas
    Image 1 has no valid GT: every row background, match 0."""
    rng = np.random.default_rng(7)
    N, S, G = 2, 70, 5
    image_hw = np.array([[100, 120], [90, 110]], np.int32)
    c = rng.uniform([0, 0], [90, 110], size=(N, S, 2))
    hw = rng.uniform(4, 50, size=(N, S, 2))
    boxes = np.concatenate([c - hw / 2, c + hw / 2], -1).astype(F32)
    deltas = (rng.normal(size=(N, S, 4)) * [1.0, 1.0, 0.5, 0.5]).astype(F32)
    valid = np.ones((N, S), bool)
    gt_boxes = np.array([[[30, 30, 60, 70], [30, 30, 60, 70], [0, 0, 10, 10], [60, 80, 100, 120],
                          [20, 5, 45, 25]]] * N, F32)
    boxes[0, 0] = [200, 200, 240, 260]
    boxes[0, 1] = [32, 30, 60, 68]
    boxes[0, 2] = [0, 0, 10, 20]
    boxes[0, 3] = [70, 90, 90, 110]
    deltas[0, :5] = 0
    valid[0, 4] = False
    gt = {"gt_boxes": gt_boxes,
          "is_valid": np.array([[1, 1, 1, 1, 1], [0, 0, 0, 0, 0]], bool),
          "gt_classes": np.array([[3, 9, 11, 5, 7], [1, 2, 3, 4, 5]], np.int64),
          "gt_is_crowd": np.array([[0, 0, 0, 1, 0], [0, 0, 0, 0, 0]], bool),
          "gt_difficult": np.zeros((N, G), bool)}
    return deltas.reshape(N * S, 4), boxes, valid, image_hw, gt
