"""YOLOv4's training loss restated line by line from the reference, torch on
the CPU, one image at a time (lib/modeling/single_stage_heads/
yolov4_outputs.py:59-206 _get_ground_truth, :208-264 _get_predictions,
:266-329 losses; lib/modeling/matcher.py:176-267 YOLOMatcher;
lib/structures/box_list_ops.py:295-372 pairwise_iou, :375-450 matched_iou;
lib/layers/loss.py:140-196 iou_loss).  float64 by default (the tests' truth);
float32 gives "the reference's own float32 error".  Gradients are autograd's.

Every quirk is kept as written: the GT's (h, w) in stride units compared with
cell anchors in pixels, the sparse.to_dense scatters (last write wins for the
box, every write sets its class), no negatives without a valid GT, crowd and
difficult matrices that only turn zeros of respond_bgd into -1, the padded
image area in the box weight, matched_iou's width2 = x_max1 - x_min2.

Two places the reference leaves undefined are excluded by the callers' inputs:
a GT whose cell is outside the grid (asserted here) and a predicted box that
coincides with its target (0 / 0 in alpha).
"""
import math

import numpy as np
import torch

STRIDES = [8, 16, 32]
CELL_HW = [[[16, 12], [36, 19], [28, 40]], [[75, 36], [55, 76], [146, 72]],
           [[110, 142], [243, 192], [410, 459]]]   # (h, w) of the [0, 0, h, w] cell anchors
SCALE_YX = [1.2, 1.1, 1.05]


def cell_anchors():
    return [np.array([[0, 0, h, w] for h, w in lvl], np.float32) for lvl in CELL_HW]


def get_predictions(logits, K, dtype):
    """:208-264.  logits[l] [N, H, W, A * (5 + K)] -> boxes [N, P, 4], conf
    [N, P], raw conf [N, P], raw prob [N, P, K]."""
    boxes_all, conf_all, raw_conf_all, raw_prob_all = [], [], [], []
    for level, x in enumerate(logits):
        cell = torch.tensor(cell_anchors()[level], dtype=dtype)
        A = cell.shape[0]
        stride, scale_yx = STRIDES[level], SCALE_YX[level]
        N, H, W, _ = x.shape
        x = x.reshape(N, H, W, A, 5 + K)
        raw_dydx, raw_dhdw, raw_conf, raw_prob = torch.split(x, [2, 2, 1, K], dim=-1)
        gy, gx = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype),
                                indexing="ij")
        anchor_grid = torch.stack([gy, gx], -1).reshape(1, H, W, 1, 2).expand(N, H, W, A, 2)
        dydx = scale_yx * torch.sigmoid(raw_dydx) - 0.5 * (scale_yx - 1)
        pred_yx = (anchor_grid + dydx) * stride
        pred_hw = torch.exp(raw_dhdw) * cell[:, 2:]
        box_min = pred_yx - 0.5 * pred_hw
        box_max = pred_yx + 0.5 * pred_hw
        boxes_all.append(torch.cat([box_min, box_max], -1).reshape(N, -1, 4))
        conf_all.append(torch.sigmoid(raw_conf).reshape(N, -1))
        raw_conf_all.append(raw_conf.reshape(N, -1))
        raw_prob_all.append(raw_prob.reshape(N, -1, K))
    return (torch.cat(boxes_all, 1), torch.cat(conf_all, 1), torch.cat(raw_conf_all, 1),
            torch.cat(raw_prob_all, 1))


def pairwise_iou(b1, b2, iou_type="iou"):
    """:295-372.  b1 [M, 4], b2 [P, 4] -> [M, P]."""
    y_min1, x_min1, y_max1, x_max1 = [c.reshape(-1, 1) for c in b1.unbind(1)]
    y_min2, x_min2, y_max2, x_max2 = [c.reshape(1, -1) for c in b2.unbind(1)]
    zero = torch.zeros((), dtype=b1.dtype)
    intersect_heights = torch.maximum(zero, torch.minimum(y_max1, y_max2) - torch.maximum(y_min1, y_min2))
    intersect_widths = torch.maximum(zero, torch.minimum(x_max1, x_max2) - torch.maximum(x_min1, x_min2))
    intersections = intersect_heights * intersect_widths
    height1, width1 = y_max1 - y_min1, x_max1 - x_min1
    areas1 = height1 * width1
    height2, width2 = y_max2 - y_min2, x_max2 - x_min2
    areas2 = height2 * width2
    unions = areas1 + areas2 - intersections
    iou = torch.where(unions == 0.0, torch.zeros_like(unions), intersections / unions)
    if iou_type == "iou":
        return iou
    assert iou_type == "ciou"
    max_ymax, min_ymin = torch.maximum(y_max1, y_max2), torch.minimum(y_min1, y_min2)
    max_xmax, min_xmin = torch.maximum(x_max1, x_max2), torch.minimum(x_min1, x_min2)
    convex_diagonal_squares = (max_ymax - min_ymin) ** 2 + (max_xmax - min_xmin) ** 2
    centerpoint_distance_squares = ((x_min1 + x_max1) / 2. - (x_min2 + x_max2) / 2.) ** 2 + \
        ((y_min1 + y_max1) / 2. - (y_min2 + y_max2) / 2.) ** 2
    diou = iou - torch.where(convex_diagonal_squares == 0.0, torch.zeros_like(iou),
                             centerpoint_distance_squares / convex_diagonal_squares)
    v = 4 / math.pi ** 2 * (torch.atan(width1 / height1) - torch.atan(width2 / height2)) ** 2
    alpha = v / (1. - iou + v)
    return diou - alpha * v


def matched_iou_ciou(b1, b2):
    """:375-450 with iou_type "ciou".  b1, b2 [R, 4] -> [R]."""
    y_min1, x_min1, y_max1, x_max1 = b1.unbind(1)
    y_min2, x_min2, y_max2, x_max2 = b2.unbind(1)
    zero = torch.zeros((), dtype=b1.dtype)
    intersect_heights = torch.maximum(zero, torch.minimum(y_max1, y_max2) - torch.maximum(y_min1, y_min2))
    intersect_widths = torch.maximum(zero, torch.minimum(x_max1, x_max2) - torch.maximum(x_min1, x_min2))
    intersections = intersect_heights * intersect_widths
    height1 = y_max1 - y_min1
    width1 = x_max1 - x_min1
    areas1 = height1 * width1
    height2 = y_max2 - y_min2
    width2 = x_max1 - x_min2          # :405, as written
    areas2 = height2 * width2
    unions = areas1 + areas2 - intersections
    iou = torch.where(unions == 0.0, torch.zeros_like(unions), intersections / unions)
    max_ymax, min_ymin = torch.maximum(y_max1, y_max2), torch.minimum(y_min1, y_min2)
    max_xmax, min_xmin = torch.maximum(x_max1, x_max2), torch.minimum(x_min1, x_min2)
    convex_diagonal_squares = (max_ymax - min_ymin) ** 2 + (max_xmax - min_xmin) ** 2
    centerpoint_distance_squares = ((x_min1 + x_max1) / 2. - (x_min2 + x_max2) / 2.) ** 2 + \
        ((y_min1 + y_max1) / 2. - (y_min2 + y_max2) / 2.) ** 2
    diou = iou - torch.where(convex_diagonal_squares == 0.0, torch.zeros_like(iou),
                             centerpoint_distance_squares / convex_diagonal_squares)
    v = 4 / math.pi ** 2 * (torch.atan(width1 / height1) - torch.atan(width2 / height2)) ** 2
    alpha = v / (1. - iou + v)
    return diou - alpha * v


def yolo_matcher(threshold, anchor_matrix, pred_matrix, crowd_matrix, difficult_matrix):
    """matcher.py:197-267."""
    M, N = pred_matrix.shape
    if M > 0:
        max_iou = pred_matrix.max(dim=0).values
        respond_bgd = torch.where(max_iou < threshold, torch.ones(N, dtype=torch.int64),
                                  torch.zeros(N, dtype=torch.int64))
        best_anchor_inds = torch.argmax(anchor_matrix, dim=1)
    else:
        max_iou = torch.full((N,), float("nan"), dtype=pred_matrix.dtype)
        best_anchor_inds = torch.zeros(M, dtype=torch.int64)
        respond_bgd = torch.zeros(N, dtype=torch.int64)
    crowd_bool = crowd_matrix.max(dim=0).values > 1e-3 if crowd_matrix.shape[0] > 0 else \
        torch.zeros(N, dtype=torch.bool)
    respond_bgd = torch.where((respond_bgd == 0) & crowd_bool, torch.zeros_like(respond_bgd) - 1,
                              respond_bgd)
    difficult_bool = difficult_matrix.max(dim=0).values > threshold \
        if difficult_matrix.shape[0] > 0 else torch.zeros(N, dtype=torch.bool)
    respond_bgd = torch.where((respond_bgd == 0) & difficult_bool,
                              torch.zeros_like(respond_bgd) - 1, respond_bgd)
    return best_anchor_inds, respond_bgd, max_iou


def to_dense(indices, values, shape, dtype):
    """tf.sparse.to_dense(validate_indices=False) on the CPU: the writes in
    order, the last one stays."""
    out = torch.zeros(shape, dtype=dtype)
    for ind, val in zip(indices.tolist(), values.tolist()):
        out[tuple(ind)] = val
    return out


def ground_truth_single_image(gt_boxes, gt_classes, is_valid, is_crowd, is_difficult,
                              predicted_boxes, grid_sizes, K, threshold):
    """get_ground_truth_single_image, :74-198."""
    dtype = predicted_boxes.dtype
    A = 3
    is_valid_bool = is_valid & ~is_crowd & ~is_difficult
    valid_boxes = gt_boxes[is_valid_bool]
    crowd_boxes = gt_boxes[is_crowd]
    difficult_boxes = gt_boxes[is_difficult]
    anchor_match_matrix, grid_inds = [], []
    for cell, stride in zip(cell_anchors(), STRIDES):
        y_min, x_min, y_max, x_max = [c.reshape(-1, 1) for c in valid_boxes.unbind(1)]
        y_min, y_max = y_min * 1. / stride, y_max * 1. / stride
        x_min, x_max = x_min * 1. / stride, x_max * 1. / stride
        center_y, center_x = (y_min + y_max) / 2., (x_min + x_max) / 2.
        height, width = y_max - y_min, x_max - x_min
        grid_inds.append(torch.cat([torch.floor(center_y).long(), torch.floor(center_x).long()], 1))
        zeroed = torch.cat([torch.zeros_like(height), torch.zeros_like(width), height, width], 1)
        anchor_match_matrix.append(pairwise_iou(zeroed, torch.tensor(cell, dtype=dtype)))
    anchor_match_matrix = torch.cat(anchor_match_matrix, 1)
    grid_inds = torch.stack(grid_inds)  # [L, M, 2]
    predicted_match_matrix = pairwise_iou(valid_boxes, predicted_boxes, "ciou")
    crowd_matrix = pairwise_iou(crowd_boxes, predicted_boxes, "ciou")
    difficult_matrix = pairwise_iou(difficult_boxes, predicted_boxes, "ciou")
    best_anchor_inds, respond_bgd, max_iou = yolo_matcher(
        threshold, anchor_match_matrix, predicted_match_matrix, crowd_matrix, difficult_matrix)
    level_assignments = best_anchor_inds // A
    M = level_assignments.shape[0]
    grid_idxs = grid_inds[level_assignments, torch.arange(M)]
    level_anchor_inds = best_anchor_inds % A
    matched_anchor_inds = torch.cat([grid_idxs, level_anchor_inds[:, None]], 1)
    classes = gt_classes[is_valid_bool].long()
    matched_classes_inds = torch.cat([matched_anchor_inds, classes[:, None]], 1)
    respond_bbox, label_prob, target_boxes = [], [], []
    for level, (H, W) in enumerate(grid_sizes):
        level_inds = torch.nonzero(level_assignments == level)[:, 0]
        inds = matched_anchor_inds[level_inds]
        assert ((inds[:, 0] >= 0) & (inds[:, 0] < H) & (inds[:, 1] >= 0) & (inds[:, 1] < W)).all(), \
            "a GT centre outside the grid: undefined in the reference"
        ones = torch.ones(len(level_inds), dtype=dtype)
        respond_bbox.append(to_dense(inds, ones, (H, W, A), dtype).reshape(-1))
        label_prob.append(to_dense(matched_classes_inds[level_inds], ones, (H, W, A, K),
                                   dtype).reshape(-1, K))
        level_gt_boxes = valid_boxes[level_inds]
        target_boxes.append(torch.stack(
            [to_dense(inds, level_gt_boxes[:, i], (H, W, A), dtype).reshape(-1) for i in range(4)], -1))
    respond_bbox = torch.cat(respond_bbox)
    label_prob = torch.cat(label_prob)
    respond_bgd = (1. - respond_bbox) * respond_bgd.to(dtype)
    target_boxes = torch.cat(target_boxes)
    return respond_bgd, respond_bbox, label_prob, target_boxes, max_iou


def losses(logits, gt, K, threshold, cls_normalizer, iou_normalizer, image_hw, dtype=torch.float64):
    """YOLOV4Outputs.losses, :266-329.  logits: list of [N, H, W, A * (5 + K)]
    tensors (converted to ``dtype``; leaves that require grad).  gt: dict of
    gt_boxes [N, G, 4], gt_classes, is_valid, gt_is_crowd, gt_difficult.
    Returns a dict: the three losses, num_pos, num_neg, state [N, P] (0
    neither, 1 negative, 2 positive), label_prob, target_boxes, max_iou
    [N, P] (NaN rows for an image without a valid GT), leaves (the logits the
    losses were computed from, for .grad)."""
    leaves = [torch.as_tensor(x).detach().to(dtype).requires_grad_(True) for x in logits]
    pred_boxes, pred_confs, pred_conf_logits, pred_cls_logits = get_predictions(leaves, K, dtype)
    N = pred_boxes.shape[0]
    grid_sizes = [(int(x.shape[1]), int(x.shape[2])) for x in leaves]
    rows = []
    for n in range(N):  # tf.map_fn(back_prop=False)
        rows.append(ground_truth_single_image(
            torch.as_tensor(gt["gt_boxes"][n]).to(dtype), torch.as_tensor(gt["gt_classes"][n]),
            torch.as_tensor(gt["is_valid"][n]).bool(), torch.as_tensor(gt["gt_is_crowd"][n]).bool(),
            torch.as_tensor(gt["gt_difficult"][n]).bool(), pred_boxes[n].detach(), grid_sizes, K,
            threshold))
    respond_bgd, respond_bbox, label_prob, gt_boxes, max_iou = [torch.stack(c) for c in zip(*rows)]
    pos_masks = respond_bbox > 0
    neg_masks = respond_bgd > 0
    valid_masks = pos_masks | neg_masks
    num_images = float(N)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    cls_loss = cls_normalizer / num_images * bce(pred_cls_logits[pos_masks], label_prob[pos_masks],
                                                 reduction="sum") if pos_masks.any() else \
        torch.zeros((), dtype=dtype)
    gtb, pb = gt_boxes[pos_masks], pred_boxes[pos_masks]
    gt_box_area = (gtb[:, 2] - gtb[:, 0]) * (gtb[:, 3] - gtb[:, 1])
    image_area = float(image_hw[0] * image_hw[1])
    box_loss_scales = 2.0 - gt_box_area / image_area
    weight = box_loss_scales * iou_normalizer / num_images
    box_loss = ((1 - matched_iou_ciou(pb, gtb)) * weight).sum() if pos_masks.any() else \
        torch.zeros((), dtype=dtype)
    conf_focal = ((respond_bbox - pred_confs) ** 2)[valid_masks]
    conf_loss = 1. / num_images * (conf_focal * bce(pred_conf_logits[valid_masks],
                                                    respond_bbox[valid_masks],
                                                    reduction="none")).sum() \
        if valid_masks.any() else torch.zeros((), dtype=dtype)
    return {"conf_loss": conf_loss, "cls_loss": cls_loss, "box_loss": box_loss,
            "num_pos": int(pos_masks.sum()), "num_neg": int(neg_masks.sum()),
            "state": (pos_masks.to(torch.uint8) * 2 + neg_masks.to(torch.uint8)),
            "label_prob": label_prob, "target_boxes": gt_boxes, "max_iou": max_iou,
            "leaves": leaves}


def gradients(out, upstream):
    """d (sum of upstream[k] * loss k) / d logits, per level (zeros where no
    loss reaches)."""
    total = sum(float(upstream[k]) * out[k] for k in ("conf_loss", "cls_loss", "box_loss"))
    if not total.requires_grad:
        return [torch.zeros_like(x) for x in out["leaves"]]
    grads = torch.autograd.grad(total, out["leaves"], allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(grads, out["leaves"])]


# ------------------------------------------------------------------- cases
def make_logits(seed, N, K, hw, A=3):
    """(dy, dx) ~ N(0, 2), (dh, dw) ~ N(0, 0.5) clipped to [-2, 2], conf ~
    N(-1, 2), classes ~ N(-2, 2); float32."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in hw:
        x = rng.normal(0, 2, size=(N, h, w, A, 5 + K))
        x[..., 2:4] = np.clip(rng.normal(0, 0.5, size=x[..., 2:4].shape), -2, 2)
        x[..., 4] = rng.normal(-1, 2, size=x[..., 4].shape)
        x[..., 5:] = rng.normal(-2, 2, size=x[..., 5:].shape)
        out.append(torch.from_numpy(x.reshape(N, h, w, A * (5 + K)).astype(np.float32)))
    return out


def grids(H, W):
    return [(H // s, W // s) for s in STRIDES]


def hand_made_case(seed=0):
    """N = 2, image 64 x 96 (grids 8 x 12, 4 x 6, 2 x 3: P = 378), A = 3, K = 3,
    G = 8.  A GT's anchor row has 9 columns, column l * A + a being
    IoU([0, 0, h / stride_l, w / stride_l], cell anchor (l, a) in pixels): the
    reference's mix of units.  A box that fits the image is at most 8 x 12
    such units at level 0 and smaller at the others, so every cell anchor
    contains it and the smallest one, (level 0, anchor 0) = 16 x 12, wins;
    levels 1 and 2 are reached only by GT far larger than the image (the
    reference does not clip them), centred inside it.  Image 0, by GT row
    (y0, x0, y1, x1 | class):

      0  [8, 16, 24, 28] | 0        level 0, anchor 0; centre (16, 22) / 8 ->
                                    cell (2, 2): slot (2 * 12 + 2) * 3 = 78
      1  [10, 18, 22, 26] | 2       the same centre: slot 78 again, with
                                    another class -> the slot keeps GT 1's
                                    box and the classes {0, 2}
      2  [0, 0, 64, 96] | 1         8 x 12 units against 16 x 12 px: IoU 0.5,
                                    level 0, anchor 0; cell (4, 6): slot 162
      3  [30, 40, 50, 70] | 1       crowd: not valid
      4  [5, 60, 25, 90] | 2        difficult: not valid
      5  [-368, -152, 432, 248] | 0     800 x 400: 50 x 25 units at level 1,
                                    IoU 1250 / 2700 = 0.46 with its anchor 0
                                    (75 x 36); 0.22 at best at level 0.  Cell
                                    (32, 48) / 16 = (2, 3): slot 288 + 15 * 3
                                    = 333
      6  [-1568, -1552, 1632, 1648] | 2   3200 x 3200: 100 x 100 units at level
                                    2, IoU 10000 / 15620 = 0.64 with its anchor
                                    0 (110 x 142); 0.26 at best at level 1.
                                    Cell (1, 1): slot 360 + 4 * 3 = 372
      7                             padding (is_valid False)

    Image 1: one crowd row and padding, no valid GT: no positives and no
    negatives.  Returns (logits, gt dict, expected dict)."""
    K, G = 3, 8
    hw = grids(64, 96)
    logits = make_logits(seed, 2, K, hw)
    boxes = np.zeros((2, G, 4), np.float32)
    boxes[0, 0] = [8, 16, 24, 28]
    boxes[0, 1] = [10, 18, 22, 26]
    boxes[0, 2] = [0, 0, 64, 96]
    boxes[0, 3] = [30, 40, 50, 70]
    boxes[0, 4] = [5, 60, 25, 90]
    boxes[0, 5] = [-368, -152, 432, 248]
    boxes[0, 6] = [-1568, -1552, 1632, 1648]
    boxes[1, 0] = [10, 10, 40, 50]
    classes = np.zeros((2, G), np.int64)
    classes[0, :7] = [0, 2, 1, 1, 2, 0, 2]
    is_valid = np.zeros((2, G), bool)
    is_valid[0, :7] = True
    is_valid[1, 0] = True
    crowd = np.zeros((2, G), bool)
    crowd[0, 3] = True
    crowd[1, 0] = True
    difficult = np.zeros((2, G), bool)
    difficult[0, 4] = True
    gt = {"gt_boxes": torch.from_numpy(boxes), "gt_classes": torch.from_numpy(classes),
          "is_valid": torch.from_numpy(is_valid), "gt_is_crowd": torch.from_numpy(crowd),
          "gt_difficult": torch.from_numpy(difficult)}
    expected = {
        "slot": [[78, 78, 162, -1, -1, 333, 372, -1], [-1] * G],
        "owner": {(0, 78): 1, (0, 162): 2, (0, 333): 5, (0, 372): 6},
        "multi_hot": {(0, 78): [1, 0, 1], (0, 162): [0, 1, 0], (0, 333): [1, 0, 0],
                      (0, 372): [0, 0, 1]},
        "num_pos": 4,
    }
    return logits, gt, expected


def random_case(seed, N, K, H, W, G, num_valid):
    """GT with log-uniform sides in [8, 1.5 * the image's], centres strictly
    inside the image on a 1 / 4-pixel lattice (so the division by the strides
    is exact in float32 and float64 alike), a few crowd / difficult rows."""
    rng = np.random.default_rng(seed + 1000)
    logits = make_logits(seed, N, K, grids(H, W))
    boxes = np.zeros((N, G, 4), np.float32)
    classes = rng.integers(0, K, (N, G))
    is_valid = np.zeros((N, G), bool)
    crowd = np.zeros((N, G), bool)
    difficult = np.zeros((N, G), bool)
    for n in range(N):
        m = min(G, num_valid)
        is_valid[n, :m] = True
        h = np.round(np.exp(rng.uniform(np.log(8), np.log(1.5 * H), m)) * 2) / 2
        w = np.round(np.exp(rng.uniform(np.log(8), np.log(1.5 * W), m)) * 2) / 2
        cy = np.round(rng.uniform(1, H - 1, m) * 4) / 4
        cx = np.round(rng.uniform(1, W - 1, m) * 4) / 4
        boxes[n, :m] = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
        if m >= 4:
            crowd[n, m - 1] = True
            difficult[n, m - 2] = True
    gt = {"gt_boxes": torch.from_numpy(boxes), "gt_classes": torch.from_numpy(classes),
          "is_valid": torch.from_numpy(is_valid), "gt_is_crowd": torch.from_numpy(crowd),
          "gt_difficult": torch.from_numpy(difficult)}
    return logits, gt


def threshold_margin(out, threshold):
    """min |max CIoU - threshold| over every prediction of the images that have
    a valid GT (the others have no maximum and no negatives)."""
    m = out["max_iou"]
    m = m[~torch.isnan(m)]
    return float((m - threshold).abs().min()) if m.numel() else float("inf")
