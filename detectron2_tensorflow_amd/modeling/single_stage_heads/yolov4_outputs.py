"""YOLOv4 training targets and losses (lib/modeling/single_stage_heads/
yolov4_outputs.py:59-206 _get_ground_truth, :266-329 losses;
lib/modeling/matcher.py:176-267 YOLOMatcher; lib/structures/box_list_ops.py:
295-450 pairwise / matched CIoU; lib/layers/loss.py:140-196 iou_loss).

Two arms behind FUSED_YOLO_LOSS (this module owns the toggle):

* fused: ops.yolov4_loss, the kernels of csrc/yolo_loss.hip (GPU tensors);
* tensor: ``yolov4_losses_dense`` below, the same loss on dense torch tensors
  in the dtype of the logits, any device: the CPU path and the tests' other
  arm.  It selects the positives with boolean masks, which synchronises with
  the host on a GPU; the fused arm does not.

Both keep the reference's behaviour listed in DESIGN.md section 9 ("YOLOv4
loss: reference behaviour kept"): the GT's (h, w) in stride units against
cell anchors in pixels, the highest GT index's box and the multi-hot classes
of a slot that several GT share, no negatives in an image without a valid GT,
the padded batch area in the box weight, and matched_iou's width2 =
x_max1 - x_min2.
"""
import math

import torch
import torch.nn.functional as F

from ...layers import ops

# True: the HIP kernels on GPU tensors; False: the tensor formulation.
# (measured in DESIGN.md section 5, "YOLOv4 training")
FUSED_YOLO_LOSS = True

_CIOU_V = 4 / math.pi ** 2


class YOLOMatcher(object):
    """matcher.py:176-267 on dense rows: ``anchor_matrix`` [..., M, L * A]
    and ``pred_matrix`` [..., M, P] hold one row per GT slot, ``valid``
    [..., M] marks the rows that exist (the reference's boolean_mask).
    Returns (best_anchor_inds [..., M], respond_bgd [..., P]): the first
    maximum of each GT's anchor row, and 1 where the maximum over the valid
    rows of pred_matrix is below the threshold -- 0 everywhere when no row is
    valid (:236-242).  The crowd and difficult matrices only turn zeros of
    respond_bgd into -1 (:244-266), which every reader treats as 0
    (yolov4_outputs.py:195, :278), so they are accepted and applied the same
    way but change no loss."""

    def __init__(self, threshold):
        self.threshold = threshold

    def __call__(self, anchor_matrix, pred_matrix, crowd_matrix=None, difficult_matrix=None,
                 valid=None):
        if valid is None:
            valid = torch.ones(pred_matrix.shape[:-1], dtype=torch.bool, device=pred_matrix.device)
        best_anchor_inds = torch.argmax(anchor_matrix, dim=-1)  # the first maximum (tf.argmax)
        best_anchor_inds = torch.where(valid, best_anchor_inds, torch.zeros_like(best_anchor_inds))
        respond_bgd = self._below(pred_matrix, valid, self.threshold).to(torch.int64)
        for matrix, thr in ((crowd_matrix, 1e-3), (difficult_matrix, self.threshold)):
            if matrix is None:
                continue
            rows = torch.ones(matrix.shape[:-1], dtype=torch.bool, device=matrix.device)
            above = ~self._below(matrix, rows, thr, strict=False) & rows.any(-1, keepdim=True)
            respond_bgd = torch.where((respond_bgd == 0) & above, respond_bgd - 1, respond_bgd)
        return best_anchor_inds, respond_bgd

    @staticmethod
    def _below(matrix, rows, thr, strict=True):
        """max over the marked rows < thr (strict) / <= thr, False with no row."""
        neg = torch.full_like(matrix, -math.inf)
        m = torch.where(rows[..., None], matrix, neg).amax(dim=-2) if matrix.shape[-2] else \
            neg.new_full(matrix.shape[:-2] + matrix.shape[-1:], -math.inf)
        below = (m < thr) if strict else (m <= thr)
        return below & rows.any(-1, keepdim=True)


def predictions(pred_logits, strides, cell_anchors, scale_yx, num_classes):
    """_get_predictions (:208-264) in the logits' dtype: boxes [N, P, 4], conf
    logits [N, P], class logits [N, P, K], level-major then (h, w, a)."""
    K = int(num_classes)
    boxes, conf, cls = [], [], []
    for x, stride, cell, s in zip(pred_logits, strides, cell_anchors, scale_yx):
        N, H, W, _ = x.shape
        cell = torch.as_tensor(cell).to(x).reshape(-1, 4)
        A = cell.shape[0]
        x = x.reshape(N, H, W, A, 5 + K)
        gy, gx = torch.meshgrid(torch.arange(H, device=x.device, dtype=x.dtype),
                                torch.arange(W, device=x.device, dtype=x.dtype), indexing="ij")
        grid = torch.stack([gy, gx], -1)[None, :, :, None, :]
        dydx = float(s) * torch.sigmoid(x[..., 0:2]) - 0.5 * (float(s) - 1)
        yx = (grid + dydx) * float(stride)
        hw = torch.exp(x[..., 2:4]) * cell[:, 2:]
        boxes.append(torch.cat([yx - 0.5 * hw, yx + 0.5 * hw], -1).reshape(N, -1, 4))
        conf.append(x[..., 4].reshape(N, -1))
        cls.append(x[..., 5:].reshape(N, -1, K))
    return torch.cat(boxes, 1), torch.cat(conf, 1), torch.cat(cls, 1)


def _iou_parts(b1, b2, width2):
    y1a, x1a, y2a, x2a = b1.unbind(-1)
    y1b, x1b, y2b, x2b = b2.unbind(-1)
    zero = torch.zeros((), dtype=b1.dtype, device=b1.device)
    ih = torch.maximum(zero, torch.minimum(y2a, y2b) - torch.maximum(y1a, y1b))
    iw = torch.maximum(zero, torch.minimum(x2a, x2b) - torch.maximum(x1a, x1b))
    inter = ih * iw
    h1, w1 = y2a - y1a, x2a - x1a
    h2 = y2b - y1b
    unions = h1 * w1 + h2 * width2 - inter
    safe = torch.where(unions == 0, torch.ones_like(unions), unions)
    iou = torch.where(unions == 0, torch.zeros_like(unions), inter / safe)
    c2 = (torch.maximum(y2a, y2b) - torch.minimum(y1a, y1b)) ** 2 + \
         (torch.maximum(x2a, x2b) - torch.minimum(x1a, x1b)) ** 2
    d2 = ((x1a + x2a) / 2. - (x1b + x2b) / 2.) ** 2 + ((y1a + y2a) / 2. - (y1b + y2b) / 2.) ** 2
    safe_c = torch.where(c2 == 0, torch.ones_like(c2), c2)
    diou = iou - torch.where(c2 == 0, torch.zeros_like(c2), d2 / safe_c)
    v = _CIOU_V * (torch.atan(w1 / h1) - torch.atan(width2 / h2)) ** 2
    den = 1. - iou + v
    # coincident boxes: 0 / 0 in the reference, alpha * v = 0 here
    safe_d = torch.where(den == 0, torch.ones_like(den), den)
    return diou - torch.where(den == 0, torch.zeros_like(den), v / safe_d * v)


def pairwise_ciou(boxes1, boxes2):
    """box_list_ops.pairwise_iou(iou_type="ciou") (:295-372): boxes1
    [..., M, 4], boxes2 [..., P, 4] -> [..., M, P]."""
    b1, b2 = boxes1[..., :, None, :], boxes2[..., None, :, :]
    return _iou_parts(b1, b2, b2[..., 3] - b2[..., 1])


def matched_ciou(boxes1, boxes2):
    """box_list_ops.matched_iou(iou_type="ciou") (:375-450), row by row, with
    its width2 = x_max1 - x_min2 (:405)."""
    return _iou_parts(boxes1, boxes2, boxes1[..., 3] - boxes2[..., 1])


def _plain_iou(b1, b2):
    """pairwise_iou (iou_type "iou") of [..., 4] against [A, 4] -> [..., A]."""
    b1, b2 = b1[..., None, :], b2
    zero = torch.zeros((), dtype=b1.dtype, device=b1.device)
    ih = torch.maximum(zero, torch.minimum(b1[..., 2], b2[:, 2]) - torch.maximum(b1[..., 0], b2[:, 0]))
    iw = torch.maximum(zero, torch.minimum(b1[..., 3], b2[:, 3]) - torch.maximum(b1[..., 1], b2[:, 1]))
    inter = ih * iw
    unions = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1]) + \
        (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1]) - inter
    safe = torch.where(unions == 0, torch.ones_like(unions), unions)
    return torch.where(unions == 0, torch.zeros_like(unions), inter / safe)


def assign(matcher, gt_boxes, valid, strides, cell_anchors, grid_hw, pred_matrix=None):
    """:86-146 on dense rows: gt_boxes [N, G, 4], valid [N, G].  Returns
    (slot [N, G] int64: the flat prediction index, -1 for a row that is not
    valid or whose cell is outside the grid -- the reference's scatter is
    undefined there; respond_bgd [N, P] or None without pred_matrix)."""
    N, G = valid.shape
    A = torch.as_tensor(cell_anchors[0]).reshape(-1, 4).shape[0]
    rows, cells = [], []
    for cell, stride in zip(cell_anchors, strides):
        cell = torch.as_tensor(cell).to(gt_boxes).reshape(-1, 4)
        y0, x0, y1, x1 = (gt_boxes * 1. / float(stride)).unbind(-1)
        h, w = y1 - y0, x1 - x0
        cells.append(torch.stack([torch.floor((y0 + y1) / 2.), torch.floor((x0 + x1) / 2.)], -1))
        zeroed = torch.stack([torch.zeros_like(h), torch.zeros_like(w), h, w], -1)
        rows.append(_plain_iou(zeroed, cell))
    anchor_matrix = torch.cat(rows, -1)  # [N, G, L * A]
    if pred_matrix is None:
        best = torch.argmax(anchor_matrix, dim=-1)
        bgd = None
    else:
        best, bgd = matcher(anchor_matrix, pred_matrix, valid=valid)
    level, a = best // A, best % A
    cells = torch.stack(cells, 2)  # [N, G, L, 2]
    cyx = torch.gather(cells, 2, level[..., None, None].expand(-1, -1, 1, 2))[:, :, 0]
    H = torch.tensor([h for h, _ in grid_hw], device=valid.device)[level]
    W = torch.tensor([w for _, w in grid_hw], device=valid.device)[level]
    sizes = [h * w * A for h, w in grid_hw]
    p0 = torch.tensor([sum(sizes[:i]) for i in range(len(sizes))], device=valid.device)[level]
    cy, cx = cyx[..., 0], cyx[..., 1]
    inside = (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
    slot = p0 + (cy.clamp(min=0).long() * W + cx.clamp(min=0).long()) * A + a
    return torch.where(valid & inside, slot, torch.full_like(slot, -1)), bgd


def yolov4_losses_dense(pred_logits, strides, cell_anchors, scale_yx, num_classes, gt_boxes,
                        gt_classes, valid, image_hw, iou_threshold, cls_normalizer,
                        iou_normalizer, debug=None):
    """The arguments and the result of ops.yolov4_loss: (conf_loss, cls_loss,
    box_loss, num_pos, num_neg).  ``valid`` is is_valid & ~crowd & ~difficult.
    ``debug``: a dict that receives slot, owner and state (0 neither, 1
    negative, 2 positive)."""
    K = int(num_classes)
    N = pred_logits[0].shape[0]
    dt, dev = pred_logits[0].dtype, pred_logits[0].device
    boxes, conf_logits, cls_logits = predictions(pred_logits, strides, cell_anchors, scale_yx, K)
    P = boxes.shape[1]
    gt_boxes = gt_boxes.to(dt)
    valid = valid.bool()
    G = valid.shape[1]
    grid_hw = [(int(t.shape[1]), int(t.shape[2])) for t in pred_logits]
    with torch.no_grad():  # map_fn(back_prop=False), :201-206
        pred_matrix = pairwise_ciou(gt_boxes, boxes.detach())
        slot, bgd = assign(YOLOMatcher(iou_threshold), gt_boxes, valid, strides, cell_anchors,
                           grid_hw, pred_matrix)
        # sparse.to_dense(validate_indices=False): the last write (the highest
        # GT index) leaves the box, the classes of all writers stay set
        idx = torch.where(slot >= 0, slot, torch.full_like(slot, P))
        gi = torch.arange(G, device=dev).expand(N, G)
        owner = torch.full((N, P + 1), -1, dtype=torch.int64, device=dev)
        owner = owner.scatter_reduce(1, idx, gi, "amax")[:, :P] if G else owner[:, :P]
        label = torch.zeros((N, P + 1, K), dtype=dt, device=dev)
        if G:
            ni = torch.arange(N, device=dev)[:, None].expand(N, G)
            label[ni, idx, gt_classes.long().clamp(0, K - 1)] = 1.0
        label = label[:, :P]
        pos = owner >= 0
        neg = ~pos & (bgd > 0)
        target = torch.gather(gt_boxes, 1, owner.clamp(min=0)[..., None].expand(-1, -1, 4)) if G \
            else boxes.new_zeros((N, P, 4))
    rb = pos.to(dt)
    n_img = float(N)
    cls_loss = cls_normalizer / n_img * F.binary_cross_entropy_with_logits(
        cls_logits[pos], label[pos], reduction="sum")
    tb, pb = target[pos], boxes[pos]
    area = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    image_area = float(image_hw[0] * image_hw[1])
    weight = (2.0 - area / image_area) * iou_normalizer / n_img
    box_loss = ((1 - matched_ciou(pb, tb)) * weight).sum()
    vm = pos | neg
    focal = (rb - torch.sigmoid(conf_logits))[vm] ** 2
    conf_loss = 1. / n_img * (focal * F.binary_cross_entropy_with_logits(
        conf_logits[vm], rb[vm], reduction="none")).sum()
    if debug is not None:
        debug.update(slot=slot, owner=owner, state=(pos.to(torch.uint8) * 2 + neg.to(torch.uint8)))
    return conf_loss, cls_loss, box_loss, pos.sum(), neg.sum()


def yolov4_losses(pred_logits, strides, cell_anchors, scale_yx, num_classes, gt_boxes, gt_classes,
                  valid, image_hw, iou_threshold, cls_normalizer, iou_normalizer, debug=None):
    """The arm FUSED_YOLO_LOSS selects (the kernels need GPU tensors)."""
    fn = ops.yolov4_loss if FUSED_YOLO_LOSS and pred_logits[0].is_cuda else yolov4_losses_dense
    return fn(pred_logits, strides, cell_anchors, scale_yx, num_classes, gt_boxes, gt_classes,
              valid, image_hw, iou_threshold, cls_normalizer, iou_normalizer, debug=debug)
