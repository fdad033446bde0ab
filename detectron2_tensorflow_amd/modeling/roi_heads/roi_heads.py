"""ROIHeads / StandardROIHeads (lib/modeling/roi_heads/roi_heads.py:66-605).

Dense, synchronisation-free layout: the RPN hands over [N, P] proposals with
an is_valid mask; every slot is pooled (invalid slots pool a zero box and are
dropped by the fused Fast R-CNN post-processing through roi_slot = -1), so
the box branch needs no tf.where / host round trip.  The mask branch pools
the [N, max_det] detections the same way and zeroes invalid rows — the
values the reference's SparseBoxList.to_dense produces.
"""
from typing import Any, NamedTuple, Optional

import torch

from ...layers import ShapeSpec, handoff, ops
from ...structures import BoxList
from ...utils import capture, host_sync
from ...utils.registry import Registry
from ..box_regression import Box2BoxTransform
from ..poolers import ROIPooler
from .box_head import build_box_head
from ..matcher import Matcher, match_boxes, subsample_labels
from .fast_rcnn import FastRCNNOutputLayers, fast_rcnn_inference, fast_rcnn_losses
from .mask_head import build_mask_head, mask_rcnn_inference, mask_rcnn_loss

from ...layers import Layer


# Per-step constant index tensors (image id of each row, per-image bases),
# cached per shape and device: read-only, so one tensor serves every step
# (two launches each fewer per use).
_INDEX_CACHE = {}


def _cached_index(kind, n, m, device):
    key = (kind, int(n), int(m), str(device))
    t = _INDEX_CACHE.get(key)
    if t is None:
        if len(_INDEX_CACHE) > 256:
            _INDEX_CACHE.clear()
        if kind == "img":  # arange(n).repeat_interleave(m), int32
            t = torch.arange(n, dtype=torch.int32, device=device).repeat_interleave(m)
        elif kind == "slot":  # arange(m).repeat(n), int32
            t = torch.arange(m, dtype=torch.int32, device=device).repeat(n)
        else:  # "base": arange(n)[:, None] * m, int64
            t = torch.arange(n, device=device)[:, None] * m
        # (made inside a hipGraph capture, the tensor holds its values only
        # once that graph has replayed: not cached for anything else)
        if not capture.capturing():
            _INDEX_CACHE[key] = t
    return t

ROI_HEADS_REGISTRY = Registry("ROI_HEADS")

# GPU: the sampled ROI batch in fg-first order straight from the fused
# sampler (d2mi_subsample order output) instead of a key sort (A/B switch)
FUSED_ORDER = True
# The label / take / mask-prep glue on d2mi_roi_gt_classes and
# d2mi_roi_sample_take (False: torch's gathers, selects, argsort; tests compare).
FUSED_SAMPLE_TAKE = True


def build_roi_heads(cfg, input_shape, **kwargs):
    return ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, input_shape, **kwargs)


class MaskPrep(NamedTuple):
    """The training mask branch's inputs over the first F = int(S *
    POSITIVE_FRACTION) slots per image.  The six per-row tensors (ROWS; compact
    rows: fg first, each group in slot order) are None until _prepared."""
    fg_slots: torch.Tensor  # [N*F] bool foreground flags, in slot order
    boxes: Optional[torch.Tensor] = None
    classes: Optional[torch.Tensor] = None
    fg: Optional[torch.Tensor] = None
    img: Optional[torch.Tensor] = None
    gt_mask_index: Optional[torch.Tensor] = None  # row of the flattened gt_masks
    gt_boxes: Optional[torch.Tensor] = None
    gt_masks: Optional[torch.Tensor] = None  # [N*G, ...]
    count: Optional[torch.Tensor] = None  # device-side foreground count (the fused sampler's)
    pending: Any = None  # the count's host read in flight (host_sync.start_read)

    ROWS = ("boxes", "classes", "fg", "img", "gt_mask_index", "gt_boxes")

    def head(self, n):
        return self._replace(**{k: getattr(self, k)[:n] for k in self.ROWS})

    def device_count(self):
        return self.count if self.count is not None else self.fg_slots.sum()


class ROIHeads(Layer):
    # True: in training the head's poolers take the merged ROIAlign backward and
    # meet the RPN's gradient on the shared levels (rcnn._tag_shared_levels).
    # False where the pooled map has one reader and no pooler pair.
    merged_pool_backward = True
    # True: the training forward can return its mask loss unrun (a
    # DeferredMaskLoss), so the step can be captured into hipGraphs.  False
    # where the forward itself needs the foreground count on the host.
    mask_loss_deferrable = True

    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(**kwargs)
        h = cfg.MODEL.ROI_HEADS
        self.batch_size_per_image = h.BATCH_SIZE_PER_IMAGE
        self.positive_sample_fraction = h.POSITIVE_FRACTION
        # the first slots per image, which hold every sampled foreground proposal
        self.mask_slots = int(h.BATCH_SIZE_PER_IMAGE * h.POSITIVE_FRACTION)
        self.test_score_thresh = h.SCORE_THRESH_TEST
        self.test_nms_thresh = h.NMS_THRESH_TEST
        self.test_nms_cls_agnostic = h.NMS_CLS_AGNOSTIC
        self.test_detections_per_img = cfg.TEST.DETECTIONS_PER_IMAGE
        self.in_features = list(h.IN_FEATURES)
        self.num_classes = h.NUM_CLASSES
        self.proposal_append_gt = h.PROPOSAL_APPEND_GT
        self.feature_strides = {k: v.stride for k, v in input_shape.items()}
        self.feature_channels = {k: v.channels for k, v in input_shape.items()}
        self.cls_agnostic_bbox_reg = cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG
        self.smooth_l1_beta = cfg.MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA
        self.box2box_transform = Box2BoxTransform(weights=cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS)
        self.proposal_matcher = Matcher(h.IOU_THRESHOLDS, h.IOU_LABELS,
                                        allow_low_quality_matches=False)

    def label_and_sample_proposals(self, proposals, targets):
        """roi_heads.py:100-232 batched: append GT (proposal_utils.py:7-60), match
        (crowd -> ignore bg, difficult -> ignore bg above the threshold), gt_classes
        (fg class / bg = NUM_CLASSES / -1), subsample, fg-first order, pad.
        Returns a dict of [N, S] tensors: boxes, gt_classes, gt_boxes, gt_index
        (matched GT row), is_valid."""
        return self._sample(proposals, targets)[0]

    def _sample(self, proposals, targets, mask_slots=0):
        """(label_and_sample_proposals' dict, the MaskPrep over the first
        mask_slots slots per image that the fused sampler makes in the same
        launch, or None: mask_slots 0, or the tensor arm)."""
        boxes = proposals.boxes
        pvalid = proposals.get_field("is_valid")
        gt_boxes = targets["gt_boxes"]
        gvalid = targets["is_valid"].bool()
        N, G = gvalid.shape
        zeros = torch.zeros_like(gvalid)
        crowd = targets.get("gt_is_crowd", zeros).bool()
        difficult = targets.get("gt_difficult", zeros).bool()
        if self.proposal_append_gt:
            boxes = torch.cat([boxes, gt_boxes.to(boxes.dtype)], dim=1)
            pvalid = torch.cat([pvalid, gvalid], dim=1)
        M = boxes.shape[1]
        # (matched against the valid GT that are neither crowd nor difficult)
        matches, labels = match_boxes(self.proposal_matcher, gt_boxes, gvalid, boxes,
                                      crowd=crowd, difficult=difficult)
        K = self.num_classes
        S = self.batch_size_per_image
        if boxes.is_cuda and FUSED_ORDER and FUSED_SAMPLE_TAKE:
            # two launches for the glue (d2mi_roi_gt_classes, d2mi_roi_sample_take),
            # the mask branch's fg-first inputs and foreground count included
            gt_classes = ops.roi_gt_classes(labels, matches, targets["gt_classes"], pvalid, K)
            _, _, order, valid = subsample_labels(gt_classes, S, self.positive_sample_fraction, K,
                                                  order_slots=S)
            sampled, fused = ops.roi_sample_take(order, valid, boxes, gt_classes, matches,
                                                 gt_boxes, K, mask_slots)
            if fused is not None:
                rows, fg_slots, count = fused
                fused = MaskPrep(fg_slots, *rows, gt_masks=targets["gt_masks"].flatten(0, 1),
                                 count=count)
            return sampled, fused
        gcls = torch.gather(targets["gt_classes"].long(), 1, matches)
        # label 1 -> the matched GT class, 0 -> background K, -1 -> ignored;
        # invalid proposal slots -> -1
        gt_classes = torch.where(labels == 1, gcls, torch.where(labels == 0, K, labels))
        gt_classes = torch.where(pvalid, gt_classes, -1)
        if boxes.is_cuda and FUSED_ORDER:
            # fused: the sampled rows come back in fg-first, index order
            _, _, order, valid = subsample_labels(gt_classes, S, self.positive_sample_fraction, K,
                                                  order_slots=S)
        else:
            pos, neg = subsample_labels(gt_classes, S, self.positive_sample_fraction, K)
            ar = torch.arange(M, device=boxes.device)
            key = torch.where(pos, 0, torch.where(neg, 1, 2)) * M + ar
            if M < S:
                key = torch.cat([key, torch.full((N, S - M), 3 * M, dtype=key.dtype,
                                                 device=key.device)], dim=1)
            key = key.sort(dim=1).values[:, :S]
            valid = key < 2 * M
            order = torch.where(valid, key % M, torch.zeros_like(key))
        take = lambda t: torch.gather(t, 1, order)
        take4 = lambda t: torch.gather(t, 1, order[..., None].expand(-1, -1, 4))
        gidx = take(matches)
        return {"boxes": take4(boxes), "gt_classes": take(gt_classes), "gt_index": gidx,
                "gt_boxes": torch.gather(gt_boxes, 1, gidx[..., None].expand(-1, -1, 4)),
                "is_valid": valid}, None

    def _proposal_rows(self, proposals):
        """The inference prologue: (boxes [N, P, 4], valid [N, P], image id and
        slot of each of the N*P rows -- slot -1 on an invalid row, which the
        fused post-processing drops --, N, P)."""
        boxes = proposals.boxes
        valid = proposals.get_field("is_valid")
        N, P = valid.shape
        img = _cached_index("img", N, P, boxes.device)
        slot = _cached_index("slot", N, P, boxes.device)
        slot = torch.where(valid.reshape(-1), slot, torch.full_like(slot, -1))
        return boxes, valid, img, slot, N, P

    def _detections(self, boxes, scores, classes, valid, image_shapes):
        res = BoxList(boxes)
        res.add_field("scores", scores)
        res.add_field("pred_classes", classes)
        res.add_field("is_valid", valid)
        res.set_tracking("image_shape", image_shapes)
        return res


class DeferredMaskLoss:
    """The training mask loss of a StandardROIHeads forward, not yet run:
    the foreground count is known only on the device (``count``), and the
    compacted mask branch's row count depends on it.  A step captured into
    hipGraphs (engine/graphed.py) replays the forward up to here, reads
    ``count`` once, and replays the mask branch + backward graph captured for
    that row count (``compute(rows)``, run once per distinct row count at
    capture time) on the step's MaskPrep (``plan``).  The eager trainer never
    sees one (defer_mask_loss False)."""

    def __init__(self, heads, feats, sampled, targets, plan, share):
        self.heads, self.feats, self.sampled, self.targets = heads, feats, sampled, targets
        self.plan, self.share = plan, share
        self.count = plan.device_count()
        self.slots = plan.fg_slots.numel()

    def rows_for(self, nfg):
        return self.heads.mask_rows(int(nfg), self.slots)

    def compute(self, rows):
        return self.heads._mask_loss(self.feats, self.sampled, self.targets, self.plan, self.share,
                                     rows=rows)


@ROI_HEADS_REGISTRY.register()
class StandardROIHeads(ROIHeads):
    """The step every ROI head runs (``call``: inference _forward_box ->
    forward_with_given_boxes; training _sample -> _plan_mask -> _losses).  A
    variant overrides the pieces: its layers (_init_box_head, _init_mask_head),
    _box_losses or the whole _losses, the middle of _forward_box, _mask_outputs."""
    MASK_ROW_BUCKET = 32
    # the mask branch's fg-first ordering and per-slot gathers issued before
    # the foreground-count read, so less host work follows it
    MASK_PREP_EARLY = True

    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(cfg, input_shape, **kwargs)
        self.mask_on = cfg.MODEL.MASK_ON
        self.use_mini_masks = cfg.TRANSFORM.RESIZE.USE_MINI_MASKS
        # True: mask head on the foreground rows only, like the reference (one
        # host sync per step); False: fixed [N, S*POSITIVE_FRACTION] rows with
        # a validity mask (no host sync, capturable).
        self.mask_compact_rows = True
        # True (set by engine.graphed.GraphedTrainer): the training forward
        # returns a DeferredMaskLoss instead of reading the foreground count
        self.defer_mask_loss = False
        self.last_mask_rows = None
        self._init_box_head(cfg)
        if self.mask_on:
            self._init_mask_head(cfg)

    def _pooler(self, p):
        """(the pooler of the config node p on in_features, the shape of its rows)"""
        scales = tuple(1.0 / self.feature_strides[k] for k in self.in_features)
        chans = {self.feature_channels[f] for f in self.in_features}
        assert len(chans) == 1, chans
        return (ROIPooler(p.POOLER_RESOLUTION, scales, p.POOLER_SAMPLING_RATIO, p.POOLER_TYPE),
                ShapeSpec(channels=chans.pop(), height=p.POOLER_RESOLUTION,
                          width=p.POOLER_RESOLUTION))

    def _init_box_head(self, cfg):
        self.box_pooler, pooled = self._pooler(cfg.MODEL.ROI_BOX_HEAD)
        self.box_head = build_box_head(cfg, pooled, scope="box_head")
        self.box_predictor = FastRCNNOutputLayers(self.box_head.output_size, self.num_classes,
                                                  self.cls_agnostic_bbox_reg, scope="box_predictor")

    def _init_mask_head(self, cfg):
        self.mask_pooler, pooled = self._pooler(cfg.MODEL.ROI_MASK_HEAD)
        self.mask_head = build_mask_head(cfg, pooled, scope="mask_head")

    def call(self, images, features, proposals, targets=None):
        feats = [features[f] for f in self.in_features]
        if not self.training:
            pred = self._forward_box(feats, proposals, images.image_shapes)
            return self.forward_with_given_boxes(features, pred), {}
        if targets is None:
            raise ValueError("ROI-head training needs targets")
        sampled, fused = self._sample(
            proposals, targets, self.mask_slots if self.mask_on and self.mask_compact_rows else 0)
        plan = self._plan_mask(sampled, fused, targets)
        return sampled, self._losses(feats, sampled, plan, images, targets)

    def _defers(self):
        return self.mask_loss_deferrable and self.mask_compact_rows and self.defer_mask_loss

    def _plan_mask(self, sampled, fused, targets):
        """The step's MaskPrep (None without a mask branch): the fused
        sampler's, or the foreground flags with the per-row tensors made here
        (MASK_PREP_EARLY) or left to _prepared.  With compact rows the count's
        host read starts here, to run while the box branch is enqueued (the
        device never idles at the read); a deferred mask loss starts none."""
        if not self.mask_on:
            return None
        plan = fused if fused is not None else MaskPrep(self._mask_fg(sampled))  # (once per step)
        if self.mask_compact_rows:
            if not self._defers():
                plan = plan._replace(pending=host_sync.start_read(plan.device_count()))
            # (deferred too, r5: in a replayed step these small gathers are
            # issued inside graph A, under the box branch's kernels, not at
            # graph B's head where the host's per-node submission outran them)
            if self.MASK_PREP_EARLY:
                plan = self._prepared(plan, sampled, targets)
        return plan

    def _prepared(self, plan, sampled, targets):
        if plan.boxes is not None:
            return plan
        return self._mask_prep(sampled, targets, plan.fg_slots)._replace(pending=plan.pending)

    def _losses(self, feats, sampled, plan, images, targets):
        # the box and mask poolers read the same p2..p5: one gradient map
        # set for both backwards (ops.roi._RoIAlignFn grad_share)
        share = handoff.PoolerShare() if self.mask_on else None
        losses = self._box_losses(feats, sampled, images.image_shapes, targets, share)
        if plan is not None and self._defers():
            losses["loss_mask"] = DeferredMaskLoss(self, feats, sampled, targets, plan, share)
        elif plan is not None:
            losses["loss_mask"] = self._mask_loss(feats, sampled, targets, plan, share)
        return losses

    def _box_features(self, x, boxes, valid):
        """The box head on the pooled rows of boxes [N, P, 4] / valid [N, P]
        (a subclass whose head looks at the proposals routes them here)."""
        return self.box_head(x)

    def _forward_box(self, feats, proposals, image_shapes):
        boxes, valid, img, slot, N, P = self._proposal_rows(proposals)
        x = self.box_pooler.pool(feats, boxes.reshape(-1, 4), img)
        x = self._box_features(x, boxes, valid)
        return self._predict(x, boxes, img, slot, N, P, image_shapes)

    def _predict(self, x, boxes, img, slot, N, P, image_shapes):
        logits, deltas = self.box_predictor(x)
        return self._detections(*fast_rcnn_inference(
            logits, deltas, boxes.reshape(-1, 4), img, slot, N, P, image_shapes,
            self.box2box_transform, self.test_score_thresh, self.test_nms_thresh,
            self.test_detections_per_img, self.test_nms_cls_agnostic)[:4], image_shapes)

    def _box_losses(self, feats, sampled, image_shapes, targets, grad_share=None):
        # (image_shapes and targets: the step's context, for CascadeROIHeads)
        boxes = sampled["boxes"]
        N, S = boxes.shape[:2]
        img = _cached_index("img", N, S, boxes.device)
        x = self.box_pooler.pool(feats, boxes.reshape(-1, 4).contiguous(), img,
                                 grad_share=grad_share)
        return self._predictor_losses(self._box_features(x, boxes, sampled["is_valid"]), sampled)

    def _predictor_losses(self, x, sampled):
        logits, deltas = self.box_predictor(x)
        return fast_rcnn_losses(logits, deltas, sampled["boxes"].reshape(-1, 4),
                                sampled["gt_classes"].reshape(-1),
                                sampled["gt_boxes"].reshape(-1, 4), sampled["is_valid"].reshape(-1),
                                self.box2box_transform, self.smooth_l1_beta)

    def _mask_fg(self, sampled):
        """Foreground flags of the first int(S * POSITIVE_FRACTION) slots per image:
        valid and not background.  (A sampled slot is a positive, class in
        [0, K), or a negative, class K -- the ignored -1 rows are never
        sampled -- so `class < K` is the reference's `!= -1 and != bg` there.)"""
        return (sampled["is_valid"][:, :self.mask_slots]
                & (sampled["gt_classes"][:, :self.mask_slots] < self.num_classes)).reshape(-1)

    def mask_rows(self, nfg, slots):
        """Rows the compacted mask branch runs for nfg foreground proposals out
        of ``slots``: nfg rounded up to a multiple of MASK_ROW_BUCKET (at least
        one bucket, at most every slot) -- a handful of distinct shapes."""
        b = self.MASK_ROW_BUCKET
        return min(slots, max(b, -(-nfg // b) * b))

    def _mask_prep(self, sampled, targets, fg=None):
        """The MaskPrep of the sampled rows, made with tensor ops: the per-slot
        inputs over the first int(S * POSITIVE_FRACTION) slots per image, and
        (compact rows) the slots in fg-first order -- everything that does not
        need the foreground count, so the host issues it before the count's read."""
        N, F_ = sampled["boxes"].shape[0], self.mask_slots
        boxes = sampled["boxes"][:, :F_].reshape(-1, 4)
        dev = boxes.device
        cls = sampled["gt_classes"][:, :F_].reshape(-1)
        fg = self._mask_fg(sampled) if fg is None else fg
        img = _cached_index("img", N, F_, dev)
        gm = targets["gt_masks"]
        G = gm.shape[1]
        mind = (sampled["gt_index"][:, :F_] + _cached_index("base", N, G, dev)).reshape(-1)
        gt_boxes = sampled["gt_boxes"][:, :F_].reshape(-1, 4)
        rows = (boxes, cls, fg, img, mind, gt_boxes)
        if self.mask_compact_rows:
            # fg rows first, each group in index order (a stable sort of ~fg);
            # the count only decides how many of them run (a view)
            order = torch.argsort((~fg).to(torch.uint8), stable=True)
            rows = tuple(t[order] for t in rows)
        return MaskPrep(fg, *rows, gt_masks=gm.flatten(0, 1))

    def _mask_loss(self, feats, sampled, targets, plan, grad_share=None, rows=None):
        """_forward_mask training branch (roi_heads.py:594-600) over the first
        int(S * POSITIVE_FRACTION) slots per image, which hold every sampled
        foreground proposal (select_foreground_proposals, roi_heads.py:35-62)."""
        plan = self._prepared(plan, sampled, targets)
        if self.mask_compact_rows:
            # The reference runs the mask head on the foreground proposals only
            # (select_foreground_proposals, roi_heads.py:35-62 + :594-600).  One
            # host read of the foreground count; the rows are gathered fg-first
            # (image order kept) and padded to a multiple of MASK_ROW_BUCKET
            # with masked-out rows, which bounds the number of distinct shapes.
            # (rows given: a deferred mask loss, DeferredMaskLoss.compute)
            if rows is None:
                rows = self.mask_rows(host_sync.finish_read(plan.pending)[0], plan.fg_slots.numel())
            plan = plan.head(rows)
        self.last_mask_rows = int(plan.boxes.shape[0])
        x = self.mask_pooler.pool(feats, plan.boxes.contiguous(), plan.img, grad_share=grad_share)
        _, logits = self.mask_head(x)
        return self._mask_rcnn_loss(logits, plan)

    def _mask_rcnn_loss(self, logits, plan):
        return mask_rcnn_loss(logits, plan.boxes, plan.gt_boxes, plan.classes, plan.gt_masks,
                              plan.gt_mask_index, plan.fg, self.use_mini_masks)

    def _mask_outputs(self, feats, boxes, img):
        """The mask head's (deconv, logits) on boxes [R, 4] of images img [R]."""
        return self.mask_head(self.mask_pooler.pool(feats, boxes, img))

    def forward_with_given_boxes(self, features, instances, image_shape=None):
        assert not self.training
        assert instances.has_field("pred_classes")
        if not self.mask_on:
            return instances
        feats = [features[f] for f in self.in_features]
        boxes = instances.boxes
        N, D = boxes.shape[:2]
        img = _cached_index("img", N, D, boxes.device)
        _, logits = self._mask_outputs(feats, boxes.reshape(-1, 4), img)
        masks = mask_rcnn_inference(logits, instances.get_field("pred_classes").reshape(-1))
        valid = instances.get_field("is_valid").reshape(-1)
        masks = masks * valid[:, None, None].to(masks.dtype)
        instances.add_field("pred_masks", masks.reshape(N, D, *masks.shape[1:]))
        return instances

