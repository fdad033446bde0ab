"""CascadeROIHeads (lib/modeling/roi_heads/cascade_rcnn.py:14-273).

Three (len(ROI_BOX_CASCADE_HEAD.IOUS)) box heads on one shared pooler, each
with its own class-agnostic predictor and Box2BoxTransform.  Stage k > 0 runs
on stage k - 1's decoded, clipped boxes; the hand-over between two stages is
one launch (ops.cascade_refine: decode, clip, validity and, in training, the
re-match against the ground truth at IOUS[k] with its gathers).  Inference
averages the stages' softmax scores inside the fused Fast R-CNN
post-processing (ops.fast_rcnn_inference_stages) and decodes the last stage's
deltas.  The mask branch, the deferred mask loss and forward_with_given_boxes
are StandardROIHeads'.

Deviations from the reference: stage k matches with
its own proposal_matchers[k] threshold (the reference builds them and then
calls the stage-0 matcher); rows the crowd / difficult rule ignores keep
their box and drop out of that stage's losses; gt_index indexes the full GT
list; training validity chains through the stages.
"""
import torch

from ...layers import ShapeSpec, ops
from ...structures import BoxList
from ..box_regression import Box2BoxTransform
from ..matcher import Matcher
from ..poolers import ROIPooler
from .box_head import build_box_head
from .fast_rcnn import FastRCNNOutputLayers, fast_rcnn_losses
from .roi_heads import ROI_HEADS_REGISTRY, StandardROIHeads, _cached_index


@ROI_HEADS_REGISTRY.register()
class CascadeROIHeads(StandardROIHeads):
    def _init_box_head(self, cfg):
        b = cfg.MODEL.ROI_BOX_HEAD
        weights = cfg.MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS
        ious = [float(t) for t in cfg.MODEL.ROI_BOX_CASCADE_HEAD.IOUS]
        self.num_cascade_stages = len(ious)
        assert len(weights) == self.num_cascade_stages
        assert 1 <= self.num_cascade_stages <= 4, "the fused score average takes 1..4 stages"
        assert b.CLS_AGNOSTIC_BBOX_REG, "CascadeROIHeads only support class-agnostic regression"
        assert ious[0] == cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS[0]
        scales = tuple(1.0 / self.feature_strides[k] for k in self.in_features)
        chans = {self.feature_channels[f] for f in self.in_features}
        assert len(chans) == 1, chans
        c = chans.pop()
        self.box_pooler = ROIPooler(b.POOLER_RESOLUTION, scales, b.POOLER_SAMPLING_RATIO,
                                    b.POOLER_TYPE)
        pooled = ShapeSpec(channels=c, height=b.POOLER_RESOLUTION, width=b.POOLER_RESOLUTION)
        heads, predictors = [], []
        self.box2box_transform = []
        # (stage 0 is matched by ROIHeads.proposal_matcher, in label_and_sample_proposals)
        self.proposal_matchers = [None]
        for k in range(self.num_cascade_stages):
            head = build_box_head(cfg, pooled, scope=f"box_head_stage{k + 1}")
            heads.append(head)
            predictors.append(FastRCNNOutputLayers(head.output_size, self.num_classes, True,
                                                   scope=f"box_predictor_stage{k + 1}"))
            self.box2box_transform.append(Box2BoxTransform(weights=weights[k]))
            if k > 0:
                self.proposal_matchers.append(Matcher([ious[k]], [0, 1],
                                                      allow_low_quality_matches=False))
        self.box_head = torch.nn.ModuleList(heads)
        self.box_predictor = torch.nn.ModuleList(predictors)
        # set by call() for the duration of one forward (the inherited call
        # passes neither to _box_losses)
        self._cascade_image_hw = self._cascade_targets = None

    def _run_stage(self, feats, boxes, img, k, grad_share=None):
        x = self.box_pooler.pool(feats, boxes.reshape(-1, 4).contiguous(), img,
                                 grad_share=grad_share)
        if self.training:
            # the heads' losses are added, the gradient on the shared features
            # is their mean (cascade_rcnn.py:227-231)
            x = ops.scale_gradient(x, 1.0 / self.num_cascade_stages)
        return self.box_predictor[k](self.box_head[k](x))

    def _box_losses(self, feats, sampled, grad_share=None):
        """Stage 0 on the sampled proposals, stage k > 0 on stage k - 1's
        refined boxes re-labelled at IOUS[k] (no resampling):
        loss_cls_stage{k} / loss_box_reg_stage{k}."""
        targets, image_hw = self._cascade_targets, self._cascade_image_hw
        if targets is None or image_hw is None:
            raise RuntimeError("CascadeROIHeads._box_losses runs inside call(): the stage "
                               "hand-overs need its image shapes and targets")
        boxes = sampled["boxes"]
        N, S = boxes.shape[:2]
        img = _cached_index("img", N, S, boxes.device)
        cur = {"boxes": boxes, "is_valid": sampled["is_valid"], "gt_classes": sampled["gt_classes"],
               "gt_boxes": sampled["gt_boxes"], "loss_valid": sampled["is_valid"]}
        losses = {}
        for k in range(self.num_cascade_stages):
            if k > 0:
                cur = ops.cascade_refine(
                    deltas, cur["boxes"], cur["is_valid"], image_hw,
                    self.box2box_transform[k - 1].weights,
                    self.box2box_transform[k - 1].scale_clamp, gt_boxes=targets["gt_boxes"],
                    gt_valid=targets["is_valid"], gt_classes=targets["gt_classes"],
                    gt_crowd=targets.get("gt_is_crowd"), gt_difficult=targets.get("gt_difficult"),
                    iou_thr=self.proposal_matchers[k].thresholds[1], num_classes=self.num_classes)
            # the mask pooler's two-party backward hand-off is met by stage 0's
            # pooling (the standard box / mask pair); the later stages' pools
            # take the plain backward
            logits, deltas = self._run_stage(feats, cur["boxes"], img, k,
                                             grad_share if k == 0 else None)
            stage = fast_rcnn_losses(logits, deltas, cur["boxes"].reshape(-1, 4),
                                     cur["gt_classes"].reshape(-1),
                                     cur["gt_boxes"].reshape(-1, 4), cur["loss_valid"].reshape(-1),
                                     self.box2box_transform[k], self.smooth_l1_beta)
            losses.update({f"{name}_stage{k}": v for name, v in stage.items()})
        return losses

    def call(self, images, features, proposals, targets=None):
        # the stage hand-overs need the image shapes and the ground truth,
        # which StandardROIHeads.call does not pass to _box_losses
        self._cascade_image_hw = images.image_shapes
        self._cascade_targets = targets
        try:
            return super().call(images, features, proposals, targets)
        finally:
            self._cascade_image_hw = self._cascade_targets = None

    def _forward_box(self, feats, proposals, image_shapes):
        boxes = proposals.boxes
        valid = proposals.get_field("is_valid")
        N, P = valid.shape
        dev = boxes.device
        img = _cached_index("img", N, P, dev)
        slot = _cached_index("slot", N, P, dev)
        slot = torch.where(valid.reshape(-1), slot, torch.full_like(slot, -1))
        stage_logits = []
        for k in range(self.num_cascade_stages):
            if k > 0:
                t = self.box2box_transform[k - 1]
                boxes = ops.cascade_refine(deltas, boxes, valid, image_shapes, t.weights,
                                           t.scale_clamp)["boxes"]
            logits, deltas = self._run_stage(feats, boxes, img, k)
            stage_logits.append(logits)
        t = self.box2box_transform[-1]
        ob, os_, oc, ov, _ = ops.fast_rcnn_inference_stages(
            stage_logits, deltas, boxes.reshape(-1, 4), img, slot, N, P, image_shapes, t.weights,
            self.test_score_thresh, self.test_nms_thresh, self.test_detections_per_img,
            cls_agnostic=self.num_classes != 1, scale_clamp=t.scale_clamp,
            nms_cls_agnostic=self.test_nms_cls_agnostic)
        res = BoxList(ob)
        res.add_field("scores", os_)
        res.add_field("pred_classes", oc)
        res.add_field("is_valid", ov)
        res.set_tracking("image_shape", image_shapes)
        return res
