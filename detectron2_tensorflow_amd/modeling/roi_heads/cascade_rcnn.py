"""CascadeROIHeads (lib/modeling/roi_heads/cascade_rcnn.py:14-273).

Three (len(ROI_BOX_CASCADE_HEAD.IOUS)) box heads on one shared pooler, each
with its own class-agnostic predictor and Box2BoxTransform.  Stage k > 0 runs
on stage k - 1's decoded, clipped boxes; the hand-over between two stages is
one launch (ops.cascade_refine: decode, clip, validity and, in training, the
re-match against the ground truth at IOUS[k] with its gathers).  Inference
averages the stages' softmax scores inside the fused Fast R-CNN
post-processing (ops.fast_rcnn_inference_stages) and decodes the last stage's
deltas.  The step (call), the mask branch, the deferred mask loss and
forward_with_given_boxes are StandardROIHeads'; the stage hand-overs get the
image shapes and the ground truth as _box_losses' arguments.

Deviations from the reference: stage k matches with
its own proposal_matchers[k] threshold (the reference builds them and then
calls the stage-0 matcher); rows the crowd / difficult rule ignores keep
their box and drop out of that stage's losses; gt_index indexes the full GT
list; training validity chains through the stages.
"""
import torch

from ...layers import ops
from ..box_regression import Box2BoxTransform
from ..matcher import Matcher
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
        self.box_pooler, pooled = self._pooler(b)
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

    def _run_stage(self, feats, boxes, img, k, grad_share=None):
        x = self.box_pooler.pool(feats, boxes.reshape(-1, 4).contiguous(), img,
                                 grad_share=grad_share)
        if self.training:
            # the heads' losses are added, the gradient on the shared features
            # is their mean (cascade_rcnn.py:227-231)
            x = ops.scale_gradient(x, 1.0 / self.num_cascade_stages)
        return self.box_predictor[k](self.box_head[k](x))

    def _box_losses(self, feats, sampled, image_shapes, targets, grad_share=None):
        """Stage 0 on the sampled proposals, stage k > 0 on stage k - 1's
        refined boxes re-labelled at IOUS[k] against ``targets`` (no
        resampling): loss_cls_stage{k} / loss_box_reg_stage{k}."""
        boxes = sampled["boxes"]
        N, S = boxes.shape[:2]
        img = _cached_index("img", N, S, boxes.device)
        cur = {"boxes": boxes, "is_valid": sampled["is_valid"], "gt_classes": sampled["gt_classes"],
               "gt_boxes": sampled["gt_boxes"], "loss_valid": sampled["is_valid"]}
        losses = {}
        for k in range(self.num_cascade_stages):
            if k > 0:
                cur = ops.cascade_refine(
                    deltas, cur["boxes"], cur["is_valid"], image_shapes,
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

    def _forward_box(self, feats, proposals, image_shapes):
        boxes, valid, img, slot, N, P = self._proposal_rows(proposals)
        stage_logits = []
        for k in range(self.num_cascade_stages):
            if k > 0:
                t = self.box2box_transform[k - 1]
                boxes = ops.cascade_refine(deltas, boxes, valid, image_shapes, t.weights,
                                           t.scale_clamp)["boxes"]
            logits, deltas = self._run_stage(feats, boxes, img, k)
            stage_logits.append(logits)
        t = self.box2box_transform[-1]
        return self._detections(*ops.fast_rcnn_inference_stages(
            stage_logits, deltas, boxes.reshape(-1, 4), img, slot, N, P, image_shapes, t.weights,
            self.test_score_thresh, self.test_nms_thresh, self.test_detections_per_img,
            cls_agnostic=self.num_classes != 1, scale_clamp=t.scale_clamp,
            nms_cls_agnostic=self.test_nms_cls_agnostic)[:4], image_shapes)

