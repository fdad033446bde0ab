"""PanopticFPN (lib/modeling/meta_arch/panoptic_fpn.py:16-296).

Mask R-CNN (backbone, FPN, RPN, StandardROIHeads) plus the semantic head of
semantic_seg.py on the same FPN levels.  Training returns loss_sem_seg, the
detector losses x INSTANCE_LOSS_WEIGHT and the RPN losses;
batched_inputs["sem_seg"] is [N, H, W] integer labels.  Inference returns
"instances" (masks pasted onto the canvas: the "raw" format is refused, as in
the reference), "sem_seg" ([N, H, W] int64 class map) and, with
COMBINE.ENABLED, "panoptic_seg": the dict of
combine_semantic_and_instance_outputs (ops.panoptic_combine).

The FPN levels have three readers here (RPN head, ROI poolers, semantic
head), so the two-reader level hand-off of GeneralizedRCNN._tag_shared_levels
is not engaged: autograd sums the three gradients.

Deviations (unbound names in the reference, not behaviours): ``image_shapes``
at :86 is images.image_shapes; ``self.output_resolution`` at :112 is
segmentation_output_resolution; the labels are padded to the image canvas
(the neck's divisibility), not the backbone's.
"""
from ...layers import Layer, ops
from ..backbone import build_backbone
from ..necks import build_neck
from ..postprocessing import detector_postprocess
from ..proposal_generator import build_proposal_generator
from ..roi_heads import build_roi_heads
from .build import META_ARCH_REGISTRY
from .rcnn import _Preprocess
from .semantic_seg import build_sem_seg_head


@META_ARCH_REGISTRY.register()
class PanopticFPN(_Preprocess, Layer):
    def __init__(self, cfg, **kwargs):
        super().__init__(**kwargs)
        p = cfg.MODEL.PANOPTIC_FPN
        self.instance_loss_weight = p.INSTANCE_LOSS_WEIGHT
        self.combine_on = p.COMBINE.ENABLED
        self.combine_overlap_threshold = p.COMBINE.OVERLAP_THRESH
        self.combine_stuff_area_limit = p.COMBINE.STUFF_AREA_LIMIT
        self.combine_instances_confidence_threshold = p.COMBINE.INSTANCES_CONFIDENCE_THRESH
        self.backbone = build_backbone(cfg, scope="backbone")
        self.neck = build_neck(cfg, self.backbone.output_shape(), scope="neck")
        self.proposal_generator = build_proposal_generator(cfg, self.neck.output_shape(),
                                                           scope="proposal_generator")
        self.roi_heads = build_roi_heads(cfg, self.neck.output_shape(), scope="roi_heads")
        self.sem_seg_head = build_sem_seg_head(cfg, self.neck.output_shape(), scope="sem_seg_head")
        self._init_preprocess(cfg)
        self.segmentation_output_format = cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT
        self.segmentation_output_resolution = cfg.MODEL.SEGMENTATION_OUTPUT.FIXED_RESOLUTION
        assert self.segmentation_output_format != "raw", "Must transform box masks to image masks."

    def call(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        images = self.preprocess_image(batched_inputs)
        features = self.neck(self.backbone(images.tensor))
        _, sem_seg_losses = self.sem_seg_head(features, batched_inputs["sem_seg"],
                                              images.image_shapes)
        gt = batched_inputs.get("instances")
        if self.proposal_generator is not None:
            proposals, proposal_losses, _ = self.proposal_generator(images, features, gt)
        else:
            proposals, proposal_losses = batched_inputs["proposals"], {}
        _, detector_losses = self.roi_heads(images, features, proposals, gt)
        losses = {}
        losses.update(sem_seg_losses)
        losses.update({k: v * self.instance_loss_weight for k, v in detector_losses.items()})
        losses.update(proposal_losses)
        return losses

    def inference(self, batched_inputs):
        assert not self.training
        images = self.preprocess_image(batched_inputs)
        features = self.neck(self.backbone(images.tensor))
        logits, _ = self.sem_seg_head(features)
        if self.proposal_generator is not None:
            proposals, *_ = self.proposal_generator(images, features, None)
        else:
            proposals = batched_inputs["proposals"]
        results, _ = self.roi_heads(images, features, proposals, None)
        assert results.has_field("pred_masks"), "PanopticFPN needs MODEL.MASK_ON"
        fmt = self.segmentation_output_format
        if fmt == "fixed":
            shape = (self.segmentation_output_resolution,) * 2
        else:  # "conventional": the padded input canvas
            shape = tuple(images.tensor.shape[1:3])
        inst = {"boxes": results.boxes, "classes": results.get_field("pred_classes"),
                "scores": results.get_field("scores"), "is_valid": results.get_field("is_valid"),
                "masks": results.get_field("pred_masks")}
        inst = detector_postprocess(inst, shape, fmt, images.image_shapes)
        sem_seg = self.sem_seg_head.predictions(logits, images, fmt,
                                                self.segmentation_output_resolution)
        out = {"instances": inst, "sem_seg": sem_seg}
        if self.combine_on:
            out["panoptic_seg"] = ops.panoptic_combine(
                inst["masks"], inst["scores"], inst["classes"], inst["boxes"], inst["is_valid"],
                sem_seg, self.combine_overlap_threshold, self.combine_stuff_area_limit,
                self.combine_instances_confidence_threshold, self.sem_seg_head.num_classes)
        return out
