"""YOLOV4Head (lib/modeling/single_stage_heads/yolov4.py:22-170,
yolov4_outputs.py:59-390).

Tower: per level a 3x3 conv (MODEL.YOLOV4.NORM / ACTIVATION) to CONV_DIMS *
2^i and a 1x1 ``pred`` conv (bias, no norm, no activation) to A * (K + 5), on
the MFMA conv kernel.  Inference is one fused op, d2mi_yolov4_inference: the
max-class score of every prediction, the threshold, the decode of the
survivors, class-agnostic NMS and the padding to DETECTIONS_PER_IMAGE.

Training (a head built in the training phase, ``finalize(cfg, True, ...)``):
the tower's BatchNorms run on batch statistics and ``call`` returns the
reference's conf / cls / box losses (yolov4_outputs.py:266-329) from
yolov4_outputs.yolov4_losses -- the fused target assignment and CIoU loss of
csrc/yolo_loss.hip, or the tensor formulation.  The form is fixed when the
head is built: a head built in the inference phase has
neither and refuses ``.train()``.
"""
import torch

from ...layers import Conv2D, Layer, get_norm, ops
from ...layers import initializers as init
from ...layers.normalization import batch_norm_arg_scope, norm_phase
from ...structures import BoxList
from ...utils.arg_scope import arg_scope
from ..anchor_generator import build_anchor_generator
from . import yolov4_outputs
from .build import SINGLE_STAGE_HEADS_REGISTRY
from .yolov4_outputs import YOLOMatcher


class YOLOV4Tower(Layer):
    def __init__(self, cfg, in_channels, num_anchors, **kwargs):
        super().__init__(**kwargs)
        num_classes = cfg.MODEL.SINGLE_STAGE_HEAD.NUM_CLASSES
        conv_dims = cfg.MODEL.YOLOV4.CONV_DIMS
        normalizer = get_norm(cfg.MODEL.YOLOV4.NORM)
        assert len(set(num_anchors)) == 1, \
            "Using different number of anchors between levels is not currently supported!"
        A = num_anchors[0]
        convs, preds = [], []
        with arg_scope([Conv2D], stride=1, normalizer=normalizer,
                       normalizer_params={"scope": "norm"}, use_bias=not normalizer,
                       activation=cfg.MODEL.YOLOV4.ACTIVATION, padding="SAME", impl="auto",
                       weights_initializer=init.random_normal(0.01)), \
                batch_norm_arg_scope(cfg.MODEL.YOLOV4.NORM):  # (training = the phase, no sync)
            for i in range(3):
                head_dims = 2 ** i * conv_dims
                convs.append(Conv2D(in_channels[i], head_dims, 3, scope=f"conv{i + 1}"))
                preds.append(Conv2D(head_dims, A * (num_classes + 5), 1, normalizer=None,
                                    use_bias=True, activation=None, scope=f"pred{i + 1}"))
        self.convs = torch.nn.ModuleList(convs)
        self.preds = torch.nn.ModuleList(preds)

    def call(self, features):
        return [pred(conv(f)) for conv, pred, f in zip(self.convs, self.preds, features)]


@SINGLE_STAGE_HEADS_REGISTRY.register()
class YOLOV4Head(Layer):
    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(**kwargs)
        self.num_classes = cfg.MODEL.SINGLE_STAGE_HEAD.NUM_CLASSES
        self.in_features = list(cfg.MODEL.SINGLE_STAGE_HEAD.IN_FEATURES)
        shapes = [input_shape[f] for f in self.in_features]
        self.in_strides = [s.stride for s in shapes]
        self.in_channels = [s.channels for s in shapes]
        self.anchor_generator = build_anchor_generator(cfg, shapes)
        self.head = YOLOV4Tower(cfg, self.in_channels, self.anchor_generator.num_cell_anchors,
                                scope="head")
        y = cfg.MODEL.YOLOV4
        self.cls_normalizer = y.CLS_NORMALIZER
        self.iou_normalizer = y.IOU_NORMALIZER
        self.score_threshold = y.SCORE_THRESH_TEST
        self.nms_threshold = y.NMS_THRESH_TEST
        self.max_detections_per_image = cfg.TEST.DETECTIONS_PER_IMAGE
        self.scale_yx = list(y.SCALE_YX)
        # the form is fixed here, by the phase batch_norm_arg_scope read for the
        # tower above, never by .training
        self.built_for_training = bool(norm_phase())
        self.matcher = None
        if self.built_for_training:
            self.matcher = YOLOMatcher(cfg.MODEL.SINGLE_STAGE_HEAD.IOU_THRESHOLDS[0])

    def call(self, images, features, targets=None):
        if self.training and not self.built_for_training:
            raise NotImplementedError(
                "this YOLOV4Head was built in the inference phase: its BatchNorms do not run on "
                "batch statistics and neither the YOLOMatcher nor the CIoU loss was constructed; "
                "build the model with finalize(cfg, True, ...) to train")
        pred_logits = self.head([features[f] for f in self.in_features])
        if self.training:
            if targets is None:
                raise ValueError("YOLOv4 training needs targets")
            return None, self.losses(images, pred_logits, targets)
        return self.inference(pred_logits), {}

    def losses(self, images, pred_logits, gt):
        """YOLOV4Outputs.losses (yolov4_outputs.py:266-329).  The GT that count
        are is_valid & ~crowd & ~difficult (:80); the box weight's area is the
        padded batch tensor's (:46, :301)."""
        valid = gt["is_valid"].bool()
        for k in ("gt_is_crowd", "gt_difficult"):
            if gt.get(k) is not None:
                valid = valid & ~gt[k].bool()
        image_hw = tuple(images.tensor.shape[1:3])
        conf, cls, box, _, _ = yolov4_outputs.yolov4_losses(
            pred_logits, self.anchor_generator.strides, self.anchor_generator.cell_anchors,
            self.scale_yx, self.num_classes, gt["gt_boxes"], gt["gt_classes"], valid, image_hw,
            self.matcher.threshold, self.cls_normalizer, self.iou_normalizer)
        return {"conf_loss": conf, "cls_loss": cls, "box_loss": box}

    def inference(self, pred_logits):
        ob, os_, oc, ov = ops.yolov4_inference(
            pred_logits, self.anchor_generator.strides, self.anchor_generator.cell_anchors,
            self.scale_yx, self.num_classes, self.score_threshold, self.nms_threshold,
            self.max_detections_per_image)
        res = BoxList(ob)
        res.add_field("scores", os_)
        res.add_field("pred_classes", oc)
        res.add_field("is_valid", ov)
        return res
