"""YOLOV4Head (lib/modeling/single_stage_heads/yolov4.py:22-170,
yolov4_outputs.py:208-264, :331-390).  Inference only.

Tower: per level a 3x3 conv (MODEL.YOLOV4.NORM / ACTIVATION) to CONV_DIMS *
2^i and a 1x1 ``pred`` conv (bias, no norm, no activation) to A * (K + 5), on
the MFMA conv kernel.  Inference is one fused op, d2mi_yolov4_inference: the
max-class score of every prediction, the threshold, the decode of the
survivors, class-agnostic NMS and the padding to DETECTIONS_PER_IMAGE.

Training is not implemented: the reference's loss (yolov4_outputs.py:266-329)
needs training-mode batch statistics in the neck and head (NORM "BN":
layers.BatchNorm has that form, but these builders build the inference form),
YOLOMatcher and a CIoU loss.
"""
import torch

from ...layers import Conv2D, Layer, get_norm, ops
from ...layers import initializers as init
from ...structures import BoxList
from ...utils.arg_scope import arg_scope
from ..anchor_generator import build_anchor_generator
from .build import SINGLE_STAGE_HEADS_REGISTRY


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
                       weights_initializer=init.random_normal(0.01)):
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

    def call(self, images, features, targets=None):
        if self.training:
            raise NotImplementedError(
                "YOLOv4 training is not implemented: the reference's loss needs training-mode "
                "batch statistics in the neck and head (NORM \"BN\"), YOLOMatcher and a CIoU "
                "loss; this head runs inference only")
        pred_logits = self.head([features[f] for f in self.in_features])
        return self.inference(pred_logits), {}

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
