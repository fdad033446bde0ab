from .box_head import ROI_BOX_HEAD_REGISTRY, FastRCNNConvFCHead, build_box_head
from .fast_rcnn import FastRCNNOutputLayers
from .mask_head import ROI_MASK_HEAD_REGISTRY, MaskRCNNConvUpsampleHead, build_mask_head, mask_rcnn_inference
from .roi_heads import ROI_HEADS_REGISTRY, ROIHeads, StandardROIHeads, build_roi_heads
from .res5_heads import Res5ROIHeads
from .cascade_rcnn import CascadeROIHeads
from .relation_module import ObjectRelationModule, relation_dense
from .relation_network import RelationBoxHead, RelationRoiHeads

__all__ = ["ObjectRelationModule", "relation_dense", "RelationBoxHead", "RelationRoiHeads","ROI_BOX_HEAD_REGISTRY", "FastRCNNConvFCHead", "build_box_head", "FastRCNNOutputLayers",
           "ROI_MASK_HEAD_REGISTRY", "MaskRCNNConvUpsampleHead", "build_mask_head",
           "mask_rcnn_inference", "ROI_HEADS_REGISTRY", "ROIHeads", "StandardROIHeads",
           "build_roi_heads", "CascadeROIHeads", "Res5ROIHeads"]
