"""RelationBoxHead / RelationRoiHeads (lib/modeling/roi_heads/relation_network.py:14-87).

Relation Networks for Object Detection on the Fast R-CNN box head: one
ObjectRelationModule ``r{k+1}`` after each ``fc{k+1}``, so every proposal's
feature is updated from all proposals of its image.  RelationRoiHeads is
StandardROIHeads with the proposals handed to the box head; the predictor,
the losses, inference and the mask branch are unchanged.

ROI_BOX_RELATION_HEAD.DUPLICATE_REMOVAL_IOU, RANK_EMBEDDING_DIM and
NMS_NUM_GROUP are read by nothing in the reference (its duplicate-removal
network was never written); they are loaded and unused here too.
"""
import torch

from .box_head import ROI_BOX_HEAD_REGISTRY, FastRCNNConvFCHead
from .relation_module import ObjectRelationModule
from .roi_heads import ROI_HEADS_REGISTRY, StandardROIHeads


@ROI_BOX_HEAD_REGISTRY.register()
class RelationBoxHead(FastRCNNConvFCHead):
    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(cfg, input_shape, **kwargs)
        h = cfg.MODEL.ROI_BOX_HEAD
        r = cfg.MODEL.ROI_BOX_RELATION_HEAD
        self.geometry_embedding_dim = r.GEOMETRY_EMBEDDING_DIM
        self.relations = torch.nn.ModuleList(
            ObjectRelationModule(input_size=h.FC_DIM, embedding_dim=r.GEOMETRY_EMBEDDING_DIM,
                                 key_dim=r.KEY_DIM, num_groups=r.NUM_GROUPS, scope=f"r{k + 1}")
            for k in range(h.NUM_FC))

    def call(self, x, boxes, valid):
        """x: the pooled rows of boxes [N, P, 4] / valid [N, P], image-major."""
        for layer in self.convs:
            x = layer(x)
        if len(self.fcs):
            if x.dim() > 2:
                x = x.reshape(x.shape[0], -1)
            for fc, relation in zip(self.fcs, self.relations):
                x = relation(fc(x), boxes, valid)
        return x


@ROI_HEADS_REGISTRY.register()
class RelationRoiHeads(StandardROIHeads):
    def _box_features(self, x, boxes, valid):
        return self.box_head(x, boxes, valid)
