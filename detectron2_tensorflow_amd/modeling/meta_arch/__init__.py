from .build import META_ARCH_REGISTRY, build_model
from .rcnn import GeneralizedRCNN, ProposalNetwork
from .single_stage_detector import SingleStageDetector
from .semantic_seg import (SEM_SEG_HEADS_REGISTRY, SemanticSegmentor, SemSegFPNHead,
                           build_sem_seg_head)
from .panoptic_fpn import PanopticFPN

__all__ = ["META_ARCH_REGISTRY", "build_model", "GeneralizedRCNN", "ProposalNetwork",
           "SingleStageDetector", "SEM_SEG_HEADS_REGISTRY", "SemanticSegmentor", "SemSegFPNHead",
           "build_sem_seg_head", "PanopticFPN"]
