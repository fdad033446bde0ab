from .build import NECK_REGISTRY, DummyNeck, build_neck
from .fpn import FPN, LastLevelMaxPool, LastLevelP6P7
from .yolov4 import SPP, YOLOV4, BottomUp, TopDown

__all__ = ["NECK_REGISTRY", "build_neck", "DummyNeck", "FPN", "LastLevelMaxPool", "LastLevelP6P7",
           "YOLOV4", "SPP", "TopDown", "BottomUp"]
