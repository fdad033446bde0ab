"""CPU tests of the Panoptic FPN family: the config tree, the two
meta-architectures, the semantic head's variable names against the converter's
golden layout, and the new ABI entries (no compute calls without a GPU)."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATEGORY_MAP = {"num_thing_classes": 80, "num_stuff_classes": 54, "stuff_ignore_value": 255}
NEW_SYMBOLS = ("d2mi_sem_seg_loss_workspace_size", "d2mi_sem_seg_loss_fwd", "d2mi_sem_seg_loss_bwd",
               "d2mi_sem_seg_argmax", "d2mi_panoptic_combine_workspace_size",
               "d2mi_panoptic_combine")


def _cfg(meta_arch=None):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(
        ROOT, "configs", "COCO-PanopticSegmentation", "panoptic_fpn_R_50_1x.yaml"))
    if meta_arch is not None:
        cfg.MODEL.META_ARCHITECTURE = meta_arch
    finalize(cfg, training=False, world_size=1, category_map=CATEGORY_MAP)
    return cfg


def test_panoptic_fpn_and_semantic_segmentor_build():
    from detectron2_tensorflow_amd.modeling import (META_ARCH_REGISTRY, SEM_SEG_HEADS_REGISTRY,
                                                    PanopticFPN, SemanticSegmentor, SemSegFPNHead,
                                                    build_model)
    cfg = _cfg()
    c = cfg.MODEL.PANOPTIC_FPN
    assert c.INSTANCE_LOSS_WEIGHT == 1.0 and c.COMBINE.ENABLED is True
    assert c.COMBINE.OVERLAP_THRESH == 0.5 and c.COMBINE.STUFF_AREA_LIMIT == 4096
    assert c.COMBINE.INSTANCES_CONFIDENCE_THRESH == 0.5
    assert cfg.MODEL.SEM_SEG_HEAD.LOSS_WEIGHT == 0.5  # Base-Panoptic-FPN.yaml
    model = build_model(cfg)
    assert type(model) is PanopticFPN and META_ARCH_REGISTRY.get("PanopticFPN") is PanopticFPN
    assert type(model.sem_seg_head) is SemSegFPNHead
    assert SEM_SEG_HEADS_REGISTRY.get("SemSegFPNHead") is SemSegFPNHead
    assert model.combine_stuff_area_limit == 4096 and model.sem_seg_head.num_classes == 54
    seg = build_model(_cfg("SemanticSegmentor"))
    assert type(seg) is SemanticSegmentor
    assert not hasattr(seg, "roi_heads") and type(seg.sem_seg_head) is SemSegFPNHead


def test_panoptic_fpn_refuses_the_raw_mask_format():
    import pytest
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(
        ROOT, "configs", "COCO-PanopticSegmentation", "panoptic_fpn_R_50_1x.yaml"))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    finalize(cfg, training=False, world_size=1, category_map=CATEGORY_MAP)
    with pytest.raises(AssertionError, match="Must transform box masks"):
        build_model(cfg)


def test_sem_seg_head_variables_match_the_converter_layout():
    """Every sem_seg_head/* name the reference's converter emits for a
    PanopticFPN (the panoptic_fpn layout of convert_d2_golden.npz) is a
    variable of the model and the other way round; p2..p5 have 1, 1, 2, 3
    units; a head built at the fixture's sizes has the fixture's shapes."""
    from detectron2_tensorflow_amd.layers import Conv2D, ShapeSpec
    from detectron2_tensorflow_amd.modeling import build_model, build_sem_seg_head
    z = np.load(os.path.join(ROOT, "tests", "golden", "convert_d2_golden.npz"))
    pre = "panoptic_fpn|out|"
    want = {k[len(pre):]: z[k].shape for k in z.files if k.startswith(pre + "sem_seg_head/")}
    assert len(want) == 23
    cfg = _cfg()
    model = build_model(cfg)
    got = {k: tuple(v.shape) for k, v in model.reference_variables(include_scope=False)
           if k.startswith("sem_seg_head/")}
    assert set(got) == set(want), set(got) ^ set(want)
    head = model.sem_seg_head
    units = [sum(isinstance(m, Conv2D) for m in h._layers) for h in head.scale_heads]
    assert head.in_features == ["p2", "p3", "p4", "p5"] and units == [1, 1, 2, 3]
    assert got["sem_seg_head/p2_0/weights"] == (3, 3, 256, 128)
    assert got["sem_seg_head/p5_4/norm/gamma"] == (128,)
    assert got["sem_seg_head/predictor/weights"] == (1, 1, 128, 54)  # unpadded parameters
    assert got["sem_seg_head/predictor/bias"] == (54,)
    # the fixture's sizes: 3 FPN channels, 3 conv channels, 4 classes
    from detectron2_tensorflow_amd.config import get_cfg
    small = get_cfg()
    small.MODEL.SEM_SEG_HEAD.CONVS_DIM = 3
    small.MODEL.SEM_SEG_HEAD.NUM_CLASSES = 4
    shapes = {f"p{l}": ShapeSpec(channels=3, stride=2 ** l) for l in range(2, 7)}
    tiny = build_sem_seg_head(small, shapes, scope="sem_seg_head")
    got = {k: tuple(v.shape) for k, v in tiny.reference_variables()}
    assert got == {k: tuple(v) for k, v in want.items()}


def test_new_symbols_are_exported():
    import torch  # noqa: F401  (binds the HIP runtime torch ships)
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    lib = ctypes.CDLL(_C.LIB_PATH)
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s) or s not in _C.EXPORTED]
    assert not missing, missing
    c = ctypes
    P, I, F, Z = c.c_void_p, c.c_int, c.c_float, c.c_size_t
    loaded = _C.load()
    assert loaded.d2mi_sem_seg_argmax.argtypes == [P, I, I, I, I, I, P, I, P, P]
    assert loaded.d2mi_sem_seg_loss_fwd.argtypes == [P, I, I, I, I, I, P, I, I, P, I, I, F, P, P,
                                                     P, Z, P]
    assert loaded.d2mi_panoptic_combine_workspace_size.restype is Z


def test_short_workspace_is_refused_on_the_host():
    """One byte less than the queried size is refused before any launch, with
    the "too small (have < need)" message of the other ops."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    ws = ctypes.c_void_p(256)  # non-null, never dereferenced: the carve is refused first
    calls = [
        ("sem_seg_loss", lib.d2mi_sem_seg_loss_workspace_size(2, 19, 35),
         lambda n: lib.d2mi_sem_seg_loss_fwd(None, 2, 19, 35, 54, 56, None, 76, 140, None, 255, 4,
                                             1.0, None, None, ws, n, None)),
        ("panoptic_combine", lib.d2mi_panoptic_combine_workspace_size(2, 8, 6),
         lambda n: lib.d2mi_panoptic_combine(None, None, None, None, None, None, 2, 8, 24, 40,
                                             0.5, 20.0, 0.5, 6, None, None, None, None, None,
                                             None, None, None, None, ws, n, None)),
    ]
    for name, size, call in calls:
        assert size > 1, name
        rc = call(size - 1)
        msg = _C.last_error()
        assert rc < 0 and "too small" in msg and f"{size - 1} < {size}" in msg, (name, rc, msg)
        # the full size passes the carve and stops at the null pointers (still no launch)
        rc = call(size)
        assert rc < 0 and "null pointer" in _C.last_error(), (name, rc, _C.last_error())


def test_host_side_argument_errors():
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    rc = lib.d2mi_sem_seg_argmax(None, 1, 4, 4, 57, 56, None, 4, None, None)
    assert rc < 0 and "logits shape" in _C.last_error()
    rc = lib.d2mi_sem_seg_argmax(None, 1, 4, 4, 54, 56, None, 9, None, None)
    assert rc < 0 and "scale" in _C.last_error()
    assert lib.d2mi_sem_seg_loss_workspace_size(0, 4, 4) == 0
