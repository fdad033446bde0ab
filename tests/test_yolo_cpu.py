"""YOLOv4 without a GPU: the numpy restatement (tests/yolo_reference.py)
reproduces its hand-made case, the shipped config builds with the reference's
structure and variable names, the anchor generator follows the reference
formula, training is refused by name, and the host-side checks of the new C
entry points (workspace bound, one byte short, argument errors)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import yolo_reference as yref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
YOLO = "COCO-Detection/yolov4_D_53_PAN_1x.yaml"
LEVELS_608 = [(76, 76), (38, 38), (19, 19)]


def _cfg(edit=None, training=False):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", YOLO))
    if edit is not None:
        edit(cfg)
    return finalize(cfg, training, 1, CATS)


def _build(edit=None, seed=0, training=False):
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = _cfg(edit, training)
    torch.manual_seed(seed)
    try:
        return cfg, build_model(cfg)
    finally:
        from detectron2_tensorflow_amd.utils.training import set_training_phase
        set_training_phase(False)


def test_reference_reproduces_the_hand_made_case():
    case, want = yref.hand_made_case()
    boxes, conf, score, cls, prob = yref.predictions(
        case["logits"], case["strides"], case["cell_hw"], case["scale_yx"], case["num_classes"])
    assert boxes.shape == (1, 18, 4) and prob.shape == (1, 18, 3)
    # the rows the case is about, as its docstring states them
    assert score[0, [0, 1, 3, 6, 12, 15]].tolist() == [1.0, 0.5, 0.5, 0.5, 0.5, 0.25]
    assert cls[0, [0, 1, 3, 6, 12]].tolist() == [2, 1, 0, 2, 0]
    assert prob[0, 12, 0] == prob[0, 12, 1]                      # the class tie
    assert np.array_equal(boxes[0, 0], boxes[0, 1])              # the coincident pair
    assert (np.delete(score[0], [0, 1, 3, 6, 12, 15]) < 1e-6).all()
    got = yref.inference(case["logits"], case["strides"], case["cell_hw"], case["scale_yx"],
                         case["num_classes"], case["thresh"], case["nms_thresh"], case["max_det"])
    for g, k in zip(got, ("boxes", "scores", "classes", "is_valid")):
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), k


def test_reference_spp_counts_the_border_as_zero():
    x = -np.ones((1, 3, 4, 2), np.float32)
    x[0, 1, 1, 0] = -0.5
    out = yref.spp(x)
    assert out.shape == (1, 3, 4, 8)
    # every window of a 3 x 4 map leaves it: the zero border is the maximum
    assert (out[..., :6] == 0).all() and np.array_equal(out[..., 6:], x)
    y = np.zeros((1, 15, 15, 1), np.float32) - 1
    y[0, 7, 7, 0] = 2.0
    o = yref.spp(y)[0, :, :, :3, ...].reshape(15, 15, 3)
    assert o[7, 7].tolist() == [2.0, 2.0, 2.0]
    assert o[7, 4].tolist() == [2.0, 2.0, -1.0]      # 3 away: inside 13 and 9, outside 5
    assert o[7, 2].tolist() == [2.0, 0.0, -1.0]      # 5 away: the 9 window reaches the zero border
    assert o[5, 10, 2] == -1.0                       # a 5 window inside the map, away from the peak


def test_yolov4_config_builds_with_the_reference_structure():
    from detectron2_tensorflow_amd.layers import BatchNorm, Conv2D
    from detectron2_tensorflow_amd.modeling import YOLOAnchorGenerator
    from detectron2_tensorflow_amd.modeling.backbone import DarkNet53
    from detectron2_tensorflow_amd.modeling.necks import YOLOV4
    from detectron2_tensorflow_amd.modeling.single_stage_heads import YOLOV4Head
    cfg, model = _build()
    assert isinstance(model.backbone, DarkNet53) and isinstance(model.neck, YOLOV4)
    assert isinstance(model.detector, YOLOV4Head)
    assert isinstance(model.detector.anchor_generator, YOLOAnchorGenerator)
    assert not model.training

    def convs(m):
        return [c for c in m.modules() if isinstance(c, Conv2D)]

    assert [len(convs(m)) for m in (model.backbone, model.neck, model.detector)] == [72, 32, 6]
    assert sum(isinstance(m, BatchNorm) for m in model.modules()) == 107
    names = {n: tuple(t.shape) for n, t in model.reference_variables(include_scope=False)}
    assert sum(n.endswith("/weights") for n in names) == 110
    assert sum(n.endswith("/norm/gamma") for n in names) == 107
    assert names["backbone/stem/weights"] == (3, 3, 3, 32)
    assert names["backbone/res1/block_1/conv1/weights"] == (1, 1, 64, 32)   # all_narrow=False
    assert names["backbone/res3/block_8/conv2/weights"] == (3, 3, 128, 128)
    assert names["backbone/res5/final/norm/moving_variance"] == (1024,)
    assert names["neck/process1/conv4/norm/gamma"] == (512,)
    assert names["neck/process1/conv4/weights"] == (1, 1, 2048, 512)        # the SPP concat
    assert names["neck/process3/conv2/weights"] == (1, 1, 256, 128)
    assert names["neck/process5/conv1/weights"] == (3, 3, 256, 512)
    assert names["head/head/conv2/weights"] == (3, 3, 256, 512)
    assert names["head/head/pred3/weights"] == (1, 1, 1024, 255)
    assert names["head/head/pred3/bias"] == (255,)
    # pred: bias, no norm, no activation; every other conv: norm, no bias
    for c in convs(model):
        is_pred = c.scope.startswith("pred")
        assert (c.bias is not None) == is_pred and (c.normalizer_fn is None) == is_pred, c.scope
        assert (c.act_fn is None) == is_pred, c.scope
    # FREEZE_AT = 2: the stem, res1 and res2 do not train
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and all(n.startswith(("backbone.stem.", "backbone.stages.0.",
                                        "backbone.stages.1.")) for n in frozen)
    assert all(p.requires_grad for n, p in model.named_parameters()
               if n.startswith(("backbone.stages.2.", "neck.", "detector.")))
    # MODEL.YOLOV4 as the reference has it
    y = cfg.MODEL.YOLOV4
    assert (y.CONV_DIMS, y.NORM, y.ACTIVATION) == (256, "BN", "leaky_relu")
    assert list(y.SCALE_YX) == [1.2, 1.1, 1.05]
    assert (y.CLS_NORMALIZER, y.IOU_NORMALIZER, y.SCORE_THRESH_TEST, y.NMS_THRESH_TEST) == \
        (1.0, 0.07, 0.05, 0.5)
    head = model.detector
    assert (head.score_threshold, head.nms_threshold, head.max_detections_per_image) == (0.05, 0.5, 100)


def test_backbone_and_neck_output_shapes():
    def all_stages(c):
        c.MODEL.RESNETS.OUT_FEATURES = ["res1", "res2", "res3", "res4", "res5"]

    from detectron2_tensorflow_amd.modeling import build_backbone
    shape = build_backbone(_cfg(all_stages)).output_shape()
    assert {k: (v.channels, v.stride) for k, v in shape.items()} == {
        "res1": (64, 2), "res2": (128, 4), "res3": (256, 8), "res4": (512, 16), "res5": (1024, 32)}
    _, model = _build()
    assert {k: (v.channels, v.stride) for k, v in model.backbone.output_shape().items()} == {
        "res3": (256, 8), "res4": (512, 16), "res5": (1024, 32)}
    assert {k: (v.channels, v.stride) for k, v in model.neck.output_shape().items()} == {
        "p3": (128, 8), "p4": (256, 16), "p5": (512, 32)}
    assert model.neck.size_divisibility == 32


def test_yolo_anchor_generator_matches_the_reference_formula():
    _, model = _build()
    ag = model.detector.anchor_generator
    sizes = [[[12, 16], [19, 36], [40, 28]], [[36, 75], [76, 55], [72, 146]],
             [[142, 110], [192, 243], [459, 410]]]
    assert ag.strides == [8, 16, 32] and ag.num_cell_anchors == [3, 3, 3] and ag.box_dim == 4
    for cell, level in zip(ag.cell_anchors, sizes):
        # [0, 0, height, width] for each (width, height): note the swap
        assert cell.tolist() == [[0.0, 0.0, float(h), float(w)] for w, h in level]
    grids = [(3, 2), (2, 2), (1, 1)]
    for got, (H, W), stride, level in zip(ag.grid_anchors(grids, "cpu"), grids, ag.strides, sizes):
        want = np.zeros((H, W, 3, 4), np.float32)
        for a, (w, h) in enumerate(level):
            want[:, :, a, 0] = np.arange(H, dtype=np.float32)[:, None]
            want[:, :, a, 1] = np.arange(W, dtype=np.float32)[None, :]
            want[:, :, a, 2] = np.float32(h) / np.float32(stride)
            want[:, :, a, 3] = np.float32(w) / np.float32(stride)
        assert np.array_equal(got.numpy(), want.reshape(-1, 4))


def test_training_mode_raises_and_names_what_is_missing():
    _, model = _build()
    model.detector.train()
    with pytest.raises(NotImplementedError) as e:
        model.detector(None, {}, None)
    msg = str(e.value)
    assert "batch statistics" in msg and "YOLOMatcher" in msg and "CIoU" in msg


def _lib():
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    return _C, _C.load()


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_workspace_is_linear_and_one_byte_short_is_refused():
    _C, lib = _lib()
    N, A = 4, 3
    lhw = _i32([v for hw in LEVELS_608 for v in hw])
    P = sum(h * w for h, w in LEVELS_608) * A
    assert P == 22743
    size = lib.d2mi_yolov4_workspace_size(N, 3, lhw, A)
    assert 1 < size <= 128 * N * P + 65536, size
    # linear: the batch of 8 costs no more than twice the batch of 4 (plus alignment)
    assert lib.d2mi_yolov4_workspace_size(2 * N, 3, lhw, A) <= 2 * size + 4096
    ws = ctypes.c_void_p(256)  # non-null, never dereferenced: the carve is refused first

    def call(n):
        return lib.d2mi_yolov4_inference(None, lhw, None, None, None, 3, A, 80, N, 0.05, 0.5, 100,
                                         None, None, None, None, ws, n, None)

    rc = call(size - 1)
    msg = _C.last_error()
    assert rc < 0 and "too small" in msg and f"{size - 1} < {size}" in msg, (rc, msg)


def test_host_side_argument_errors_without_gpu():
    _C, lib = _lib()
    lhw = _i32([2, 2] * 9)
    ws = ctypes.c_void_p(256)
    big = 1 << 30

    def inference(L, A, K, max_det=100):
        return lib.d2mi_yolov4_inference(None, lhw, None, None, None, L, A, K, 1, 0.05, 0.5,
                                         max_det, None, None, None, None, ws, big, None)

    def dense(L, A, K):
        return lib.d2mi_yolov4_predictions(None, lhw, None, None, None, L, A, K, 1, None, None,
                                           None, None, None)

    for fn in (inference, dense):
        assert fn(3, 3, 0) < 0 and "K=0" in _C.last_error()
        assert fn(9, 3, 80) < 0 and "L=9" in _C.last_error()         # D2MI_MAX_LEVELS = 8
        assert fn(3, 13, 80) < 0 and "A=13" in _C.last_error()       # kMaxA = 12
        assert fn(3, 3, 80) < 0 and "null" in _C.last_error()        # sizes fine: no host arrays
    assert inference(3, 3, 80, max_det=1001) < 0 and "max_det" in _C.last_error()
    assert lib.d2mi_yolov4_workspace_size(1, 9, lhw, 3) == 0
    assert lib.d2mi_spp_pool(None, 1, 4, 4, 6, None, None) < 0 and "multiple of 4" in _C.last_error()
    assert lib.d2mi_activation(None, 8, 3, 0.1, None) < 0 and "code 3" in _C.last_error()
    assert lib.d2mi_activation(None, 0, 2, 0.0, None) == 0            # nothing to do


def test_activations_keep_the_torch_composition_on_the_cpu():
    from detectron2_tensorflow_amd.layers import get_activation
    x = torch.linspace(-6, 6, 25)
    keep = x.clone()
    assert torch.equal(get_activation("mish")(x), x * torch.tanh(torch.nn.functional.softplus(x)))
    assert torch.equal(get_activation("leaky_relu")(x), torch.nn.functional.leaky_relu(x, 0.1))
    assert torch.equal(x, keep)
