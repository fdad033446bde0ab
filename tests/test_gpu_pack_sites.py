"""No site that keeps a packed copy of its weights (layers/conv_weights.py:
Versioned) serves a stale one: after the in-place update an optimizer makes,
the forward equals that of a freshly built layer holding the updated weights.
(Conv2D inside a PackGroup: test_pack_weights_many_and_pack_group.)"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu


def _conv2d():
    from detectron2_tensorflow_amd.layers import Conv2D
    make = lambda: Conv2D(8, 8, 3, impl="mfma", scope="conv")
    return make, lambda m, x: m(x), lambda m: [m.weights], (1, 8, 8, 8), True


def _deform(which):
    from detectron2_tensorflow_amd.layers import DeformConv2D
    make = lambda: DeformConv2D(8, 8, 3, scope="dconv")
    moved = lambda m: [m.offset_weights if which == "offset" else m.weights]
    # (grad off: the column conv's packed copy is cached for constant weights only)
    return make, lambda m, x: m(x), moved, (1, 8, 8, 8), False


def _sem_seg_predictor():
    from detectron2_tensorflow_amd.config import get_cfg
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling import build_sem_seg_head
    cfg = get_cfg()
    h = cfg.MODEL.SEM_SEG_HEAD
    h.CONVS_DIM, h.NUM_CLASSES, h.NORM = 8, 6, ""  # 6 classes: padded to 8 columns
    shapes = {f"p{l}": ShapeSpec(channels=8, stride=2 ** l) for l in range(2, 6)}
    make = lambda: build_sem_seg_head(cfg, shapes, scope="sem_seg_head")
    return make, lambda m, x: m._predict(x), lambda m: [m.predictor.weights], (1, 8, 8, 8), True


def _linear():
    from detectron2_tensorflow_amd.layers import Linear
    assert Linear.MFMA_MIN_K == 4096
    make = lambda: Linear(4096, 8, scope="fc")
    return make, lambda m, x: m(x), lambda m: [m.weights], (4, 4096), True


def _rpn_head():
    from detectron2_tensorflow_amd.config import get_cfg
    from detectron2_tensorflow_amd.layers import ShapeSpec
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import StandardRPNHead
    cfg = get_cfg()
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[32]]  # x 3 aspect ratios: 3 anchors, a 16-wide 1x1

    def make():
        head = StandardRPNHead(cfg, [ShapeSpec(channels=8, stride=16)])
        assert head.A == 3
        return head

    def run(m, x):
        _, logits, deltas = m([x])
        return torch.cat([logits[0], deltas[0]], 3)

    # every one of the four tensors the fused 1x1 is made of
    moved = lambda m: [m.objectness_logits.weights, m.anchor_deltas.weights,
                       m.objectness_logits.bias, m.anchor_deltas.bias]
    return make, run, moved, (1, 8, 8, 8), True


SITES = {
    "conv2d": _conv2d,
    "deform_offset_conv": lambda: _deform("offset"),
    "deform_column_conv": lambda: _deform("cols"),
    "sem_seg_predictor": _sem_seg_predictor,
    "linear": _linear,
    "rpn_head_fused_1x1": _rpn_head,
}


@pytest.mark.parametrize("site", SITES)
def test_no_packing_site_serves_a_stale_copy(dev, site):
    make, run, moved, x_shape, with_grad = SITES[site]()
    g = torch.Generator().manual_seed(5)
    layer = make().to(dev)
    with torch.no_grad():  # (zero-initialised offset weights / biases would hide an update)
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    x = torch.randn(x_shape, generator=g).to(dev)
    with contextlib.nullcontext() if with_grad else torch.no_grad():
        before = run(layer, x)
        for _ in range(2):  # two steps: the second update finds a filled cache
            with torch.no_grad():
                for p in moved(layer):
                    p.add_(torch.randn(p.shape, generator=g).to(dev) * 0.1)
            got = run(layer, x)
        fresh = make().to(dev)
        fresh.load_state_dict(layer.state_dict())
        want = run(fresh, x)
    assert not torch.equal(got, before)  # (the update moves the output at all)
    assert torch.equal(got, want)
