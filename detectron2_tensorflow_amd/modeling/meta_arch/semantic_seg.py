"""SemanticSegmentor / SemSegFPNHead (lib/modeling/meta_arch/semantic_seg.py:17-221).

SemSegFPNHead: per FPN level p2..p5 a chain of max(1, log2(stride) -
log2(COMMON_STRIDE)) units of 3x3 conv -> GroupNorm(32) -> ReLU, each
followed by a x2 upsample when the level is coarser than COMMON_STRIDE; the
chains are summed and a 1x1 ``predictor`` gives NUM_CLASSES logits at
COMMON_STRIDE.  The reference's Upsample(factor=2, method="bilinear") is the
NEAREST x2 upsample (Upsample.__init__ swallows ``method``,
lib/layers/wrappers.py:104-116), reproduced here.  Without a gradient the
GroupNorm kernel's relu / up2 / accumulate epilogues write every unit's
output upsampled, the last one of a chain straight into the running sum.

The predictor runs on the MFMA conv: its NUM_CLASSES (54) output channels are
padded to a multiple of 4 by constant zero columns appended to the weight and
bias views (the parameters keep the reference shapes), so the head's logits
are rows of ``ldc`` >= NUM_CLASSES floats whose pad channels are 0 and get a
zero gradient.

The final x COMMON_STRIDE resize (resize_images(..., align_corners=True) is
the half-pixel ResizeBilinear: the wrapper drops align_corners, DESIGN
section 9) is never materialised: the head returns the COMMON_STRIDE logits,
the loss is ops.sem_seg_loss (resize + softmax cross-entropy fused, forward
and backward) and the prediction ops.sem_seg_argmax (resize + the zero pad of
sem_seg_postprocess + argmax fused).

Deviations (unbound names in the reference, not behaviours): ``image_shapes``
at :70 and :88 is images.image_shapes; the labels are padded (with the ignore
value) to the image canvas -- the neck's divisibility -- not the backbone's.
batched_inputs["sem_seg"] is [N, H, W] integer labels.
"""
import numpy as np
import torch

from ...layers import Conv2D, GroupNorm, Layer, Sequential, Upsample
from ...layers import initializers as init
from ...layers import ops
from ...layers.conv_weights import Versioned
from ...layers.convolutional import conv_padded_out
from ...utils.arg_scope import arg_scope
from ...utils.registry import Registry
from ..backbone import build_backbone
from ..necks import build_neck
from .build import META_ARCH_REGISTRY
from .rcnn import _Preprocess

SEM_SEG_HEADS_REGISTRY = Registry("SEM_SEG_HEADS")


def build_sem_seg_head(cfg, input_shape, **kwargs):
    return SEM_SEG_HEADS_REGISTRY.get(cfg.MODEL.SEM_SEG_HEAD.NAME)(cfg, input_shape, **kwargs)


@SEM_SEG_HEADS_REGISTRY.register()
class SemSegFPNHead(Layer):
    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(**kwargs)
        h = cfg.MODEL.SEM_SEG_HEAD
        self.in_features = list(h.IN_FEATURES)
        strides = {k: v.stride for k, v in input_shape.items()}
        chans = {k: v.channels for k, v in input_shape.items()}
        self.ignore_value = h.IGNORE_VALUE
        self.num_classes = h.NUM_CLASSES
        dims = h.CONVS_DIM
        self.common_stride = h.COMMON_STRIDE
        self.loss_weight = h.LOSS_WEIGHT
        norm = GroupNorm if h.NORM == "GN" else None
        heads, layers = [], []
        with arg_scope([Conv2D], kernel_size=3, stride=1, padding="SAME", use_bias=norm is None,
                       normalizer=norm,
                       normalizer_params={"num_groups": 32, "scope": "norm"} if norm else None,
                       activation="relu", weights_initializer=init.variance_scaling()):
            for f in self.in_features:
                head = Sequential()
                n = max(1, int(np.log2(strides[f]) - np.log2(self.common_stride)))
                for k in range(n):
                    conv = Conv2D(chans[f] if k == 0 else dims, dims, scope=f"{f}_{2 * k}")
                    layers.append(conv)
                    head.add(conv)
                    if strides[f] != self.common_stride:
                        head.add(Upsample(factor=2, method="bilinear"))
                heads.append(head)
        self.scale_layers = torch.nn.ModuleList(layers)
        self.scale_heads = heads
        self.predictor = Conv2D(dims, self.num_classes, kernel_size=1, stride=1, padding="VALID",
                                use_bias=True, normalizer=None, activation=None,
                                weights_initializer=init.variance_scaling(), scope="predictor")
        padc = (-self.num_classes) % 4
        # constant zero columns for the MFMA predictor (not variables)
        self.register_buffer("_pred_pad_w", torch.zeros(1, 1, dims, padc), persistent=False)
        self.register_buffer("_pred_pad_b", torch.zeros(padc), persistent=False)
        self._pred_pack = Versioned()

    def _merged(self, features):
        """The sum of the scale heads (semantic_seg.py:191-195)."""
        res = None
        for i, f in enumerate(self.in_features):
            x = features[f]
            layers = self.scale_heads[i]._layers
            convs = [m for m in layers if isinstance(m, Conv2D)]
            up = any(isinstance(m, Upsample) for m in layers)
            norm = convs[-1].normalizer_fn
            fusable = (res is not None and isinstance(norm, GroupNorm) and norm.fused_ok(x)
                       and all(c.act_fn is not None for c in convs))
            if not fusable:
                y = self.scale_heads[i](x)
                res = y if res is None else res + y
                continue
            for conv in convs[:-1]:  # GN + ReLU + nearest x2 in one pass
                x = conv.normalizer_fn(conv(x, raw=True), relu=True, up2=up)
            norm(convs[-1](x, raw=True), relu=True, up2=up, accumulate_into=res)
        return res

    def _predict(self, x):
        """[N, h, w, ldc] logits, ldc = NUM_CLASSES padded to a multiple of 4."""
        p = self.predictor
        return conv_padded_out(x, p.weights, p.bias, self._pred_pad_w, self._pred_pad_b,
                               self._pred_pack, 1, (0, 0))

    def call(self, features, targets=None, image_shapes=None):
        """(logits [N, h, w, ldc] at COMMON_STRIDE, losses).  targets
        [N, Hl, Wl] integer labels on the image canvas, image_shapes [N, 2]
        the true shapes (training)."""
        x = self._predict(self._merged(features))
        if not self.training:
            return x, {}
        if targets is None or image_shapes is None:
            raise ValueError("SemSegFPNHead training needs targets and image_shapes")
        loss = ops.sem_seg_loss(x, targets, image_shapes, self.ignore_value, self.common_stride,
                                self.loss_weight, num_classes=self.num_classes)
        return x, {"loss_sem_seg": loss}

    def predictions(self, logits, images, output_format, fixed_resolution):
        """sem_seg_postprocess + tf.argmax (postprocessing.py:62-95,
        semantic_seg.py:81-91): the class map [N, H, W] int64.  "conventional"
        is one fused kernel; "fixed" (crop to the true shape, resize to the
        fixed square: not a hot path, one host read of the shapes) composes
        ops.resize_bilinear with torch.argmax."""
        N, h, w, _ = logits.shape
        s = self.common_stride
        if output_format != "fixed":
            if (h * s, w * s) != tuple(images.tensor.shape[1:3]):
                raise ValueError(f"logits {h}x{w} at stride {s} do not cover the "
                                 f"{tuple(images.tensor.shape[1:3])} canvas")
            return ops.sem_seg_argmax(logits, images.image_shapes, s, self.num_classes)
        full = ops.resize_bilinear(logits[..., :self.num_classes].contiguous(), (h * s, w * s))
        out = []
        for n, (th, tw) in enumerate(images.image_shapes.tolist()):
            crop = full[n:n + 1, :th, :tw].contiguous()
            out.append(ops.resize_bilinear(crop, (fixed_resolution,) * 2).argmax(-1))
        return torch.cat(out)


@META_ARCH_REGISTRY.register()
class SemanticSegmentor(_Preprocess, Layer):
    """semantic_seg.py:24-104: backbone + neck + semantic head."""

    def __init__(self, cfg, **kwargs):
        super().__init__(**kwargs)
        self.backbone = build_backbone(cfg, scope="backbone")
        self.neck = build_neck(cfg, self.backbone.output_shape(), scope="neck")
        self.sem_seg_head = build_sem_seg_head(cfg, self.neck.output_shape(), scope="sem_seg_head")
        self._init_preprocess(cfg)
        self.segmentation_output_format = cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT
        self.segmentation_output_resolution = cfg.MODEL.SEGMENTATION_OUTPUT.FIXED_RESOLUTION

    def call(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        images = self.preprocess_image(batched_inputs)
        features = self.neck(self.backbone(images.tensor))
        _, losses = self.sem_seg_head(features, batched_inputs["sem_seg"], images.image_shapes)
        return losses

    def inference(self, batched_inputs):
        assert not self.training
        images = self.preprocess_image(batched_inputs)
        features = self.neck(self.backbone(images.tensor))
        logits, _ = self.sem_seg_head(features)
        return {"sem_seg": self.sem_seg_head.predictions(
            logits, images, self.segmentation_output_format, self.segmentation_output_resolution)}
