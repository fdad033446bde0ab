"""YOLOv4 neck: SPP + PAN (lib/modeling/necks/yolov4.py:22-291).

Every conv is Conv2D + MODEL.NECK.NORM + MODEL.NECK.ACTIVATION (leaky ReLU,
alpha 0.1) on the MFMA conv kernel with the BatchNorm folded at inference;
built in the training phase the BatchNorms run on batch statistics.
The SPP block's three stride-1 max pools and their concat are one HIP launch
(d2mi_spp_pool) on GPU tensors that need no gradient, the MaxPool2D
composition otherwise.  Concat orders are the reference's: SPP [pool13,
pool9, pool5, x], TopDown [x2, x1], BottomUp [x1, x2].
"""
import math

import torch

from ...layers import Conv2D, Layer, MaxPool2D, ShapeSpec, Upsample, get_norm, ops
from ...layers import initializers as init
from ...layers.normalization import batch_norm_arg_scope
from ...utils.arg_scope import add_arg_scope, arg_scope
from .build import NECK_REGISTRY
from .fpn import assert_strides_are_log2_contiguous


@add_arg_scope
class SPP(Layer):
    # the pools and the concat as one HIP launch (False: MaxPool2D x 3 + cat; tests compare)
    FUSED_POOL = True

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__(in_channels=in_channels, out_channels=out_channels, **kwargs)
        self.conv1 = Conv2D(in_channels, out_channels, 1, scope="conv1")
        self.conv2 = Conv2D(out_channels, out_channels * 2, 3, scope="conv2")
        self.conv3 = Conv2D(out_channels * 2, out_channels, 1, scope="conv3")
        self.maxpool1 = MaxPool2D(kernel_size=13, scope="pool1")
        self.maxpool2 = MaxPool2D(kernel_size=9, scope="pool1")
        self.maxpool3 = MaxPool2D(kernel_size=5, scope="pool1")
        self.conv4 = Conv2D(out_channels * 4, out_channels, 1, scope="conv4")
        self.conv5 = Conv2D(out_channels, out_channels * 2, 3, scope="conv5")
        self.conv6 = Conv2D(out_channels * 2, out_channels, 1, scope="conv6")

    def pool_concat(self, x):
        needs_grad = torch.is_grad_enabled() and x.requires_grad
        if self.FUSED_POOL and x.is_cuda and not needs_grad and x.shape[-1] % 4 == 0:
            return ops.spp_pool(x)
        return torch.cat([self.maxpool1(x), self.maxpool2(x), self.maxpool3(x), x], dim=3)

    def call(self, x):
        x = self.conv3(self.conv2(self.conv1(x)))
        x = self.pool_concat(x)
        return self.conv6(self.conv5(self.conv4(x)))


@add_arg_scope
class TopDown(Layer):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__(in_channels=in_channels, out_channels=out_channels, **kwargs)
        self.conv1 = Conv2D(out_channels * 2, out_channels, 1, scope="conv1")
        self.upsample = Upsample(2)
        self.conv2 = Conv2D(in_channels, out_channels, 1, scope="conv2")
        self.conv3 = Conv2D(out_channels * 2, out_channels, 1, scope="conv3")
        self.conv4 = Conv2D(out_channels, out_channels * 2, 3, scope="conv4")
        self.conv5 = Conv2D(out_channels * 2, out_channels, 1, scope="conv5")
        self.conv6 = Conv2D(out_channels, out_channels * 2, 3, scope="conv6")
        self.conv7 = Conv2D(out_channels * 2, out_channels, 1, scope="conv7")

    def call(self, x1, x2):
        x1 = self.upsample(self.conv1(x1))
        x2 = self.conv2(x2)
        x = torch.cat([x2, x1], dim=3)
        return self.conv7(self.conv6(self.conv5(self.conv4(self.conv3(x)))))


@add_arg_scope
class BottomUp(Layer):
    def __init__(self, out_channels, **kwargs):
        super().__init__(out_channels=out_channels, **kwargs)
        self.conv1 = Conv2D(out_channels // 2, out_channels, 3, stride=2, scope="conv1")
        self.conv2 = Conv2D(out_channels * 2, out_channels, 1, scope="conv2")
        self.conv3 = Conv2D(out_channels, out_channels * 2, 3, scope="conv3")
        self.conv4 = Conv2D(out_channels * 2, out_channels, 1, scope="conv4")
        self.conv5 = Conv2D(out_channels, out_channels * 2, 3, scope="conv5")
        self.conv6 = Conv2D(out_channels * 2, out_channels, 1, scope="conv6")

    def call(self, x1, x2):
        x = torch.cat([self.conv1(x1), x2], dim=3)
        return self.conv6(self.conv5(self.conv4(self.conv3(self.conv2(x)))))


@NECK_REGISTRY.register()
class YOLOV4(Layer):
    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(**kwargs)
        self.in_features = list(cfg.MODEL.NECK.IN_FEATURES)
        assert len(self.in_features) == 3, self.in_features
        self.in_strides = [input_shape[f].stride for f in self.in_features]
        self.in_channels = [input_shape[f].channels for f in self.in_features]
        assert_strides_are_log2_contiguous(self.in_strides)
        self.out_channels = cfg.MODEL.NECK.OUT_CHANNELS
        self.norm = cfg.MODEL.NECK.NORM
        self.activation = cfg.MODEL.NECK.ACTIVATION
        c = self.out_channels
        with arg_scope([Conv2D], use_bias=self.norm == "", normalizer=get_norm(self.norm),
                       normalizer_params={"scope": "norm"}, activation=self.activation,
                       impl="auto", weights_initializer=init.variance_scaling(1.0)), \
                batch_norm_arg_scope(self.norm):  # (BN / SyncBN: training = the phase, no sync)
            self.process1 = SPP(self.in_channels[2], c * 4, scope="process1")
            self.process2 = TopDown(self.in_channels[1], c * 2, scope="process2")
            self.process3 = TopDown(self.in_channels[0], c, scope="process3")
            self.process4 = BottomUp(c * 2, scope="process4")
            self.process5 = BottomUp(c * 4, scope="process5")
        self._out_feature_strides = {f"p{int(math.log2(s))}": s for s in self.in_strides}
        self._out_features = sorted(self._out_feature_strides)
        self._out_feature_channels = {f: 2 ** i * c for i, f in enumerate(self._out_features)}
        self._size_divisibility = self.in_strides[-1]

    @property
    def size_divisibility(self):
        return self._size_divisibility

    def call(self, bottom_up_features):
        c3, c4, c5 = [bottom_up_features[f] for f in self.in_features]
        l5 = self.process1(c5)
        l4 = self.process2(l5, c4)
        l3 = self.process3(l4, c3)
        l4 = self.process4(l3, l4)
        l5 = self.process5(l4, l5)
        return dict(zip(self._out_features, [l3, l4, l5]))

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n],
                             stride=self._out_feature_strides[n]) for n in self._out_features}
