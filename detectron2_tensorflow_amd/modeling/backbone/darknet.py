"""CSPDarkNet53 backbone (lib/modeling/backbone/darknet.py:14-249).

Every conv is Conv2D + BatchNorm + activation (MODEL.RESNETS.ACTIVATION,
"mish" by default).  Built in the training phase, the BatchNorms of the stages
that train run on batch statistics (layers/normalization.py); otherwise, and
in the frozen stages, BatchNorm folds into the weights
(Conv2D.effective_params) and the convs run on the MFMA implicit-GEMM kernel;
the 3-channel stem stays on the "auto" path.  The activation follows as one
in-place HIP pass (layers/activation.py).  Scopes, stage widths
(RES2_OUT_CHANNELS * 2^i, the reference's name for res1's width) and FREEZE_AT
follow the reference.
"""
from contextlib import ExitStack, contextmanager

import torch

from ...layers import BatchNorm, Conv2D, Layer, get_norm
from ...layers import initializers as init
from ...layers.normalization import batch_norm_arg_scope
from ...utils.arg_scope import add_arg_scope, arg_scope
from .build import BACKBONE_REGISTRY, Backbone


@contextmanager
def darknet_arg_scope(freeze, norm, activation):
    with arg_scope([Conv2D], use_bias=False, normalizer=get_norm(norm),
                   normalizer_params={"scope": "norm"}, activation=activation, impl="auto",
                   weights_initializer=init.variance_scaling(2.0, mode="fan_out")), ExitStack() as st:
        # a frozen stage: the inference form; a stage that trains: batch
        # statistics in the training phase (lib/modeling/backbone/darknet.py:14-32)
        st.enter_context(batch_norm_arg_scope(norm, freeze=freeze))
        if freeze:
            st.enter_context(arg_scope([Conv2D, BatchNorm], trainable=False))
        yield


@add_arg_scope
class DarkNetResidualBlock(Layer):
    def __init__(self, in_channels, out_channels, bottleneck_channels, **kwargs):
        assert in_channels == out_channels, (in_channels, bottleneck_channels, out_channels)
        super().__init__(in_channels=in_channels, out_channels=out_channels,
                         bottleneck_channels=bottleneck_channels, **kwargs)
        self.conv1 = Conv2D(in_channels, bottleneck_channels, 1, scope="conv1")
        self.conv2 = Conv2D(bottleneck_channels, out_channels, 3, scope="conv2")

    def call(self, x):
        return x + self.conv2(self.conv1(x))


@add_arg_scope
class DarkNetStage(Layer):
    """darknet.py:84-160: a stride-2 3x3, the cross-stage split (shortcut /
    main), num_blocks residual blocks on the main path, and the 1x1 that
    merges concat([post, shortcut])."""

    def __init__(self, in_channels, out_channels, num_blocks, all_narrow=True, **kwargs):
        super().__init__(in_channels=in_channels, out_channels=out_channels,
                         num_blocks=num_blocks, all_narrow=all_narrow, **kwargs)
        self.preconv = Conv2D(in_channels, out_channels, 3, stride=2, scope="preconv")
        block_channels = out_channels // 2 if all_narrow else out_channels
        bottleneck_channels = block_channels if all_narrow else block_channels // 2
        self.shortcut = Conv2D(out_channels, block_channels, 1, scope="shortcut")
        self.main = Conv2D(out_channels, block_channels, 1, scope="main")
        self.blocks = torch.nn.ModuleList(
            DarkNetResidualBlock(block_channels, block_channels, bottleneck_channels,
                                 scope=f"block_{i + 1}") for i in range(num_blocks))
        self.postconv = Conv2D(block_channels, block_channels, 1, scope="postconv")
        self.final = Conv2D(block_channels * 2, out_channels, 1, scope="final")

    def call(self, x):
        pre = self.preconv(x)
        shortcut = self.shortcut(pre)
        residual = self.main(pre)
        for block in self.blocks:
            residual = block(residual)
        post = self.postconv(residual)
        return self.final(torch.cat([post, shortcut], dim=3))


@BACKBONE_REGISTRY.register()
class DarkNet53(Backbone):
    def __init__(self, cfg, input_shape, **kwargs):
        super().__init__(**kwargs)
        r = cfg.MODEL.RESNETS
        norm, activation = r.NORM, r.ACTIVATION
        freeze_at = cfg.MODEL.BACKBONE.FREEZE_AT
        self._out_features = list(r.OUT_FEATURES)
        stages = {"res1": 1, "res2": 2, "res3": 3, "res4": 4, "res5": 5}
        max_stage_idx = max(stages[f] for f in self._out_features)
        num_blocks_per_stage = [1, 2, 8, 8, 4]
        with darknet_arg_scope(freeze_at > 0, norm, activation):
            self.stem = Conv2D(input_shape.channels, r.STEM_OUT_CHANNELS, 3, scope="stem")
        stride = 1
        self._out_feature_strides = {"stem": stride}
        self._out_feature_channels = {"stem": r.STEM_OUT_CHANNELS}
        in_ch, out_ch = r.STEM_OUT_CHANNELS, r.RES2_OUT_CHANNELS
        self.stages = torch.nn.ModuleList()
        self.stage_names = []
        for idx, stage_idx in enumerate(range(1, max_stage_idx + 1)):
            name = f"res{stage_idx}"
            with darknet_arg_scope(freeze_at >= stage_idx, norm, activation):
                self.stages.append(DarkNetStage(in_ch, out_ch, num_blocks_per_stage[idx],
                                                all_narrow=stage_idx != 1, scope=name))
            self.stage_names.append(name)
            stride *= 2
            self._out_feature_strides[name] = stride
            self._out_feature_channels[name] = out_ch
            in_ch, out_ch = out_ch, out_ch * 2

    def call(self, x):
        outputs = {}
        x = self.stem(x)
        if "stem" in self._out_features:
            outputs["stem"] = x
        for name, stage in zip(self.stage_names, self.stages):
            x = stage(x)
            if name in self._out_features:
                outputs[name] = x
        assert len(outputs) == len(self._out_features), list(outputs)
        return outputs
