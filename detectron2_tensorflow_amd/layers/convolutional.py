"""Conv2D / ConvTranspose2D with the reference's constructor surface
(lib/layers/convolutional.py:119-263, :747-893).

Activations are NHWC, weights are HWIO ``[k, k, in/groups, out]`` (the
reference variable layout; ConvTranspose2D keeps TF's ``[k, k, out, in]``).
``impl="mfma"`` runs the forward pass on the hand-written gfx950 MFMA
implicit-GEMM kernel (d2mi_conv2d_nhwc) — the FPN lateral/output convs, the
RPN head and the mask head use it — and raises if the tensor is not on the GPU.
``impl="torch"`` is stock PyTorch-ROCm conv2d in channels_last, used for the
backbone (a caller of the hot path, outside its scope).
``impl="auto"`` picks mfma when the shape is eligible (no groups/dilation,
Cin % 4 == 0) and the input is on the GPU; ``impl="mfma"`` with Cin % 4 != 0
runs with zero channels appended.
The MFMA conv itself, with its backward, is layers/conv_grad.py (conv_mfma);
the packed / folded weight copies are kept by layers/conv_weights.py.
"""

import torch
import torch.nn.functional as F

from ..utils.arg_scope import add_arg_scope
from . import handoff
from . import initializers as init
from . import ops
from .activation import get_activation, is_relu
from .base import Layer
from .conv_grad import conv_mfma
from .conv_weights import PackGroup, Versioned, _foldable_bn, version_key
from .normalization import BatchNorm


def epilogue(y, norm, act_fn, *, allow_fused_gn, fused_relu=False, final_relu=False):
    """What follows a conv (+ bias): the normalizer, then the activation and
    final_relu (the ReLU of a layer without one) unless the conv fused them
    (fused_relu).  allow_fused_gn: GroupNorm + ReLU as one HIP pass where the
    normalizer can (fused_ok, or train_fused_ok where it has one: the training
    kernels); only Conv2D's MFMA sites take it."""
    if final_relu and act_fn is not None:
        raise ValueError("final_relu is for layers without an activation")
    if norm is not None:
        if allow_fused_gn and is_relu(act_fn) and hasattr(norm, "fused_ok") and (
                norm.fused_ok(y) or (hasattr(norm, "train_fused_ok") and norm.train_fused_ok(y))):
            return norm(y, relu=True)
        y = norm(y)
    if act_fn is not None and not fused_relu:
        y = act_fn(y)
    if final_relu and not fused_relu:
        y = torch.relu(y)
    return y


def fix_padding(inputs, kernel_size, padding="SAME", rate=1):
    """Explicit symmetric 'SAME' padding (convolutional.py:12-23): NHWC zero pad."""
    if padding == "SAME" and kernel_size != 1:
        pb, pe = same_pads(kernel_size, rate)
        inputs = F.pad(inputs, (0, 0, pb, pe, pb, pe))
    return inputs


def same_pads(kernel_size, rate=1):
    k_eff = kernel_size + (kernel_size - 1) * (rate - 1)
    pad_total = k_eff - 1
    pb = pad_total // 2
    return pb, pad_total - pb


def _normalizer(normalizer, params, channels):
    return None if normalizer is None else normalizer(**dict(params or {}, channels=channels))


def conv_padded_out(x, w, b, pad_w, pad_b, cache, stride, pads):
    """conv_mfma of x with (w, b) and the constant zero output columns (pad_w,
    pad_b) that bring Cout to a multiple of 4; packed once per version of w."""
    key = version_key((w,))
    if pad_b.numel():
        w, b = torch.cat([w, pad_w], 3), torch.cat([b, pad_b])
    packed = cache.get(key, lambda: ops.pack_conv_weights(w.detach()))
    return conv_mfma(x, w, b, packed, stride, pads, relu=False)


@add_arg_scope
class Conv2D(Layer):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding="SAME", rate=1,
                 num_groups=1, use_bias=True, activation=None, normalizer=None,
                 normalizer_params=None, weights_initializer=None, weights_regularizer=None,
                 bias_initializer=None, bias_regularizer=None, variables_collections=None,
                 trainable=True, outputs_collections=None, impl="mfma", **kwargs):
        padding = padding.upper()
        if padding not in ("SAME", "VALID"):
            raise ValueError('"padding" must be "SAME" or "VALID."')
        if in_channels % num_groups != 0:
            raise ValueError(f'"in_channels" {in_channels} is not divisible by "num_groups" {num_groups}.')
        if out_channels % num_groups != 0:
            raise ValueError(f'"out_channels" {out_channels} is not divisible by "num_groups" {num_groups}.')
        super().__init__(in_channels=in_channels, out_channels=out_channels,
                         kernel_size=kernel_size, stride=stride, padding=padding, rate=rate,
                         num_groups=num_groups, use_bias=use_bias, activation=activation,
                         normalizer=normalizer, normalizer_params=normalizer_params,
                         weights_initializer=weights_initializer,
                         weights_regularizer=weights_regularizer,
                         bias_initializer=bias_initializer, bias_regularizer=bias_regularizer,
                         trainable=trainable, impl=impl, **kwargs)
        self.build()

    def build(self):
        shape = (self.kernel_size, self.kernel_size, self.in_channels // self.num_groups,
                 self.out_channels)
        w = torch.empty(shape, dtype=torch.float32)
        (self.weights_initializer or init.variance_scaling(2.0, distribution="untruncated_normal"))(w)
        self.weights = torch.nn.Parameter(w, requires_grad=self.trainable)
        if self.use_bias:
            b = torch.zeros(self.out_channels)
            if self.bias_initializer is not None:
                self.bias_initializer(b)
            self.bias = torch.nn.Parameter(b, requires_grad=self.trainable)
        else:
            self.bias = None
        self.normalizer_fn = _normalizer(self.normalizer, self.normalizer_params, self.out_channels)
        # a plain attribute: the one check of every call (no module lookup)
        object.__setattr__(self, "_bn_batch_stats",
                           bool(getattr(self.normalizer_fn, "batch_stats", False)))
        self.act_fn = get_activation(self.activation)
        self._pack = Versioned()  # the packed weights (packed_weights)
        self._fold = Versioned()  # the constant FrozenBN fold (effective_params)

    def _mfma_eligible(self, x, padded=False):
        # impl="mfma" with Cin % 4 != 0 (e.g. SOLOv2's 256 + 2 coordinate
        # channels) runs with zero channels appended to the input and the
        # weights (exact: the extra products are 0); "auto" keeps such convs
        # (the 3-channel stem) on MIOpen
        return (x.is_cuda and self.num_groups == 1 and self.rate == 1
                and (padded or self.in_channels % 4 == 0))

    def _key_tensors(self):
        """(weights, the other tensors the fold reads), looked up once (the
        module attribute lookups are host time on every conv call)."""
        kt = self.__dict__.get("_key_ts")
        w = self.weights
        # (re-looked up when the weights move: .to() / .cuda() also replace
        # the normalizer's buffers)
        if kt is None or kt[0] is not w or kt[2] != w.data_ptr():
            rest = [self.bias] if self.bias is not None else []
            if _foldable_bn(self.normalizer_fn):
                n = self.normalizer_fn
                rest += [t for t in (n.gamma, n.beta, n.moving_mean, n.moving_variance)
                         if t is not None]
            kt = self.__dict__["_key_ts"] = (w, tuple(rest), w.data_ptr())
        return kt

    def _param_key(self):
        w, rest, _ = self._key_tensors()
        return (w.data_ptr(), w._version) + tuple(t._version for t in rest)

    def _pack_key(self, w):
        return self._param_key() + (tuple(w.shape),)

    def effective_params(self, want_packed=False):
        """(weights HWIO, bias, normalizer still to apply, packed-or-None) with a
        frozen BatchNorm folded in by one fused HIP kernel (d2mi_fold_frozen_bn,
        differentiable w.r.t. weights / bias / gamma / beta).  Cached while
        autograd is off (inference).  A BatchNorm on batch statistics is not
        folded: it is the normalizer still to apply."""
        norm = self.normalizer_fn
        if not _foldable_bn(norm):
            return self.weights, self.bias, norm, None
        if not self.weights.is_cuda:
            raise RuntimeError(f"{self.scope}: the FrozenBN fold runs on the GPU (HIP)")
        # constant while autograd is off or nothing in the fold trains (the
        # layers below FREEZE_AT): cached per parameter version
        cacheable = not (torch.is_grad_enabled() and self.fold_trainable())
        group = self.__dict__.get("_fold_group")
        if not cacheable and group is not None:  # (the group checks the versions itself)
            got = group.fetch(self)
            if got is not None:
                return got[0], got[1], None, got[2]

        def fold():
            return ops.fold_frozen_bn(self.weights, self.bias, norm.gamma, norm.beta,
                                      norm.moving_mean, norm.moving_variance, norm.epsilon,
                                      want_packed)

        w, b, packed = self._fold.get(self._param_key(), fold) if cacheable else fold()
        return w, b, None, packed

    def fold_trainable(self):
        norm = self.normalizer_fn
        ts = (self.weights, self.bias) + ((norm.gamma, norm.beta) if _foldable_bn(norm) else ())
        return any(t is not None and t.requires_grad for t in ts)

    def wants_packed(self):
        return (self.impl in ("mfma", "auto") and self.num_groups == 1 and self.rate == 1
                and self.in_channels % 4 == 0)

    def packed_weights(self, w_eff=None):
        group = self.__dict__.get("_pack_group")
        if group is not None and PackGroup.ENABLED and (w_eff is None or w_eff is self.weights):
            return group.fetch(self)
        w = self.weights if w_eff is None else w_eff
        # the packed tensor's own shape is part of the key: a Cin-padded w_eff
        # (Cin % 4 != 0) packs to [.., Cout, Cin + pad], never to be returned
        # for the layer's own weights (or the other way round)
        return self._pack.get(self._pack_key(w), lambda: ops.pack_conv_weights(w.detach()))

    def call_levels(self, inputs):
        """This layer applied to each of ``inputs`` (feature levels sharing the
        layer, as the reference's per-level head calls do), as ONE multi-level
        MFMA launch (ops.conv2d_nhwc_levels) when nothing needs a gradient;
        per-level calls otherwise.  The normalizer / activation follow per
        level (GroupNorm + ReLU fused where it can be)."""
        padded = self.impl == "mfma"  # explicit MFMA: Cin padded to a multiple of 4
        ok = (not torch.is_grad_enabled() and self.impl in ("mfma", "auto") and len(inputs) <= 6
              and all(self._mfma_eligible(x, padded) for x in inputs)
              and not isinstance(self.normalizer_fn, BatchNorm))
        if not ok:
            return [self(x) for x in inputs]
        w, b, norm, packed = self.effective_params(want_packed=True)
        padc = (-self.in_channels) % 4
        if padc:
            inputs = [F.pad(x, (0, padc)) for x in inputs]
            w = F.pad(w, (0, 0, 0, padc))
            packed = None
        if packed is None:
            packed = self.packed_weights(w)
        pads = same_pads(self.kernel_size, self.rate) if self.padding == "SAME" else (0, 0)
        fuse_relu = norm is None and is_relu(self.act_fn)
        ys = ops.conv2d_nhwc_levels(inputs, packed, b, self.stride, pads, relu=fuse_relu)
        if (norm is not None and is_relu(self.act_fn) and hasattr(norm, "fused_ok")
                and all(norm.fused_ok(y) for y in ys)):
            # GroupNorm + ReLU over every level in one set of launches
            return ops.group_norm_levels(ys, norm.num_groups, norm.gamma, norm.beta, norm.epsilon,
                                         relu=True)
        return [epilogue(y, norm, self.act_fn, fused_relu=fuse_relu, allow_fused_gn=True)
                for y in ys]

    def call(self, inputs, topdown=None, residual=None, relu_after_add=False, final_relu=False,
             relu_input_sole_consumer=False, res_grad_to=None, grad_from=None, pair_grad=None,
             raw=False, join=None, wacc=None, rows=None):
        """topdown: fused + up2(topdown) (FPN merge); residual: fused + residual;
        relu_after_add: the layer's ReLU runs after those adds; final_relu: an
        extra ReLU after the adds for a layer without activation (the
        bottleneck's relu(conv3(x) + shortcut), blocks.py:143-186).
        relu_input_sole_consumer, res_grad_to / grad_from (a handoff.Slot),
        pair_grad / join (a handoff.Pair), wacc (a handoff.LevelAccumulator),
        rows ((handoff.RowBound, level) of the output's gradient): the gradient
        hand-offs of layers/handoff.py."""
        if self._bn_batch_stats:
            if res_grad_to is not None or grad_from is not None:
                raise ValueError(f"{self.scope}: res_grad_to / grad_from cannot be honoured under "
                                 "a BatchNorm on batch statistics (the conv runs without gradient "
                                 "hand-offs: the Slot's gradient would be lost)")
            return self._call_batch_stats(inputs, topdown, residual, relu_after_add, final_relu, raw)
        impl = self._pick_impl(inputs)
        w, b, norm, packed = self.effective_params(want_packed=(impl == "mfma"))
        if final_relu:
            if self.act_fn is not None:
                raise ValueError("final_relu is for layers without an activation")
            if impl == "torch":
                return torch.relu_(self.call(inputs, topdown, residual))
        if impl == "mfma":
            fuse_relu = norm is None and (is_relu(self.act_fn) or final_relu)
            relu_after_add = relu_after_add or final_relu
            if (topdown is not None or residual is not None) and fuse_relu and not relu_after_add:
                raise ValueError("relu(conv) + add cannot be fused; use relu_after_add")
            if join is not None:
                if self.in_channels % 4 or not torch.is_grad_enabled():
                    join = None  # (a padded input is another tensor: no join)
                else:
                    join.join_lateral()  # the pair members now leave their sum to this layer
            inputs, w, packed, pads = self._mfma_operands(inputs, w, packed)
            links = handoff.Links(bool(relu_input_sole_consumer), res_grad_to, grad_from,
                                  pair_grad, join, wacc, rows)
            ret = conv_mfma(inputs, w, b, packed, self.stride, pads, fuse_relu, topdown, residual,
                            relu_after_add, links)
            if raw:  # the conv (+ bias) alone: the caller applies the normalizer / activation
                return ret
            return epilogue(ret, norm, self.act_fn, fused_relu=fuse_relu, final_relu=final_relu,
                            allow_fused_gn=True)
        # torch (channels_last) path: backbone 3x3 convs / the stem
        has_add = topdown is not None or residual is not None
        # (an activation after the adds follows below; GN and ReLU stay two passes)
        ret = epilogue(self._conv_torch(inputs, w, b), norm,
                       None if has_add and relu_after_add else self.act_fn, allow_fused_gn=False)
        if topdown is not None:
            N, H, W, C = ret.shape
            ret = ret + topdown.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
        if residual is not None:
            ret = ret + residual
        if self.act_fn is not None and has_add and relu_after_add:
            ret = torch.relu_(ret) if is_relu(self.act_fn) else self.act_fn(ret)
        return ret

    def _pick_impl(self, inputs):
        if self.impl != "auto":
            return self.impl
        return "mfma" if self._mfma_eligible(inputs) else "torch"

    def _mfma_operands(self, inputs, w, packed):
        """(inputs, w, packed, pads) as the MFMA conv takes them: refused when
        the shape / device is not eligible; Cin % 4 != 0 runs with zero
        channels appended to the input and the weights (and packs those)."""
        if not self._mfma_eligible(inputs, padded=True):
            raise ValueError(f"{self.scope}: shape/device not supported by the MFMA conv "
                             f"(groups={self.num_groups}, rate={self.rate}, "
                             f"Cin={self.in_channels}, device={inputs.device})")
        pads = same_pads(self.kernel_size, self.rate) if self.padding == "SAME" else (0, 0)
        padc = (-self.in_channels) % 4
        if padc:
            inputs = F.pad(inputs, (0, padc))
            w = F.pad(w, (0, 0, 0, padc))
            packed = None
        if packed is None:
            packed = self.packed_weights(w)
        return inputs, w, packed, pads

    def _conv_torch(self, inputs, w, b):
        """conv (+ bias) on stock PyTorch-ROCm conv2d in channels_last, as an
        NHWC view.  A symmetric SAME pad is the conv's own zero padding (no
        padded copy of the input)."""
        pad = 0
        x = inputs
        if self.padding == "SAME" and self.kernel_size != 1:
            pb, pe = same_pads(self.kernel_size, self.rate)
            if pb == pe:
                pad = pb
            else:
                x = fix_padding(inputs, self.kernel_size, self.padding, self.rate)
        y = F.conv2d(x.permute(0, 3, 1, 2),
                     w.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last), b,
                     stride=self.stride, padding=pad, dilation=self.rate, groups=self.num_groups)
        return y.permute(0, 2, 3, 1)

    def _conv_only(self, inputs):
        """The conv (+ bias) alone, nothing fused and no gradient hand-off
        (empty handoff.Links): what runs under a BatchNorm on batch
        statistics, whose moments need the conv's raw output."""
        w, b = self.weights, self.bias
        if self._pick_impl(inputs) == "torch":
            return self._conv_torch(inputs, w, b)
        inputs, w, packed, pads = self._mfma_operands(inputs, w, None)
        return conv_mfma(inputs, w, b, packed, self.stride, pads, False, links=handoff.Links())

    def _bn_epilogue(self, y, residual, relu_after_add, final_relu):
        """act(bn(y)) with the adds of ``call``: the BatchNorm on batch
        statistics takes the residual add and a ReLU into its apply pass
        (bn + residual inside the conv would feed the sum to the moments);
        any other activation stays the separate pass it is."""
        if final_relu and self.act_fn is not None:
            raise ValueError("final_relu is for layers without an activation")
        norm = self.normalizer_fn
        if self.act_fn is None or is_relu(self.act_fn):
            return norm(y, relu=self.act_fn is not None or final_relu, residual=residual,
                        relu_after_add=relu_after_add or final_relu)
        ret = norm(y)
        if residual is not None and relu_after_add:
            return self.act_fn(ret + residual)
        ret = self.act_fn(ret)
        return ret if residual is None else ret + residual

    def _call_batch_stats(self, inputs, topdown, residual, relu_after_add, final_relu, raw):
        if topdown is not None:
            raise ValueError(f"{self.scope}: the fused top-down add cannot precede a BatchNorm on "
                             "batch statistics (FPN adds it after the lateral's norm)")
        y = self._conv_only(inputs)
        if raw:
            return y
        return self._bn_epilogue(y.contiguous(), residual, relu_after_add, final_relu)


@add_arg_scope
class DeformConv2D(Conv2D):
    """Deformable conv v1 (convolutional.py:267-503), GPU only.

    call = offset conv (``offset_weights`` / ``offset_bias``, zero-initialised,
    over the SAME-padded input, VALID) -> ops.deform_sample (the bilinear
    gather, d2mi_deform_sample_fwd) -> the main product as a 1x1 MFMA conv of
    the column matrix [N,OH,OW,k*k*C] with ``weights.reshape(1,1,k*k*C,Cout)``,
    whose epilogue, dgrad and wgrad are Conv2D's (conv_grad.conv_mfma): the FrozenBN
    fold, the fused ReLU with its tag (handoff.ReluTag), ``residual`` and
    ``final_relu`` work as there.

    The offset conv runs on the MFMA conv too (rate 1): its 2*G*k*k = 18
    output channels are padded to a multiple of 4 by concatenating constant
    zero columns to the weight and bias views (the parameters keep the
    reference shapes); the sampler reads the padded rows through its row
    stride and gives the pad channels a zero gradient.  A dilated offset conv
    (rate > 1) runs on the library conv, as a dilated Conv2D does.

    The folded weights are packed in the 1x1 layout [1,1,Cout,k*k*C] here
    (wants_packed is False: FoldGroup must not emit the 3x3 [k,k,Cout,C]
    packing for this layer)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding="SAME", rate=1,
                 num_groups=1, deform_num_groups=1, use_bias=True, activation=None,
                 normalizer=None, normalizer_params=None, weights_initializer=None,
                 weights_regularizer=None, bias_initializer=None, bias_regularizer=None,
                 variables_collections=None, trainable=True, outputs_collections=None, **kwargs):
        if in_channels % deform_num_groups != 0:
            raise ValueError(f'"in_channels" {in_channels} is not divisible by '
                             f'"deform_num_groups" {deform_num_groups}.')
        if num_groups != 1:
            raise NotImplementedError(
                "grouped deformable convs (num_groups > 1) are not implemented: no shipped "
                "config uses them")
        if kernel_size not in (1, 3):
            raise NotImplementedError("DeformConv2D: kernel_size 1 and 3 are implemented")
        kwargs.pop("impl", None)  # (an arg-scope default for Conv2D: always the HIP path here)
        Conv2D.__init__(self, in_channels, out_channels, kernel_size, stride=stride,
                        padding=padding, rate=rate, num_groups=1, use_bias=use_bias,
                        activation=activation, normalizer=normalizer,
                        normalizer_params=normalizer_params,
                        weights_initializer=weights_initializer,
                        weights_regularizer=weights_regularizer,
                        bias_initializer=None,  # the reference forces zeros (:311)
                        bias_regularizer=bias_regularizer, trainable=trainable, impl="mfma",
                        deform_num_groups=deform_num_groups, **kwargs)

    def build(self):
        super().build()
        k = self.kernel_size
        oc = self.offset_channels = 2 * self.deform_num_groups * k * k
        self.offset_weights = torch.nn.Parameter(torch.zeros(k, k, self.in_channels, oc),
                                                 requires_grad=self.trainable)
        self.offset_bias = torch.nn.Parameter(torch.zeros(oc), requires_grad=self.trainable)
        padc = (-oc) % 4
        # constant zero columns for the MFMA offset conv (not variables)
        self.register_buffer("_offset_pad_w", torch.zeros(k, k, self.in_channels, padc),
                             persistent=False)
        self.register_buffer("_offset_pad_b", torch.zeros(padc), persistent=False)
        self._offset_pack = Versioned()
        self._cols_pack = Versioned()

    def wants_packed(self):
        return False

    def _offsets(self, x, pads):
        """[N,OH,OW,>= offset_channels]: the offset conv (:380-406)."""
        if self.rate != 1 or self.in_channels % 4 != 0:
            xp = F.pad(x, (0, 0, pads[0], pads[1], pads[0], pads[1])) if any(pads) else x
            y = F.conv2d(xp.permute(0, 3, 1, 2), self.offset_weights.permute(3, 2, 0, 1),
                         self.offset_bias, stride=self.stride, dilation=self.rate)
            return y.permute(0, 2, 3, 1).contiguous()
        return conv_padded_out(x, self.offset_weights, self.offset_bias, self._offset_pad_w,
                               self._offset_pad_b, self._offset_pack, self.stride, pads)

    def call(self, inputs, residual=None, final_relu=False, res_grad_to=None, raw=False):
        """residual / final_relu / res_grad_to / raw: as Conv2D.call.  The input
        has two readers here (the offset conv and the sampler), so there is no
        relu_input_sole_consumer: the producer keeps its own ReLU backward."""
        if not inputs.is_cuda:
            raise ValueError(f"{self.scope}: DeformConv2D runs on the GPU (HIP) only, got a "
                             f"tensor on {inputs.device}")
        if final_relu and self.act_fn is not None:
            raise ValueError("final_relu is for layers without an activation")
        k = self.kernel_size
        w, b, norm, _ = self.effective_params()
        pads = same_pads(k, self.rate) if (self.padding == "SAME" and k != 1) else (0, 0)
        offsets = self._offsets(inputs, pads)
        cols = ops.deform_sample(inputs, offsets, k, self.stride, self.rate, pads,
                                 self.deform_num_groups)
        w1 = w.reshape(1, 1, k * k * self.in_channels, self.out_channels)

        def pack():
            return ops.pack_conv_weights(w1.detach())

        if torch.is_grad_enabled() and self.fold_trainable():
            packed = pack()
        else:  # constant weights: packed once per parameter version
            packed = self._cols_pack.get(self._param_key(), pack)
        if self._bn_batch_stats:
            if res_grad_to is not None:
                raise ValueError(f"{self.scope}: res_grad_to cannot be honoured under a BatchNorm "
                                 "on batch statistics (no gradient hand-offs there)")
            y = conv_mfma(cols, w1, b, packed, 1, (0, 0), False, links=handoff.Links())
            return y if raw else self._bn_epilogue(y, residual, False, final_relu)
        fuse_relu = norm is None and (is_relu(self.act_fn) or final_relu)
        links = handoff.Links(res_grad_to=res_grad_to) if res_grad_to is not None else None
        ret = conv_mfma(cols, w1, b, packed, 1, (0, 0), fuse_relu, residual=residual,
                        relu_after=bool(final_relu), links=links)
        if raw:
            return ret
        # (no fused GroupNorm + ReLU: the dconv + GN configs run the two passes)
        return epilogue(ret, norm, self.act_fn, fused_relu=fuse_relu, final_relu=final_relu,
                        allow_fused_gn=False)


@add_arg_scope
class ModulatedDeformConv2D(Layer):
    """The reference's ModulatedDeformConv2D (convolutional.py:506-745) can be
    neither constructed nor called, so there is no behaviour to match."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(
            "ModulatedDeformConv2D: the reference class cannot be constructed or called, so "
            "there is no behaviour to match -- convolutional.py:536 calls "
            "super(DeformConv2D, self).__init__ (a TypeError), :653-659 reshape 3*G*k*k offset "
            "channels to [..., 2] and then read offset[..., 2], :677 uses an undefined `batch`, "
            "and :727 calls a missing self.group_conv2d")


@add_arg_scope
class ConvTranspose2D(Layer):
    """Transposed conv (convolutional.py:747-893); weights [k, k, out, in].

    For the kernel == stride case of the mask head (2x2, s2) each input pixel
    owns a disjoint 2x2 output block, so the op is one GEMM over
    [pixels, in] x [in, k*k*out]: it runs on the MFMA conv kernel as a 1x1
    conv whose packed weight is the TF kernel itself, followed by a pixel
    shuffle."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding="SAME",
                 use_bias=True, activation=None, normalizer=None, normalizer_params=None,
                 weights_initializer=None, weights_regularizer=None, bias_initializer=None,
                 bias_regularizer=None, variables_collections=None, trainable=True,
                 outputs_collections=None, **kwargs):
        super().__init__(in_channels=in_channels, out_channels=out_channels,
                         kernel_size=kernel_size, stride=stride, padding=padding.upper(),
                         use_bias=use_bias, activation=activation, normalizer=normalizer,
                         normalizer_params=normalizer_params, weights_initializer=weights_initializer,
                         bias_initializer=bias_initializer, trainable=trainable, **kwargs)
        k = kernel_size
        w = torch.empty((k, k, out_channels, in_channels))
        # fans of a transposed kernel: tf computes them on [k, k, out, in]
        (weights_initializer or init.variance_scaling(2.0, distribution="untruncated_normal"))(w)
        self.weights = torch.nn.Parameter(w, requires_grad=trainable)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels), requires_grad=trainable) if use_bias else None
        self.normalizer_fn = _normalizer(normalizer, normalizer_params, out_channels)
        self.act_fn = get_activation(activation)

    def call(self, inputs, relu_input_sole_consumer=False):
        k, s = self.kernel_size, self.stride
        N, H, W, C = inputs.shape
        if k == s:  # the mask-head case: MFMA GEMM (raises off-GPU, no CPU fallback)
            wp = self.weights.reshape(1, 1, k * k * self.out_channels, self.in_channels)
            b = self.bias.repeat(k * k) if self.bias is not None else None
            fuse = self.normalizer_fn is None and is_relu(self.act_fn)
            links = handoff.Links(sole_consumer=True) if relu_input_sole_consumer else None
            y = conv_mfma(inputs, wp.permute(0, 1, 3, 2), b, wp.detach().contiguous(), 1, (0, 0),
                          fuse, links=links)
            y = y.reshape(N, H, W, k, k, self.out_channels).permute(0, 1, 3, 2, 4, 5)
            ret = y.reshape(N, H * k, W * k, self.out_channels)
            # (no fused GroupNorm + ReLU after the pixel shuffle, as ever)
            return epilogue(ret, self.normalizer_fn, self.act_fn, fused_relu=fuse,
                            allow_fused_gn=False)
        # general case on torch: conv_transpose2d with TF 'SAME'/'VALID' output size
        w = self.weights.permute(3, 2, 0, 1)  # [in, out, kh, kw]
        y = F.conv_transpose2d(inputs.permute(0, 3, 1, 2), w, self.bias, stride=s)
        OH = H * s + (max(k - s, 0) if self.padding == "VALID" else 0)
        OW = W * s + (max(k - s, 0) if self.padding == "VALID" else 0)
        if self.padding == "SAME":
            ph, pw = max((H - 1) * s + k - OH, 0), max((W - 1) * s + k - OW, 0)
            y = y[:, :, ph // 2: ph // 2 + OH, pw // 2: pw // 2 + OW]
        return epilogue(y.permute(0, 2, 3, 1), self.normalizer_fn, self.act_fn,
                        allow_fused_gn=False)
