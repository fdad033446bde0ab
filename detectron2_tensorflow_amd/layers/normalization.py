"""BatchNorm / GroupNorm / get_norm (lib/layers/normalization.py:15-274).

BatchNorm has two forms, chosen when the layer is built and never read from
torch's ``.training`` flag (``model.train()`` must not thaw a frozen layer):

* the inference form (FrozenBN, ``training=False``, and every layer built
  with no ``training`` keyword): the moving statistics,
      y = x * gamma * rsqrt(var + eps) + (beta - mean * gamma * rsqrt(var + eps)),
  which Conv2D folds into its weights (the hot-path configs: FrozenBN in the
  backbone, no norm in FPN / heads);
* the batch-statistics form (``training=True``; normalization.py:97-119):
  the biased moments of the batch, the moving averages updated in place with
  ``decay``, on the kernels of csrc/batch_norm.hip (ops.batch_norm_train).
  With ``sync=True`` and more than one rank the moments are those of all
  replicas' rows (what the reference's SyncBN branch, :120-165, means; it
  cannot run there).
"""
from contextlib import contextmanager

import torch

from ..utils import training as _training
from ..utils.arg_scope import add_arg_scope, arg_scope
from . import ops
from .base import Layer


@add_arg_scope
class BatchNorm(Layer):
    def __init__(self, channels, momentum=0.997, epsilon=1e-5, center=True, scale=True,
                 trainable=True, sync=False, decay=0.9, **kwargs):
        # the form is the keyword's alone: a layer built without it stays in
        # the inference form whatever the global phase says
        batch_stats = bool(kwargs.pop("training", False))
        if batch_stats and not trainable:
            raise ValueError("[BatchNorm] Frozen BatchNorm should not update EMA!")
        super().__init__(channels=channels, momentum=momentum, epsilon=epsilon, center=center,
                         scale_=scale, trainable=trainable, sync=sync, decay=decay,
                         training=batch_stats, **kwargs)
        object.__setattr__(self, "_batch_stats", batch_stats)
        self.beta = torch.nn.Parameter(torch.zeros(channels), requires_grad=trainable) if center else None
        self.gamma = torch.nn.Parameter(torch.ones(channels), requires_grad=trainable) if scale else None
        self.register_buffer("moving_mean", torch.zeros(channels))
        self.register_buffer("moving_variance", torch.ones(channels))

    @property
    def batch_stats(self):
        """True: normalises with the batch's own statistics and updates the
        moving averages; False: the inference form (foldable)."""
        return self._batch_stats

    def folded(self):
        """(scale, shift) of the frozen affine transform."""
        inv = torch.rsqrt(self.moving_variance + self.epsilon)
        scale = inv * self.gamma if self.gamma is not None else inv
        shift = -self.moving_mean * scale
        if self.beta is not None:
            shift = shift + self.beta
        return scale, shift

    def call(self, x, relu=False, residual=None, relu_after_add=False):
        """relu / residual / relu_after_add: the ReLU and the add that follow
        the layer in a conv (relu(bn(x)), relu(bn(x)) + residual,
        relu(bn(x) + residual)), fused into the batch-statistics apply pass."""
        if self._batch_stats:
            mode = ops.norm.RELU_NONE
            if relu:
                mode = (ops.norm.RELU_AFTER_ADD if relu_after_add and residual is not None
                        else ops.norm.RELU_BEFORE_ADD)
            return ops.batch_norm_train(x, self.gamma, self.beta, self.moving_mean,
                                        self.moving_variance, self.epsilon, self.decay,
                                        residual, mode, self.sync)
        scale, shift = self.folded()
        y = x * scale + shift
        if relu and not (relu_after_add and residual is not None):
            y = torch.relu(y)
        if residual is not None:
            y = y + residual
            if relu and relu_after_add:
                y = torch.relu(y)
        return y


@add_arg_scope
class GroupNorm(Layer):
    def __init__(self, channels, num_groups=32, epsilon=1e-5, trainable=True, **kwargs):
        super().__init__(channels=channels, num_groups=num_groups, epsilon=epsilon, **kwargs)
        self.gamma = torch.nn.Parameter(torch.ones(channels), requires_grad=trainable)
        self.beta = torch.nn.Parameter(torch.zeros(channels), requires_grad=trainable)

    def fused_ok(self, x):
        """The HIP GroupNorm (d2mi_group_norm_nhwc, no autograd) takes the call
        only when no gradient is needed at all: neither the input nor the
        affine parameters require one (a frozen GN in a trainable branch must
        still pass the input gradient through torch's group_norm)."""
        C = self.channels
        return (x.is_cuda and not self._needs_grad(x)
                and C % self.num_groups == 0 and (C // self.num_groups) % 4 == 0 and C <= 1024
                and self.num_groups <= 64)

    def _needs_grad(self, x):
        return torch.is_grad_enabled() and (
            x.requires_grad or self.gamma.requires_grad or self.beta.requires_grad)

    def train_fused_ok(self, x):
        """A call that needs a gradient runs the HIP training kernels
        (ops.group_norm_train's fused arm), ReLU included."""
        return self._needs_grad(x) and ops.gn_train_fused(x, self.channels, self.num_groups)

    def call(self, x, relu=False, up2=False, accumulate_into=None):
        """GroupNorm.call (normalization.py:235-260) on NHWC.  relu / up2 /
        accumulate_into fuse the ops that follow it in the SOLOv2 heads (HIP
        inference path); a call that needs a gradient runs
        ops.group_norm_train (GroupNorm + ReLU), then up2 / the sum."""
        if self.fused_ok(x):
            return ops.group_norm(x, self.num_groups, self.gamma, self.beta, self.epsilon,
                                  relu, up2, accumulate_into)
        # (without a gradient and outside fused_ok -- the CPU, C > 1024 -- torch, as ever)
        norm = ops.group_norm_train if self._needs_grad(x) else ops.norm.group_norm_torch
        y = norm(x, self.num_groups, self.gamma, self.beta, self.epsilon, relu)
        if up2:
            y = y.repeat_interleave(2, 1).repeat_interleave(2, 2)
        if accumulate_into is not None:
            return accumulate_into.add_(y)
        return y


def norm_phase():
    """The global training phase, False when unset (as Layer.__init__)."""
    try:
        return _training.get_training_phase()
    except ValueError:
        return False


@contextmanager
def batch_norm_arg_scope(norm, freeze=False, sync=False):
    """The ``training`` / ``sync`` keywords of the BatchNorm layers a builder
    makes for the config string ``norm``, passed explicitly (a BatchNorm
    built without the keyword stays in the inference form):
    "FrozenBN", or ``freeze``: training=False; "BN" / "SyncBN": training =
    the phase, and sync=True for "SyncBN" where the builder asks for it
    (``sync``: the reference sets it in the backbone scopes only,
    lib/modeling/backbone/resnet.py:35-39).  Any other norm: nothing."""
    if norm not in ("BN", "SyncBN", "FrozenBN"):
        yield
        return
    if norm == "FrozenBN" or freeze:
        kw = {"training": False}
    else:
        kw = {"training": norm_phase()}
        if norm == "SyncBN" and sync:
            kw["sync"] = True
    with arg_scope([BatchNorm], **kw):
        yield


def get_norm(norm):
    if isinstance(norm, str):
        if len(norm) == 0:
            return None
        if norm == "GN":
            return GroupNorm
        if norm in ("BN", "FrozenBN", "SyncBN"):
            return BatchNorm
        raise ValueError(f"{norm} is not recognized !")
    return norm
