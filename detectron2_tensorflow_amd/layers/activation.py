"""get_activation (lib/layers/activation.py:10-20).

"mish" and "leaky_relu" (YOLOv4's backbone and neck / head) run as one
in-place HIP pass (d2mi_activation) over a GPU tensor that needs no gradient:
the layers apply their activation to the fresh output of their own conv, so
nothing else reads the overwritten values.  With a gradient, on the CPU, or
with FUSED off they are the torch compositions.
"""
import torch
import torch.nn.functional as F

# the HIP pass on the GPU (False: the torch compositions; tests compare)
FUSED = True


def _fused_ok(x):
    return (FUSED and x.is_cuda and x.dtype is torch.float32
            and not (torch.is_grad_enabled() and x.requires_grad))


def _fused(x, code, alpha=0.0):
    from . import ops  # (activation_ is ops/detect.py's; the package imports nothing from here)
    return ops.activation_(x if x.is_contiguous() else x.contiguous(), code, alpha)


def _mish_torch(x):
    return x * torch.tanh(F.softplus(x))


def _mish(x):
    if _fused_ok(x):
        return _fused(x, 2)
    return _mish_torch(x)


def _leaky_relu(x):
    if _fused_ok(x):
        return _fused(x, 1, 0.1)
    return F.leaky_relu(x, 0.1)


_ACTS = {
    "relu": torch.relu, "relu6": F.relu6, "sigmoid": torch.sigmoid, "tanh": torch.tanh,
    "leaky_relu": _leaky_relu, "swish": F.silu, "mish": _mish,
}


def get_activation(activation):
    if activation is None or activation == "":
        return None
    if callable(activation):
        return activation
    if activation not in _ACTS:
        raise ValueError(f"{activation} is not recognized!")
    return _ACTS[activation]


def is_relu(fn):
    return fn is torch.relu or fn is F.relu or fn is torch.nn.functional.relu
