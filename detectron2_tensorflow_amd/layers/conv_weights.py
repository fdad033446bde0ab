"""Values derived from conv parameters (packed copies, FrozenBN folds), remade
when the parameters change.  A stale copy is silent (the forward runs on last
step's weights), so every site keeps its copy in a ``Versioned``; ``FoldGroup``
and ``PackGroup`` refresh those of many layers in one launch.
"""
import collections

from . import ops
from .normalization import BatchNorm


class Versioned:
    """A derived value, valid while a key is unchanged: ``version_key`` of the
    parameters it is made from (an optimizer step bumps _version, .to() or a
    loaded checkpoint moves data_ptr), or the caller's own (Conv2D._param_key)."""
    key = value = None  # (no key is None: nothing is valid yet)

    def get(self, key, make):
        if self.key != key:
            self.value, self.key = make(), key
        return self.value


def version_key(tensors, extra=()):
    return tuple((t.data_ptr(), t._version) for t in tensors) + tuple(extra)


def _foldable_bn(norm):
    """A BatchNorm in the inference form: folded into the conv weights.  One on
    batch statistics (BatchNorm.batch_stats) runs after the raw conv instead."""
    return isinstance(norm, BatchNorm) and not norm.batch_stats


def _convs(module, folded):
    from .convolutional import Conv2D
    return [m for m in module.modules()
            if isinstance(m, Conv2D) and _foldable_bn(m.normalizer_fn) == folded]


# one FoldGroup member's fold: made at ``key``, handed out once (``taken``)
_Folded = collections.namedtuple("_Folded", "w b packed taken key")


class FoldGroup:
    """The trainable Conv2D + FrozenBN layers of one network folded together:
    the first of them to run in a training forward folds all of them with
    ops.fold_frozen_bn_many (one launch, and one backward pair once every
    gradient has arrived, instead of three launches per layer); each layer
    then takes its own result once.  A layer whose parameters changed since
    (new version) or whose result was already taken (a second forward) makes
    the next fetch refold the group."""
    ENABLED = True

    def __init__(self, layers):
        self.layers = list(layers)
        self.slots = {}
        for layer in self.layers:
            layer._fold_group = self

    @classmethod
    def attach(cls, module):
        layers = _convs(module, folded=True)
        return cls(layers) if layers else None

    def fetch(self, layer):
        s = self.slots.get(id(layer))
        if s is None or s.taken or s.key != layer._param_key():
            self._fold()
            s = self.slots.get(id(layer))
            if s is None:
                return None
        self.slots[id(layer)] = _Folded(None, None, None, True, s.key)
        return s.w, s.b, s.packed

    def _fold(self):
        members = [m for m in self.layers if m.weights.is_cuda and m.fold_trainable()
                   and _foldable_bn(m.normalizer_fn)]
        norms = [m.normalizer_fn for m in members]
        outs = ops.fold_frozen_bn_many([
            (m.weights, m.bias, n.gamma, n.beta, n.moving_mean, n.moving_variance, n.epsilon,
             m.wants_packed()) for m, n in zip(members, norms)])
        self.slots = {id(m): _Folded(w, b, p, False, m._param_key())
                      for m, (w, b, p) in zip(members, outs)}


class PackGroup:
    """The un-normalised MFMA convs of one model (FPN, RPN head, ROI heads):
    their packed weight copies are refreshed together.  A layer joins on its
    first packed_weights() call; the first fetch that finds its layer's
    parameters changed (the optimizer stepped) repacks EVERY member whose
    parameters changed in one launch (ops.pack_conv_weights_many) instead of
    one launch per layer."""
    ENABLED = True

    def __init__(self):
        self.members = []

    @classmethod
    def attach(cls, module):
        layers = _convs(module, folded=False)
        g = cls() if layers else None
        for m in layers:
            m._pack_group = g
        return g

    def fetch(self, layer):
        if not any(m is layer for m in self.members):
            self.members.append(layer)
        key = layer._pack_key(layer.weights)
        if layer._pack.key == key:
            return layer._pack.value
        stale = [(m, key if m is layer else m._pack_key(m.weights)) for m in self.members]
        stale = [(m, k) for m, k in stale if m._pack.key != k]
        outs = ops.pack_conv_weights_many([m.weights.detach() for m, _ in stale])
        for (m, k), o in zip(stale, outs):
            m._pack.value, m._pack.key = o, k
        return layer._pack.value
