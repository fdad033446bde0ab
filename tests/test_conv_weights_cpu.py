"""The version-keyed weight cache, the fold / pack groups' bookkeeping
(layers/conv_weights.py) and the conv epilogue (layers/convolutional.py), on
the CPU: counting stand-ins replace the kernels."""
import itertools

import pytest
import torch

from detectron2_tensorflow_amd.layers import BatchNorm, Conv2D, get_activation, ops
from detectron2_tensorflow_amd.layers.conv_weights import (FoldGroup, PackGroup, Versioned,
                                                           version_key)
from detectron2_tensorflow_amd.layers.convolutional import epilogue


class Maker:
    """make() -> a fresh value that names the call it came from."""

    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return ("made", self.n)


def param(shape=(1, 1, 4, 4)):
    return torch.nn.Parameter(torch.zeros(shape))


# ------------------------------------------------------------------ Versioned
def test_cache_makes_once_and_remakes_when_the_parameter_moves():
    p, cache, make = param(), Versioned(), Maker()

    def get(extra=()):
        return cache.get(version_key((p,), extra), make)

    assert get() == ("made", 1) and get() == ("made", 1) and make.n == 1
    with torch.no_grad():  # the optimizer's in-place update: a new _version
        p.add_(1.0)
    assert get() == ("made", 2) and get() == ("made", 2) and make.n == 2
    p.data = p.data.clone()  # new storage (.to(), a loaded checkpoint): a new data_ptr
    assert get() == ("made", 3) and make.n == 3
    assert get((1, 1, 4, 4)) == ("made", 4)  # extra, e.g. the packed tensor's shape
    assert get((1, 1, 8, 4)) == ("made", 5)
    # back at an earlier key: remade, never the value another key made
    assert get((1, 1, 4, 4)) == ("made", 6) and get() == ("made", 7) and make.n == 7


def test_cache_takes_a_precomputed_key_and_keeps_nothing_of_a_failed_make():
    cache, make = Versioned(), Maker()
    assert cache.get((7, 0), make) == ("made", 1) and cache.get((7, 0), make) == ("made", 1)

    def fails():
        raise RuntimeError("no pack")

    with pytest.raises(RuntimeError):
        cache.get((7, 1), fails)
    assert cache.get((7, 0), make) == ("made", 1)  # (the old value is still its key's)
    assert cache.get((7, 1), make) == ("made", 2)


@pytest.mark.parametrize("moved", range(4))
def test_multi_tensor_key_remakes_when_any_one_tensor_moves(moved):
    ts = [param(), param(), param((4,)), param((4,))]  # as the RPN head's fused 1x1
    cache, make = Versioned(), Maker()
    assert cache.get(version_key(ts), make) == cache.get(version_key(ts), make) == ("made", 1)
    with torch.no_grad():
        ts[moved].mul_(2.0)
    assert cache.get(version_key(ts), make) == ("made", 2) and make.n == 2


# ------------------------------------------------------------------- epilogue
class Norm:
    """y -> 2y + 1 (then ReLU when asked to fuse it); records each call's relu.
    fusable None: a normaliser without fused_ok; else what fused_ok answers."""

    def __init__(self, fusable):
        self.calls = []
        if fusable is not None:
            self.fused_ok = lambda y: fusable

    def __call__(self, y, relu=False):
        self.calls.append(relu)
        out = 2 * y + 1
        return out.clamp_min(0) if relu else out


Y = torch.randn((1, 2, 3, 4), generator=torch.Generator().manual_seed(3))
NORMS = {"none": None, "plain": None, "fusable": True, "refuses": False}


@pytest.mark.parametrize("kind,act,fused_relu,final_relu,allow", itertools.product(
    NORMS, (None, "relu", "sigmoid"), (False, True), (False, True), (False, True)))
def test_epilogue_is_the_written_out_composition(kind, act, fused_relu, final_relu, allow):
    norm = None if kind == "none" else Norm(NORMS[kind])
    act_fn = get_activation(act)

    def run():
        return epilogue(Y.clone(), norm, act_fn, fused_relu=fused_relu, final_relu=final_relu,
                        allow_fused_gn=allow)

    if final_relu and act_fn is not None:
        with pytest.raises(ValueError, match="final_relu is for layers without an activation"):
            run()
        return
    got = run()
    fused_gn = allow and act == "relu" and kind == "fusable"
    want = Y.clone()
    if norm is not None:
        want = 2 * want + 1
    if fused_gn:
        want = want.clamp_min(0)
    else:
        if act_fn is not None and not fused_relu:
            want = act_fn(want)
        if final_relu and not fused_relu:
            want = want.clamp_min(0)
    assert torch.equal(got, want)
    assert (norm.calls if norm is not None else None) == (None if norm is None else [fused_gn])


# ------------------------------------------------------- FoldGroup / PackGroup
class _OnGpu(torch.nn.Parameter):
    """A CPU parameter that says it is on the GPU: the groups batch GPU members
    only, and the stand-in ops below never touch the data."""
    is_cuda = True


def bump(p):
    with torch.no_grad():
        p.add_(1.0)


def test_fold_group_folds_every_member_in_one_call_and_refolds_a_taken_slot(monkeypatch):
    convs = [Conv2D(4, 4, 1, normalizer=BatchNorm, use_bias=False, scope=f"c{i}")
             for i in range(3)]
    for c in convs:
        c.weights = _OnGpu(c.weights.data)
    calls = []

    def fold_many(entries):
        calls.append([e[0] for e in entries])
        return [((len(calls), i, "w"), (len(calls), i, "b"), None) for i in range(len(entries))]

    monkeypatch.setattr(ops, "fold_frozen_bn_many", fold_many)
    grp = FoldGroup(convs)
    assert all(c._fold_group is grp for c in convs)
    got = [grp.fetch(c) for c in convs]
    assert len(calls) == 1 and all(a is c.weights for a, c in zip(calls[0], convs))
    assert got == [((1, i, "w"), (1, i, "b"), None) for i in range(3)]
    # a second fetch of a taken slot (a second forward) refolds the group
    assert grp.fetch(convs[1]) == ((2, 1, "w"), (2, 1, "b"), None) and len(calls) == 2
    assert grp.fetch(convs[0]) == ((2, 0, "w"), (2, 0, "b"), None) and len(calls) == 2
    # a member whose parameters moved since the fold: refolded before it is handed out
    bump(convs[2].normalizer_fn.gamma)
    assert grp.fetch(convs[2]) == ((3, 2, "w"), (3, 2, "b"), None) and len(calls) == 3
    assert len(calls[2]) == 3


def test_pack_group_repacks_only_the_members_whose_version_moved(monkeypatch):
    convs = [Conv2D(4, 4, 1, scope=f"c{i}") for i in range(3)]
    calls = []

    def pack_many(ws):
        calls.append(list(ws))
        return [("packed", len(calls), w.data_ptr(), w._version) for w in ws]

    monkeypatch.setattr(ops, "pack_conv_weights_many", pack_many)
    grp = PackGroup()
    for c in convs:
        c._pack_group = grp
    first = [c.packed_weights() for c in convs]  # each joins on its first call
    assert [len(ws) for ws in calls] == [1, 1, 1] and len(grp.members) == 3
    assert [c.packed_weights() for c in convs] == first and len(calls) == 3
    bump(convs[0].weights)
    bump(convs[2].weights)
    got2 = convs[2].packed_weights()  # one call covers every stale member
    assert len(calls) == 4 and [w.data_ptr() for w in calls[3]] == [
        convs[0].weights.data_ptr(), convs[2].weights.data_ptr()]
    assert got2 == ("packed", 4, convs[2].weights.data_ptr(), convs[2].weights._version)
    assert convs[0].packed_weights()[1] == 4 and convs[1].packed_weights() is first[1]
    assert len(calls) == 4
