"""GroupNorm training, the parts that need no GPU: the torch arm of
ops.group_norm_train against the float64 restatement (tests/gn_reference.py),
which tensors the HIP arm takes (gn_train_fused), the new C entries' host-side
refusals, and the conv epilogue's choice to fuse the ReLU."""
import ctypes
import os
import re

import pytest
import torch

import gn_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d2mi_group_norm_train_fwd", "d2mi_group_norm_train_fwd_workspace_size",
           "d2mi_group_norm_train_bwd", "d2mi_group_norm_train_bwd_workspace_size")


def inputs(shape, seed=3, offset=30.0, spread=0.3):
    """x = 30 + 0.3 randn (a formula that cancels against the mean misses the
    bar by an order of magnitude), gamma ~ U(0.5, 1.5), beta and dy ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    return {"x": offset + spread * torch.randn(shape, generator=g),
            "gamma": 0.5 + torch.rand(C, generator=g), "beta": torch.randn(C, generator=g),
            "dy": torch.randn(shape, generator=g)}


def run_op(t, G, dev, relu, grads=(True, True, True)):
    """One forward + backward of ops.group_norm_train on ``dev``: dict of y, dx,
    dgamma, dbeta (None where ``grads`` (x, gamma, beta) asks for none)."""
    from detectron2_tensorflow_amd.layers import ops
    x, gamma, beta = (t[k].detach().clone().to(dev).requires_grad_(w)
                      for k, w in zip(("x", "gamma", "beta"), grads))
    y = ops.group_norm_train(x, G, gamma, beta, 1e-5, relu)
    y.backward(t["dy"].to(dev))
    return {"y": y.detach(), "dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


def check_against_float64(got, t, G, relu):
    """y, then dx / dgamma / dbeta, within the bar of float64.  The backward's
    ReLU mask is the checked forward's own y > 0, taken once y has met the bar;
    no element is left out of any comparison."""
    fwd = ref.forward(t["x"], G, t["gamma"], t["beta"], 1e-5, relu)
    ref.close(got["y"], fwd["y"], "y")
    mask = (got["y"].cpu() > 0) if relu else None
    bwd = ref.backward(fwd, t["dy"], t["gamma"], mask)
    for k in ("dx", "dgamma", "dbeta"):
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        ref.close(got[k], bwd[k], k)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,G", [((2, 5, 7, 8), 2), ((1, 1, 1, 8), 2), ((3, 4, 5, 6), 3)])
def test_torch_arm_on_cpu_vs_float64(shape, G, relu):
    """The torch arm's arithmetic is torch's: its CPU kernel takes the variance
    as E[x^2] - E[x]^2, a relative error of about 6e-8 * mean^2 / var (6e-4 at
    x = 30 + 0.3 randn, six times the bar; 1e-7 at the 0.5 + randn used here).
    The large-mean inputs test the project's own kernels (test_gpu_groupnorm)."""
    t = inputs(shape, offset=0.5, spread=1.0)
    check_against_float64(run_op(t, G, "cpu", relu), t, G, relu)


def test_gn_train_fused_refuses_cpu_sizes_and_toggle_off():
    from detectron2_tensorflow_amd.layers import ops
    from detectron2_tensorflow_amd.layers.ops import norm

    class OnGpu:
        """The attributes the predicate reads, of a float32 GPU tensor."""
        is_cuda, dtype = True, torch.float32

        def __init__(self, shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

    assert norm.gn_train_fused is ops.gn_train_fused
    assert not ops.gn_train_fused(torch.zeros(2, 3, 3, 64), 64, 16)       # a CPU tensor
    x = OnGpu((2, 3, 3, 64))
    old = norm.FUSED_GN_TRAIN
    try:
        norm.FUSED_GN_TRAIN = True
        assert ops.gn_train_fused(x, 64, 16)
        assert not ops.gn_train_fused(x, 64, 32)                          # C / G = 2
        assert not ops.gn_train_fused(OnGpu((2, 3, 3, 4096)), 4096, 32)   # C = 4096
        assert ops.gn_train_fused(OnGpu((2, 3, 3, 2048)), 2048, 32)
        assert not ops.gn_train_fused(OnGpu((2, 3, 3, 520)), 520, 65)     # G = 65
        norm.FUSED_GN_TRAIN = False
        assert not ops.gn_train_fused(x, 64, 16)
    finally:
        norm.FUSED_GN_TRAIN = old


def test_layer_on_cpu_takes_the_torch_arm():
    from detectron2_tensorflow_amd.layers import GroupNorm
    t = inputs((2, 5, 7, 8), offset=0.5, spread=1.0)  # (as test_torch_arm_on_cpu_vs_float64)
    gn = GroupNorm(8, num_groups=2)
    with torch.no_grad():
        gn.gamma.copy_(t["gamma"]); gn.beta.copy_(t["beta"])
    x = t["x"].clone().requires_grad_(True)
    assert not gn.fused_ok(x) and not gn.train_fused_ok(x)
    y = gn(x, relu=True)
    y.backward(t["dy"])
    got = {"y": y.detach(), "dx": x.grad, "dgamma": gn.gamma.grad, "dbeta": gn.beta.grad}
    check_against_float64(got, t, 2, True)


def test_new_entries_are_declared_in_the_header():
    src = open(os.path.join(ROOT, "include", "d2mi.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, bare), name
    assert src.count("lib/layers/normalization.py:174-260") >= 2  # each entry cites its lines


def test_new_entries_refuse_bad_sizes_and_short_workspaces_without_gpu():
    """Argument validation happens on the host before any launch: null
    pointers, no GPU."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    ws = ctypes.c_void_p(256)  # non-null, never dereferenced: the carve is refused first

    def fwd(N, H, W, C, G, n):
        return lib.d2mi_group_norm_train_fwd(None, N, H, W, C, G, None, None, 1e-5, 1, None, None,
                                             None, ws, n, None)

    def bwd(N, H, W, C, G, n):
        return lib.d2mi_group_norm_train_bwd(None, None, N, H, W, C, G, None, None, None, None,
                                             1e-5, 1, None, None, None, ws, n, None)

    for call, query in ((fwd, lib.d2mi_group_norm_train_fwd_workspace_size),
                        (bwd, lib.d2mi_group_norm_train_bwd_workspace_size)):
        for bad in ((2, 8, 8, 32, 16), (2, 8, 8, 4096, 32), (2, 8, 8, 520, 65), (2, 0, 8, 32, 4),
                    (2, 8, 8, 30, 4), (-1, 8, 8, 32, 4)):
            assert query(*bad) == 0, bad
            rc = call(*bad, 1 << 20)
            assert rc < 0 and "bad sizes" in _C.last_error(), (bad, rc, _C.last_error())
        for shape in ((2, 8, 8, 32, 4), (2, 3, 5, 2048, 32), (70, 7, 7, 256, 32)):
            size = query(*shape)
            assert size > 1, shape
            rc = call(*shape, size - 1)
            msg = _C.last_error()
            assert rc < 0 and "too small" in msg and f"{size - 1} < {size}" in msg, (shape, msg)
            rc = call(*shape, size)  # enough workspace: the null operands are refused next
            assert rc < 0 and "null operand" in _C.last_error(), (shape, _C.last_error())
        assert call(0, 8, 8, 32, 4, 0) == 0  # N == 0: nothing to do


class Norm:
    """y -> 2y + 1 (then ReLU when asked to fuse it); records each call's relu."""

    def __init__(self, fused, train_fused):
        self.calls = []
        self.fused_ok = lambda y: fused
        if train_fused is not None:
            self.train_fused_ok = lambda y: train_fused

    def __call__(self, y, relu=False):
        self.calls.append(relu)
        out = 2 * y + 1
        return out.clamp_min(0) if relu else out


@pytest.mark.parametrize("fused,train_fused,allow,act,want", [
    (False, True, True, "relu", [True]), (False, False, True, "relu", [False]),
    (False, None, True, "relu", [False]), (False, True, False, "relu", [False]),
    (False, True, True, "sigmoid", [False]), (True, False, True, "relu", [True])])
def test_epilogue_fuses_the_relu_into_a_training_normaliser(fused, train_fused, allow, act, want):
    from detectron2_tensorflow_amd.layers.activation import get_activation
    from detectron2_tensorflow_amd.layers.convolutional import epilogue
    y = torch.randn((1, 2, 3, 4), generator=torch.Generator().manual_seed(3))
    norm = Norm(fused, train_fused)
    act_fn = get_activation(act)
    got = epilogue(y.clone(), norm, act_fn, allow_fused_gn=allow)
    assert norm.calls == want  # called once
    assert torch.equal(got, act_fn(2 * y + 1))
