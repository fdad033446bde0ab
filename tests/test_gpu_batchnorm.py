"""BatchNorm on batch statistics on the GPU (csrc/batch_norm.hip): the HIP arm
against the float64 restatement (tests/bn_reference.py) and against the tensor
arm, through Conv2D and a bottleneck block, SyncBN over two processes, the
untouched frozen path, and one Trainer step of the shipped SyncBN config."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import bn_reference as ref
from test_batchnorm_cpu import (SYNCBN, _bns, _inputs, _model, check_against_float64,
                                check_sync, phase, run_layer, sync_inputs)  # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HIP_PASSES = ["bn_train_stats", "bn_train_apply", "bn_train_bwd_reduce", "bn_train_bwd_apply"]


def _recorded(fn):
    """fn() with the launch records on: (result, names of the recorded launches)."""
    from detectron2_tensorflow_amd.layers.ops import KernelTimer
    saved = (KernelTimer.enabled, KernelTimer.detail, KernelTimer.records)
    KernelTimer.reset()
    try:
        out = fn()
        names = [r[0] for r in KernelTimer.records]
    finally:
        KernelTimer.enabled, KernelTimer.detail, KernelTimer.records = saved
    return out, names


# ------------------------------------------------------ 5. HIP arm vs float64
SHAPES = [(2, 5, 7, 4), (1, 1, 1, 8), (3, 9, 11, 24), (2, 3, 5, 2048), (1, 67, 61, 64), (70, 32)]


@pytest.mark.parametrize("shape", SHAPES)
def test_hip_arm_vs_float64_and_deterministic(dev, shape):
    """Inputs 30 + 0.3 * randn: a cancelling variance formula misses the bar by
    an order of magnitude, a stable one meets it.  Two runs: the same bits."""
    t = _inputs(shape, 11)
    got, names = _recorded(lambda: run_layer(t, dev))
    assert [n for n in names if n.startswith("bn_train")] == HIP_PASSES
    check_against_float64(got, t)
    again = run_layer(t, dev)
    for k, v in got.items():
        assert v is None or torch.equal(v, again[k]), k
    if shape == (1, 1, 1, 8):  # one row: var = 0, invstd = rsqrt(eps)
        assert torch.equal(got["var"], torch.zeros_like(got["var"]))
        ref.close(got["invstd"], torch.full((8,), 1e-5, dtype=torch.float64) ** -0.5, "invstd")


@pytest.mark.parametrize("kw", [{"center": False}, {"scale": False},
                                {"center": False, "scale": False}])
def test_hip_arm_without_gamma_or_beta(dev, kw):
    t = _inputs((3, 9, 11, 24), 12)
    check_against_float64(run_layer(t, dev, **kw), t, **kw)


# ---------------------------------------------------------- 6. fused variants
@pytest.mark.parametrize("shape", [(3, 9, 11, 24), (1, 67, 61, 64), (2, 3, 5, 2048)])
@pytest.mark.parametrize("kw", [{"relu": True}, {"residual": True},
                                {"relu": True, "residual": True},
                                {"relu": True, "residual": True, "relu_after_add": True}])
def test_hip_fused_relu_and_residual(dev, shape, kw):
    kw = dict(kw)
    t = _inputs(shape, 13, kw.pop("residual", False))
    got = run_layer(t, dev, **kw)
    check_against_float64(got, t, **kw)
    again = run_layer(t, dev, **kw)
    for k, v in got.items():
        assert v is None or torch.equal(v, again[k]), k


# ------------------------------------------------------ 7. HIP vs tensor arm
@pytest.mark.parametrize("kw", [{}, {"relu": True, "residual": True, "relu_after_add": True}])
def test_toggle_selects_the_arm_and_the_arms_agree(dev, kw):
    """FUSED_BN_TRAIN is read where the passes are chosen: the launch records
    hold the four HIP passes with it on and none with it off (a write that
    reached no reader would fail here); the arms agree within the bar."""
    from detectron2_tensorflow_amd.layers.ops import norm
    kw = dict(kw)
    t = _inputs((1, 67, 61, 64), 14, kw.pop("residual", False))
    assert norm.FUSED_BN_TRAIN is True
    hip, names = _recorded(lambda: run_layer(t, dev, **kw))
    assert [n for n in names if n.startswith("bn_train")] == HIP_PASSES
    norm.FUSED_BN_TRAIN = False
    try:
        ten, names = _recorded(lambda: run_layer(t, dev, **kw))
    finally:
        norm.FUSED_BN_TRAIN = True
    assert not [n for n in names if n.startswith("bn_train")]
    for k, v in ten.items():
        if v is not None:
            assert v.is_cuda
            ref.close(hip[k], v, k)
    check_against_float64(ten, t, **kw)


def test_channels_not_a_multiple_of_four_take_the_tensor_arm(dev):
    t = _inputs((3, 4, 5, 6), 15)
    got, names = _recorded(lambda: run_layer(t, dev))
    assert not [n for n in names if n.startswith("bn_train")]
    check_against_float64(got, t)


def test_host_refuses_bad_arguments_before_any_launch(dev):
    from detectron2_tensorflow_amd import _C
    lib = _C.lib()
    rc = lib.d2mi_bn_train_apply(None, 8, 6, None, None, None, None, None, 0, None, None)
    assert rc < 0 and "multiple of 4" in _C.last_error()
    x = torch.zeros(17, device=dev)
    rc = lib.d2mi_bn_train_finalize(x.data_ptr(), 1, 8, 1e-5, 0.9, None, None, x.data_ptr(),
                                    x.data_ptr(), x.data_ptr(), None)
    assert rc < 0 and "moving" in _C.last_error()
    size = lib.d2mi_bn_train_stats_workspace_size(4087, 64)
    rc = lib.d2mi_bn_train_stats(x.data_ptr(), 4087, 64, x.data_ptr(), x.data_ptr(), size - 1, None)
    assert rc < 0 and f"{size - 1} < {size}" in _C.last_error()


# ------------------------------------------------------------ 8. through Conv2D
def _bn64(y, bn):
    """Batch-statistics BatchNorm as differentiable float64 torch ops."""
    rows = y.reshape(-1, y.shape[-1])
    mean = rows.mean(0)
    var = ((rows - mean) ** 2).mean(0)
    return (y - mean) / torch.sqrt(var + bn.epsilon) * bn.gamma64 + bn.beta64, mean, var


def _conv64(x, conv):
    w = conv.w64.permute(3, 2, 0, 1)
    p = (conv.kernel_size - 1) // 2
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, None, stride=conv.stride,
                                      padding=p).permute(0, 2, 3, 1)


def _leaves64(convs):
    """float64 leaf copies of the convs' parameters (on the CPU)."""
    for c in convs:
        c.w64 = c.weights.detach().double().cpu().requires_grad_(True)
        bn = c.normalizer_fn
        bn.gamma64 = bn.gamma.detach().double().cpu().requires_grad_(True)
        bn.beta64 = bn.beta.detach().double().cpu().requires_grad_(True)


def _randomize(convs, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for c in convs:
            bn = c.normalizer_fn
            bn.gamma.copy_(0.5 + torch.rand(bn.channels, generator=g))
            bn.beta.copy_(0.3 * torch.randn(bn.channels, generator=g))
            bn.moving_mean.copy_(torch.randn(bn.channels, generator=g))
            bn.moving_variance.copy_(0.5 + torch.rand(bn.channels, generator=g))


def _check_grads(convs, x, x64):
    ref.close(x.grad, x64.grad, "dx")
    for c in convs:
        bn = c.normalizer_fn
        ref.close(c.weights.grad, c.w64.grad, c.scope + " dw")
        ref.close(bn.gamma.grad, bn.gamma64.grad, c.scope + " dgamma")
        ref.close(bn.beta.grad, bn.beta64.grad, c.scope + " dbeta")


@pytest.fixture
def fold_calls(monkeypatch):
    """The calls of the FrozenBN fold (one layer or batched) while the test
    runs, as Conv2D reaches them (ops.fold_frozen_bn / ops.fold_frozen_bn_many)."""
    from detectron2_tensorflow_amd.layers import ops
    calls = []
    for name in ("fold_frozen_bn", "fold_frozen_bn_many"):
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("k", [3, 1])
def test_conv2d_with_batch_stats_bn(dev, k, fold_calls):
    """3x3: relu(bn(conv(x))); 1x1: relu(bn(conv(x)) + residual) (final_relu),
    on the MFMA conv: outputs, the moving update and every gradient against
    float64; nothing was folded."""
    from detectron2_tensorflow_amd.layers import BatchNorm, Conv2D
    g = torch.Generator().manual_seed(30 + k)
    conv = Conv2D(16, 16, k, use_bias=False, activation="relu" if k == 3 else None,
                  normalizer=BatchNorm, normalizer_params={"training": True}, impl="mfma",
                  scope=f"conv{k}").to(dev)
    _randomize([conv], k)
    bn = conv.normalizer_fn
    mm0, mv0 = bn.moving_mean.clone(), bn.moving_variance.clone()
    xs = torch.randn(2, 8, 8, 16, generator=g)
    rs = torch.randn(2, 8, 8, 16, generator=g)
    dy = torch.randn(2, 8, 8, 16, generator=g)
    x = xs.to(dev).requires_grad_(True)
    r = rs.to(dev).requires_grad_(True)
    y = conv(x) if k == 3 else conv(x, residual=r, final_relu=True)
    y.backward(dy.to(dev))
    _leaves64([conv])
    x64, r64 = xs.double().requires_grad_(True), rs.double().requires_grad_(True)
    z, mean, var = _bn64(_conv64(x64, conv), bn)
    y64 = torch.relu(z) if k == 3 else torch.relu(z + r64)
    y64.backward(dy.double())
    ref.close(y, y64, "y")
    _check_grads([conv], x, x64)
    if k == 1:
        ref.close(r.grad, r64.grad, "dresidual")
    ref.close(bn.moving_mean, mm0.double().cpu() * 0.9 + mean.detach() * 0.1, "moving_mean")
    ref.close(bn.moving_variance, mv0.double().cpu() * 0.9 + var.detach() * 0.1, "moving_var")
    # nothing was folded: the BatchNorm is the normalizer still to apply, on
    # the layer's own weights, and no fold ran (the frozen test below shows
    # that the same counter sees the folds of the inference form)
    assert fold_calls == []
    w, b, norm, packed = conv.effective_params(want_packed=True)
    assert w is conv.weights and norm is bn and packed is None and fold_calls == []


def _block(norm, dev, phase):
    from detectron2_tensorflow_amd.modeling.backbone.resnet import (BottleneckBlock,
                                                                   resnet_arg_scope)
    phase(True)
    torch.manual_seed(3)
    with resnet_arg_scope(False, norm):
        block = BottleneckBlock(16, 16, 8, scope="block").to(dev)
    convs = [block.conv1, block.conv2, block.conv3]
    _randomize(convs, 4)
    return block, convs


def test_bottleneck_block_with_batch_stats_bn(dev, phase, fold_calls):
    block, convs = _block("BN", dev, phase)
    assert all(c._bn_batch_stats for c in convs) and block.shortcut is None
    before = [c.normalizer_fn.moving_mean.clone() for c in convs]
    g = torch.Generator().manual_seed(5)
    xs, dy = torch.randn(2, 6, 6, 16, generator=g), torch.randn(2, 6, 6, 16, generator=g)
    x = xs.to(dev).requires_grad_(True)
    block.train()
    y = block(x)
    y.backward(dy.to(dev))
    _leaves64(convs)
    x64 = xs.double().requires_grad_(True)
    h = torch.relu(_bn64(_conv64(x64, convs[0]), convs[0].normalizer_fn)[0])
    h = torch.relu(_bn64(_conv64(h, convs[1]), convs[1].normalizer_fn)[0])
    y64 = torch.relu(_bn64(_conv64(h, convs[2]), convs[2].normalizer_fn)[0] + x64)
    y64.backward(dy.double())
    ref.close(y, y64, "y")
    _check_grads(convs, x, x64)
    for c, b in zip(convs, before):
        assert not torch.equal(c.normalizer_fn.moving_mean, b)
        assert c.effective_params()[2] is c.normalizer_fn
    assert fold_calls == []


# ------------------------------------------------------ 9. frozen path untouched
def test_frozen_block_is_the_fold_path_and_keeps_its_buffers(dev, phase, fold_calls):
    from detectron2_tensorflow_amd.layers import ops
    block, convs = _block("FrozenBN", dev, phase)
    assert not any(c._bn_batch_stats for c in convs)
    state = {k: v.clone() for k, v in block.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 6, 6, 16, generator=g).to(dev)
    with torch.no_grad():
        got = block(x)
        h = x
        for i, c in enumerate(convs):  # the fold and the fused conv, as Conv2D.call runs them
            n = c.normalizer_fn
            _, b, packed = ops.fold_frozen_bn(c.weights, None, n.gamma, n.beta, n.moving_mean,
                                              n.moving_variance, n.epsilon, True)
            p = (c.kernel_size - 1) // 2
            h = ops.conv2d_nhwc(h, packed, b, 1, (p, p), True, None, x if i == 2 else None,
                                relu_after_add=i == 2)
    assert torch.equal(got, h)
    block.train()  # a training step: torch's flag must not thaw the layers
    xg = x.clone().requires_grad_(True)
    del fold_calls[:]
    block(xg).sum().backward()
    assert len(fold_calls) == 3  # one fold per conv: the inference form is the fold path
    assert xg.grad is not None and convs[0].weights.grad is not None
    for k, v in block.state_dict().items():
        assert torch.equal(v, state[k]), k


# ------------------------------------------------------------ 10. sync, 2 ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sync_two_ranks_on_the_gpu(dev, tmp_path):
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "bn_sync_worker.py"),
                               str(tmp_path)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=120)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} exit {p.returncode}:\n{o[-4000:]}"
    ranks = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=True) for r in range(2)]
    for r in ranks:
        assert [n for n in r.pop("launches") if n.startswith("bn_train")] == HIP_PASSES
    ts, whole = sync_inputs()
    one = {k: (v if v is None else v.cpu()) for k, v in run_layer(whole, dev).items()}
    check_against_float64(one, whole)
    check_sync(ranks, ts, one)


# ---------------------------------------------- 11. one Trainer step, SyncBN config
def test_trainer_step_of_the_syncbn_config(dev, phase):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.engine import Trainer
    from detectron2_tensorflow_amd.utils.synthetic import synthetic_train_batch
    torch.manual_seed(0)
    cfg, model = _model(SYNCBN, True)
    model = model.to(dev).train()
    bns = _bns(model, "")
    live = [m for m in bns if m.batch_stats]
    frozen = [m for m in bns if not m.batch_stats]
    assert len(live) == 58 and len(frozen) == 11
    before = [(m.moving_mean.clone(), m.moving_variance.clone()) for m in bns]
    losses = Trainer(cfg, model).step(synthetic_train_batch(2, 256, 320, 0, dev))
    _C.raise_on_errors(dev)
    assert all(torch.isfinite(v).all() for v in losses.values()), losses
    for m, (mm, mv) in zip(bns, before):
        assert torch.isfinite(m.moving_mean).all() and torch.isfinite(m.moving_variance).all()
        if m.batch_stats:
            assert not torch.equal(m.moving_mean, mm) and not torch.equal(m.moving_variance, mv)
        else:
            assert torch.equal(m.moving_mean, mm) and torch.equal(m.moving_variance, mv)
    assert all(m.gamma.grad is not None for m in live)
