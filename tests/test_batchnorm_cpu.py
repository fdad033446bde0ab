"""BatchNorm on batch statistics, the parts that need no GPU: which layers the
builders put into which form, the tensor arm of ops.batch_norm_train against
the float64 restatement (tests/bn_reference.py), SyncBN over gloo at world 2
with unequal row counts, and GraphedTrainer's refusal."""
import os
import socket

import pytest
import torch

import bn_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
SYNCBN = "configs/Misc/mask_rcnn_R_50_FPN_3x_syncbn.yaml"
FROZEN = "configs/COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_1x.yaml"


@pytest.fixture
def phase():
    """Sets the global training phase for one test and puts the old value back."""
    from detectron2_tensorflow_amd.utils import training
    old = training._TRAINING
    yield training.set_training_phase
    training._TRAINING = old


def _model(path, training):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, path))
    finalize(cfg, training=training, world_size=1, category_map=CATS)
    return cfg, build_model(cfg)


def _bns(model, *prefixes):
    from detectron2_tensorflow_amd.layers import BatchNorm
    return [m for n, m in model.named_modules()
            if isinstance(m, BatchNorm) and n.startswith(prefixes)]


# ------------------------------------------------------------ 1. mode table
def test_bare_layer_ignores_the_phase_and_frozen_training_raises(phase):
    from detectron2_tensorflow_amd.layers import BatchNorm
    phase(True)
    bn = BatchNorm(8)
    assert not bn.batch_stats and not bn.training
    bn.train()  # torch's flag is not the form
    assert not bn.batch_stats
    assert BatchNorm(8, training=True).batch_stats
    assert not BatchNorm(8, training=False).batch_stats
    assert BatchNorm(8, decay=0.5, training=True).decay == 0.5
    assert BatchNorm(8).decay == 0.9 and BatchNorm(8, momentum=0.5).momentum == 0.5
    with pytest.raises(ValueError, match="Frozen BatchNorm should not update EMA"):
        BatchNorm(8, training=True, trainable=False)


@pytest.mark.parametrize("norm,freeze,train,want", [
    ("FrozenBN", False, True, (False, False)), ("FrozenBN", True, True, (False, False)),
    ("BN", True, True, (False, False)), ("SyncBN", True, True, (False, False)),
    ("BN", False, True, (True, False)), ("SyncBN", False, True, (True, True)),
    ("BN", False, False, (False, False)), ("SyncBN", False, False, (False, True)),
    ("BN", False, None, (False, False)),
])
def test_resnet_arg_scope_table(phase, norm, freeze, train, want):
    """resnet_arg_scope(freeze, norm) under the phase ``train`` (None: unset)
    -> (batch_stats, sync) of the conv's BatchNorm."""
    from detectron2_tensorflow_amd.layers import Conv2D
    from detectron2_tensorflow_amd.modeling.backbone.resnet import resnet_arg_scope
    from detectron2_tensorflow_amd.utils import training
    if train is None:
        training._TRAINING = None
    else:
        phase(train)
    with resnet_arg_scope(freeze, norm):
        conv = Conv2D(8, 8, 3)
    bn = conv.normalizer_fn
    assert (bn.batch_stats, bool(bn.sync)) == want
    assert conv._bn_batch_stats == want[0]
    assert bn.trainable == (not freeze)


@pytest.mark.parametrize("norm,train,want", [("BN", True, True), ("SyncBN", True, True),
                                             ("BN", False, False), ("SyncBN", False, False),
                                             ("FrozenBN", True, False)])
def test_head_and_neck_scopes_pass_training_and_never_sync(phase, norm, train, want):
    """FPN / FastRCNNConvFCHead / the mask head: training = the phase for BN and
    SyncBN, no sync (the reference sets sync in the backbone scopes only)."""
    from detectron2_tensorflow_amd.layers import Conv2D
    from detectron2_tensorflow_amd.layers.normalization import batch_norm_arg_scope, get_norm
    phase(train)
    with batch_norm_arg_scope(norm):
        bn = Conv2D(8, 8, 3, normalizer=get_norm(norm)).normalizer_fn
    assert bn.batch_stats == want and not bn.sync


def test_syncbn_config_modes(phase):
    _, model = _model(SYNCBN, True)
    frozen = _bns(model, "backbone.stem", "backbone.stages.0")
    assert len(frozen) == 11
    assert not any(m.batch_stats for m in frozen)
    assert not any(p.requires_grad for m in frozen for p in m.parameters())
    res = _bns(model, "backbone.stages.1", "backbone.stages.2", "backbone.stages.3")
    assert len(res) == 42 and all(m.batch_stats and m.sync for m in res)
    rest = _bns(model, "neck", "roi_heads.box_head", "roi_heads.mask_head")
    assert len(rest) == 16 and all(m.batch_stats and not m.sync for m in rest)
    assert len(_bns(model, "")) == 11 + 42 + 16
    model.eval()  # the form is fixed at construction
    assert all(m.batch_stats for m in res + rest)


def test_syncbn_config_in_inference_and_frozen_config_have_no_batch_stats_layer(phase):
    _, model = _model(SYNCBN, False)
    assert len(_bns(model, "")) == 69 and not any(m.batch_stats for m in _bns(model, ""))
    model.train()
    assert not any(m.batch_stats for m in _bns(model, ""))


def test_frozen_config_in_training_has_no_batch_stats_layer(phase):
    _, model = _model(FROZEN, True)
    bns = _bns(model, "")
    assert len(bns) == 53 and not any(m.batch_stats for m in bns)


# ------------------------------------------------- 2. tensor arm vs float64
def _inputs(shape, seed, residual=False):
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = 30 + 0.3 * torch.randn(shape, generator=g)
    t = {"x": x, "gamma": 0.5 + torch.rand(C, generator=g), "beta": torch.randn(C, generator=g),
         "mm": torch.randn(C, generator=g), "mv": 0.5 + torch.rand(C, generator=g),
         "dy": torch.randn(shape, generator=g),
         "res": torch.randn(shape, generator=g) if residual else None}
    return t


def run_layer(t, dev, center=True, scale=True, relu=False, relu_after_add=False, decay=0.9,
              sync=False):
    """One forward + backward of a batch-statistics BatchNorm on ``dev`` from
    the tensors of _inputs: dict of y, mean, var, invstd, the moving
    statistics after the update and every gradient."""
    from detectron2_tensorflow_amd.layers import ops
    leaf = lambda v: v.detach().clone().to(dev).requires_grad_(True)
    x = leaf(t["x"])
    res = None if t["res"] is None else leaf(t["res"])
    gamma = leaf(t["gamma"]) if scale else None
    beta = leaf(t["beta"]) if center else None
    mm, mv = t["mm"].clone().to(dev), t["mv"].clone().to(dev)
    mode = 0
    if relu:
        mode = 2 if relu_after_add and res is not None else 1
    stats = {}
    y = ops.batch_norm_train(x, gamma, beta, mm, mv, 1e-5, decay, res, mode, sync, stats)
    y.backward(t["dy"].to(dev))
    out = {"y": y.detach(), "moving_mean": mm, "moving_var": mv, "dx": x.grad,
           "dgamma": None if gamma is None else gamma.grad,
           "dbeta": None if beta is None else beta.grad,
           "dresidual": None if res is None else res.grad}
    out.update(stats)
    return out


def check_against_float64(got, t, center=True, scale=True, relu=False, relu_after_add=False,
                          decay=0.9):
    """Every tensor of run_layer within the bar of the float64 restatement.
    The backward's ReLU mask is the checked forward's own y > 0 (after y has
    met the bar); it may differ from float64's only where float64's
    pre-activation is within the bar of zero."""
    gamma = t["gamma"] if scale else None
    beta = t["beta"] if center else None
    fwd = ref.forward(t["x"], gamma, beta, 1e-5, t["res"], relu, relu_after_add)
    for k in ("y", "mean", "var", "invstd"):
        ref.close(got[k], fwd[k], k)
    wm, wv = ref.moving(t["mm"], t["mv"], fwd, decay)
    ref.close(got["moving_mean"], wm, "moving_mean")
    ref.close(got["moving_var"], wv, "moving_var")
    mask = None
    if relu:
        after = relu_after_add and t["res"] is not None
        # relu(z) + residual: y > 0 is not z > 0; the mask is of y - residual
        pre = got["y"].cpu() if (after or t["res"] is None) else None
        m64, t64 = ref.relu_mask(fwd, t["res"], relu, relu_after_add)
        if pre is None:
            mask = m64  # (relu before the add: the forward's mask is not visible in y)
        else:
            mask = pre > 0
            near = int((t64.abs() <= ref.BAR * float(t64.abs().max())).sum())
            assert int((mask != m64).sum()) <= near
    bwd = ref.backward(fwd, t["dy"], gamma, mask)
    for k in ("dx", "dgamma", "dbeta", "dresidual"):
        if got[k] is None:
            assert k != "dx" and ((k == "dgamma" and not scale) or (k == "dbeta" and not center)
                                  or (k == "dresidual" and t["res"] is None)), k
            continue
        ref.close(got[k], bwd[k], k)


CASES = [
    ((2, 5, 7, 8), {}), ((2, 5, 7, 8), {"center": False}), ((2, 5, 7, 8), {"scale": False}),
    ((2, 5, 7, 8), {"center": False, "scale": False}),
    ((70, 32), {}), ((1, 1, 1, 8), {}), ((3, 4, 5, 3), {}), ((6, 3), {"relu": True}),
    ((2, 5, 7, 8), {"relu": True}), ((2, 5, 7, 8), {"residual": True}),
    ((2, 5, 7, 8), {"relu": True, "residual": True}),
    ((2, 5, 7, 8), {"relu": True, "residual": True, "relu_after_add": True}),
    ((2, 5, 7, 8), {"decay": 0.5}),
]


@pytest.mark.parametrize("shape,kw", CASES)
def test_tensor_arm_vs_float64(shape, kw):
    kw = dict(kw)
    t = _inputs(shape, 3, kw.pop("residual", False))
    got = run_layer(t, "cpu", **kw)
    check_against_float64(got, t, **kw)


def test_layer_call_updates_buffers_without_autograd():
    """BatchNorm.call in the batch-statistics form: the layer's own buffers
    move by decay 0.9, in place and outside autograd."""
    from detectron2_tensorflow_amd.layers import BatchNorm
    t = _inputs((2, 5, 7, 8), 5)
    bn = BatchNorm(8, training=True)
    with torch.no_grad():
        bn.gamma.copy_(t["gamma"]); bn.beta.copy_(t["beta"])
        bn.moving_mean.copy_(t["mm"]); bn.moving_variance.copy_(t["mv"])
    mm_id = bn.moving_mean.data_ptr()
    y = bn(t["x"], relu=True)
    fwd = ref.forward(t["x"], t["gamma"], t["beta"], 1e-5, None, True)
    ref.close(y, fwd["y"], "y")
    wm, wv = ref.moving(t["mm"], t["mv"], fwd, 0.9)
    ref.close(bn.moving_mean, wm, "moving_mean")
    ref.close(bn.moving_variance, wv, "moving_variance")
    assert bn.moving_mean.data_ptr() == mm_id and not bn.moving_mean.requires_grad
    # the inference form of the same parameters does not touch them
    frozen = BatchNorm(8)
    frozen.load_state_dict(bn.state_dict())
    before = frozen.moving_mean.clone()
    frozen.train()
    frozen(t["x"])
    assert torch.equal(frozen.moving_mean, before)


# ------------------------------------------------------ 3. sync over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SYNC_SHAPES = [(1, 5, 7, 8), (1, 3, 4, 8)]


def sync_inputs():
    """Per-rank tensors (shared gamma / beta / moving buffers) and the
    one-process case on the concatenated rows."""
    ts = [_inputs(s, 20 + r) for r, s in enumerate(SYNC_SHAPES)]
    for t in ts[1:]:
        for k in ("gamma", "beta", "mm", "mv"):
            t[k] = ts[0][k]
    whole = dict(ts[0])
    whole["x"] = torch.cat([t["x"].reshape(-1, 8) for t in ts])
    whole["dy"] = torch.cat([t["dy"].reshape(-1, 8) for t in ts])
    return ts, whole


def _sync_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ts, _ = sync_inputs()
    got = run_layer(ts[rank], "cpu", sync=True)
    torch.save(got, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def check_sync(ranks, ts, one):
    """ranks: run_layer's dict per rank (sync=True); one: the same layer in
    one process on the concatenated rows."""
    n0 = ts[0]["x"].numel() // 8
    ref.close(torch.cat([r["y"].reshape(-1, 8) for r in ranks]), one["y"], "y")
    ref.close(torch.cat([r["dx"].reshape(-1, 8) for r in ranks]), one["dx"], "dx")
    assert ranks[0]["y"].reshape(-1, 8).shape[0] == n0
    for k in ("moving_mean", "moving_var", "mean", "var"):
        ref.close(ranks[0][k], one[k], k)
    for k in ("dgamma", "dbeta"):
        ref.close(ranks[0][k] + ranks[1][k], one[k], k)
        assert not torch.equal(ranks[0][k], ranks[1][k])  # local sums, not the global ones
    for k in ("mean", "invstd", "var", "moving_mean", "moving_var"):
        assert torch.equal(ranks[0][k], ranks[1][k]), k


def test_sync_gloo_world2_unequal_rows(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_sync_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2)]
    ts, whole = sync_inputs()
    one = run_layer(whole, "cpu")
    check_against_float64(one, whole)
    check_sync(ranks, ts, one)


def test_sync_at_world_one_is_the_local_path():
    """sync=True with no process group: no collective, the same bits."""
    t = _inputs((2, 5, 7, 8), 9)
    a, b = run_layer(t, "cpu", sync=True), run_layer(t, "cpu", sync=False)
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


# ------------------------------------------------- 4. GraphedTrainer refuses
def test_graphed_trainer_refuses_batch_stats(phase):
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.engine.graphed import GraphedTrainer
    from detectron2_tensorflow_amd.layers import BatchNorm, Conv2D
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, FROZEN))
    finalize(cfg, training=True, world_size=1, category_map=CATS)

    class Tiny(torch.nn.Module):
        def __init__(self, training):
            super().__init__()
            self.conv = Conv2D(4, 4, 1, normalizer=BatchNorm,
                               normalizer_params={"training": training})

    with pytest.raises(NotImplementedError, match="batch statistics"):
        GraphedTrainer(cfg, Tiny(True))
    GraphedTrainer(cfg, Tiny(False))  # the inference form is no obstacle


# ------------------------------------------ refusals around the raw-conv path
def test_batch_stats_conv_refuses_slot_handoffs_and_topdown():
    """A conv under a batch-statistics BatchNorm runs without gradient
    hand-offs: a Slot it cannot honour is refused, not dropped."""
    from detectron2_tensorflow_amd.layers import BatchNorm, Conv2D, handoff
    conv = Conv2D(4, 4, 1, use_bias=False, normalizer=BatchNorm,
                  normalizer_params={"training": True}, impl="torch")
    x = torch.randn(1, 3, 3, 4)
    for kw in ({"res_grad_to": handoff.Slot()}, {"grad_from": handoff.Slot()}):
        with pytest.raises(ValueError, match="res_grad_to / grad_from"):
            conv(x, **kw)
    with pytest.raises(ValueError, match="top-down"):
        conv(x, topdown=torch.randn(1, 2, 2, 4))
    y = conv(x, residual=torch.randn(1, 3, 3, 4), final_relu=True, relu_input_sole_consumer=True)
    assert y.shape == x.shape and float(y.detach().min()) >= 0


def test_res5_dense_refuses_batch_stats():
    from detectron2_tensorflow_amd.layers import BatchNorm, Conv2D
    from detectron2_tensorflow_amd.modeling.roi_heads.res5_dense import conv_dense
    x = torch.randn(1, 3, 3, 4)
    live = Conv2D(4, 4, 1, use_bias=False, normalizer=BatchNorm,
                  normalizer_params={"training": True}, impl="torch")
    with pytest.raises(NotImplementedError, match="batch statistics"):
        conv_dense(x, live)
    frozen = Conv2D(4, 4, 1, use_bias=False, normalizer=BatchNorm, impl="torch")
    assert conv_dense(x, frozen).shape == x.shape
