"""GPU tests of the sparse RPN-head backward: the row census of a gradient map
(d2mi_row_census), the weight gradient over its chunk bitmap
(d2mi_conv2d_wgrad_rows), the data gradient over its dilated row list
(d2mi_conv2d_nhwc_rows) and the declared row bound that switches them on in
the model.  Every comparison is torch.equal against the dense entry point in
the same process."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = {"num_thing_classes": 80, "num_stuff_classes": 53, "stuff_ignore_value": 0}
WS_KERNELS = ("ws", "ws_inc")


class _Counter:
    sparse_launches = 0


def _restated_census(G):
    """(bitmap words as python ints, non-zero rows) of G [N, H, W, C] in torch."""
    bits = G.contiguous().view(torch.int32) & 0x7fffffff
    nz = (bits != 0).any(-1).flatten().cpu()
    M = nz.numel()
    nchunks = (M + 31) // 32
    pad = torch.zeros(nchunks * 32, dtype=torch.bool)
    pad[:M] = nz
    chunk = pad.view(nchunks, 32).any(1).tolist()
    words = [0] * ((nchunks + 31) // 32)
    for c, s in enumerate(chunk):
        if s:
            words[c // 32] |= 1 << (c % 32)
    return words, int(nz.sum())


def _restated_list(G, k=3, pad=1):
    """Sorted output rows of a k x k stride-1 conv over G whose window holds a
    non-zero row (per image: nothing crosses an image border)."""
    bits = G.contiguous().view(torch.int32) & 0x7fffffff
    nz = (bits != 0).any(-1).float()[:, None]  # [N, 1, H, W]
    # output (y, x) reads inputs (y - pad + d): a max filter with that window
    padded = torch.nn.functional.pad(nz, (pad, k - 1 - pad, pad, k - 1 - pad))
    dil = torch.nn.functional.max_pool2d(padded, k, stride=1)
    return torch.nonzero(dil.flatten() > 0).flatten().cpu().tolist()


def _words(census):
    return [int(w) & 0xffffffff for w in census.bitmap.cpu().tolist()]


def _edge_pixels():
    # first pixel, a row end, the last row of image 0, the last pixel (1,040
    # pixels = 32.5 chunks: the last chunk is partial)
    return [0, 3 * 26 + 25, 19 * 26 + 7, 2 * 20 * 26 - 1]


def test_row_census_bitmap_and_count(dev):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers import ops
    torch.manual_seed(0)
    G = torch.zeros(2, 20, 26, 16, device=dev)
    flat = G.view(-1, 16)
    for p in _edge_pixels():
        flat[p] = torch.randn(16, device=dev)
    flat[600, 5] = float("nan")   # a NaN counts as non-zero
    flat[700] = -0.0              # a row of -0.0 only is a zero row
    assert torch.signbit(flat[700]).all()
    census = ops.row_census(G, 512, dilate=(3, 1))
    words, rows = _restated_census(G)
    assert rows == 5 and len(words) == 2
    assert _words(census) == words
    assert int(census.count.item()) == rows
    # chunk 700 // 32 holds the -0.0 row and nothing else: its bit is clear
    assert not (words[(700 // 32) // 32] >> ((700 // 32) % 32)) & 1
    assert (words[1] >> 0) & 1  # chunk 32: the 16 pixels of the partial last chunk
    _C.raise_on_errors(dev)     # 5 rows <= 512: no error
    # the dilated list: sorted, duplicate-free, inside each image
    want = _restated_list(G)
    n = int(census.nrows.item())
    got = census.rows.cpu().tolist()[:n]
    assert census.list_capacity == 1040 and n == len(want) and got == want
    assert got == sorted(set(got))
    assert 3 * 26 + 24 in got and 4 * 26 + 25 in got      # the row end's own neighbours
    assert 4 * 26 + 0 not in got                          # not the next row's first pixel
    assert 18 * 26 + 7 in got and 520 + 7 not in got      # image 0's last row stays in image 0
    assert 1 in got and 26 in got and 27 in got and 1039 - 27 in got
    # a dense map: every bit of the 33 chunks, every row
    full = ops.row_census(torch.ones(2, 20, 26, 4, device=dev), 2 * 20 * 26)
    assert _words(full) == [0xffffffff, 1] and int(full.count.item()) == 1040
    _C.raise_on_errors(dev)


def test_row_census_reports_a_false_bound_and_stays_inside_its_workspace(dev):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers import ops
    lib = _C.lib()
    G = torch.zeros(2, 20, 26, 16, device=dev)
    for p in (0, 40, 300, 520, 777, 1039):
        G.view(-1, 16)[p, p % 16] = 1.0
    size = ops.row_census_workspace_size(2, 20, 26, 4, 3)
    out = (_C.ctypes.c_int64 * 7)()
    assert lib.d2mi_row_census_layout(2, 20, 26, 4, 3, out, 7) == 0
    boff, words, roff, coff, noff, loff, cap = out
    assert cap == 36 and loff + 4 * cap == size  # the list is the last part
    buf = torch.full((size + 256,), 0xAB, dtype=torch.uint8, device=dev)
    _C.raise_on_errors(dev)  # (clean before)
    rc = lib.d2mi_row_census(_C.ptr(G), 2, 20, 26, 16, 4, 3, 1, _C.ptr(buf), size,
                             _C.stream_of(dev))
    assert rc == 0
    with pytest.raises(_C.D2MIError, match="non-zero gradient rows"):
        _C.raise_on_errors(dev)
    _C.raise_on_errors(dev)  # (raise_on_errors cleared the word)
    host = buf.cpu()
    assert (host[size:] == 0xAB).all()  # the guard band after the list is untouched
    assert (host[coff + 4:coff + 4 + 64] == 0xAB).all() and (host[noff + 4:noff + 4 + 64] == 0xAB).all()
    assert int(host[coff:coff + 4].view(torch.int32).item()) == 6  # the true count, reported
    # 6 rows dilate to more than 36: the count is clamped, the list holds the first 36
    full = _restated_list(G)
    assert len(full) > cap
    assert int(host[noff:noff + 4].view(torch.int32).item()) == cap
    assert host[loff:loff + 4 * cap].view(torch.int32).tolist() == full[:cap]
    want, _ = _restated_census(G)
    assert [int(w) & 0xffffffff for w in host[boff:boff + 4 * words].view(torch.int32).tolist()] == want


@pytest.fixture(scope="module")
def wgrad_case(dev):
    """x, a sparse dy (non-zero rows at the edge pixels) of the [2, 20, 26, 256]
    3x3 conv, and dense reference gradients, made once."""
    from detectron2_tensorflow_amd.layers import ops
    plan = ops.wgrad_plan(2, 20, 26, 256, 256, 3, 1, (1, 1))
    # the warp-specialised kernel with 2 pixel splits
    assert ops.WGRAD_KERNELS[plan["kernel"]] in WS_KERNELS and plan["splits"] == 2, plan
    torch.manual_seed(1)
    x = torch.randn(2, 20, 26, 256, device=dev)
    dy = torch.zeros(2, 20, 26, 256, device=dev)
    for p in _edge_pixels() + [515, 516, 517]:
        dy.view(-1, 256)[p] = torch.randn(256, device=dev)
    dw, db = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), with_bias=True)
    return x, dy, dw, db


@pytest.mark.parametrize("bitmap", ["exact", "superset", "full"])
def test_wgrad_rows_matches_dense_bit_for_bit(dev, wgrad_case, bitmap):
    from detectron2_tensorflow_amd.layers import ops
    x, dy, dw, db = wgrad_case
    src = dy
    if bitmap == "superset":
        src = dy.clone()
        src.view(-1, 256)[[64, 65, 900]] = 1.0
    elif bitmap == "full":
        src = torch.ones(2, 20, 26, 4, device=dev)
    n = _Counter()
    census = ops.row_census(src, 1040, owner=n)
    got_w, got_b = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), with_bias=True, census=census)
    assert n.sparse_launches == 1  # the bitmap kernel ran
    assert torch.equal(got_w, dw) and torch.equal(got_b, db)
    # without a bias gradient
    got = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), census=census)
    assert n.sparse_launches == 2 and torch.equal(got, dw)


def test_wgrad_rows_with_an_empty_bitmap_writes_zeros(dev, wgrad_case):
    from detectron2_tensorflow_amd.layers import ops
    x = wgrad_case[0]
    dy = torch.zeros(2, 20, 26, 256, device=dev)
    n = _Counter()
    census = ops.row_census(dy, 0, owner=n)
    assert _words(census) == [0, 0]
    want_w, want_b = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), with_bias=True)
    got_w, got_b = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), with_bias=True, census=census)
    assert n.sparse_launches == 1
    assert torch.equal(got_w, want_w) and torch.equal(got_b, want_b)
    assert not got_w.any() and not torch.signbit(got_w).any()


def test_wgrad_rows_accumulates_into_nonzero_buffers(dev, wgrad_case):
    from detectron2_tensorflow_amd.layers import ops
    x, dy, _, _ = wgrad_case
    torch.manual_seed(2)
    w0, b0 = torch.randn(3, 3, 256, 256, device=dev), torch.randn(256, device=dev)
    want = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), with_bias=True,
                            accumulate_into=(w0.clone(), b0.clone()))
    n = _Counter()
    census = ops.row_census(dy, 1040, owner=n)
    got = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), with_bias=True,
                           accumulate_into=(w0.clone(), b0.clone()), census=census)
    assert n.sparse_launches == 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], w0)


def test_wgrad_rows_runs_dense_where_the_plan_has_another_kernel(dev):
    """A 64 -> 64 3x3 is not on the warp-specialised kernel: the bitmap is
    ignored and the dense launch runs (and is counted as dense)."""
    from detectron2_tensorflow_amd.layers import ops
    plan = ops.wgrad_plan(2, 20, 26, 64, 64, 3, 1, (1, 1))
    assert ops.WGRAD_KERNELS[plan["kernel"]] not in WS_KERNELS
    torch.manual_seed(3)
    x = torch.randn(2, 20, 26, 64, device=dev)
    dy = torch.zeros(2, 20, 26, 64, device=dev)
    dy.view(-1, 64)[[0, 500, 1039]] = torch.randn(3, 64, device=dev)
    n = _Counter()
    census = ops.row_census(dy, 1040, owner=n)
    got = ops.conv2d_wgrad(x, dy, 3, 1, (1, 1), census=census)
    assert n.sparse_launches == 0
    assert torch.equal(got, ops.conv2d_wgrad(x, dy, 3, 1, (1, 1)))


DGRAD_SHAPES = {"split_k": (2, 20, 26), "unsplit": (1, 100, 256), "tail": (1, 130, 256)}


@pytest.fixture(scope="module")
def dgrad_weights(dev):
    torch.manual_seed(4)
    return torch.randn(3, 3, 256, 256, device=dev) * 0.05  # packed [KH, KW, Cout, Cin]


@pytest.mark.parametrize("variant", ["plain", "residual", "gated"])
@pytest.mark.parametrize("shape", list(DGRAD_SHAPES))
def test_dgrad_rows_matches_dense_bit_for_bit(dev, dgrad_weights, shape, variant):
    from detectron2_tensorflow_amd.layers import ops
    N, H, W = DGRAD_SHAPES[shape]
    M = N * H * W
    operands = ops.OP_ALL_ALIGNED | ops.OP_WORKSPACE | (
        ops.OP_RESIDUAL if variant != "plain" else 0) | (ops.OP_GATE if variant == "gated" else 0)
    plan = ops.conv_plan(N, H, W, 256, 256, 3, 1, (1, 1), flags=12, operands=operands)
    if shape == "split_k":
        assert plan["main_splits"] > 1 and plan["tail_tiles"] == 0, plan
    elif shape == "unsplit":
        assert plan["main_splits"] == 1 and plan["tail_tiles"] == 0, plan
    elif plan["tail_tiles"] == 0:
        pytest.skip("no tail launch in this device's plan of the 260-tile shape")
    capacity = 64 if shape == "split_k" else 256
    assert 9 * capacity + 127 < plan["main_m_end"]  # (the row-list launch is taken)
    torch.manual_seed(5)
    gy = torch.zeros(N, H, W, 256, device=dev)
    pix = [0, W - 1, W, M // 2, M // 2 + 1, M - 1]
    if plan["tail_tiles"]:
        b = plan["tail_m_base"]
        pix += [b - W - 1, b - 1, b, b + 1, b + W]  # windows on both sides of the tail's first row
    gy.view(-1, 256)[pix] = torch.randn(len(pix), 256, device=dev)
    res = gate = None
    if variant != "plain":
        res = torch.randn(N, H, W, 256, device=dev)
        res.view(-1)[::7] = -0.0  # 0.f + (-0.0) = +0.0 in the dense epilogue: an add, not a copy
    if variant == "gated":
        gate = torch.randn(N, H, W, 256, device=dev)
    want = ops.conv2d_nhwc(gy, dgrad_weights, None, 1, (1, 1), flip_taps=True, residual=res,
                           relu_gate=gate)
    n = _Counter()
    census = ops.row_census(gy, capacity, dilate=(3, 1), owner=n)
    got = ops.conv2d_nhwc(gy, dgrad_weights, None, 1, (1, 1), flip_taps=True, residual=res,
                          relu_gate=gate, census=census)
    assert n.sparse_launches == 1  # the row-list launch ran
    assert torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))  # (+0.0 / -0.0 alike)
    assert got.view(-1, 256)[pix].abs().sum() > 0


def test_dgrad_rows_runs_dense_when_the_list_is_no_shorter_than_the_launch(dev, dgrad_weights):
    from detectron2_tensorflow_amd.layers import ops
    torch.manual_seed(6)
    gy = torch.zeros(2, 20, 26, 256, device=dev)
    gy.view(-1, 256)[[3, 700]] = torch.randn(2, 256, device=dev)
    n = _Counter()
    census = ops.row_census(gy, 512, dilate=(3, 1), owner=n)  # 9 x 512 > 1,040 pixels
    got = ops.conv2d_nhwc(gy, dgrad_weights, None, 1, (1, 1), flip_taps=True, census=census)
    assert n.sparse_launches == 0
    assert torch.equal(got, ops.conv2d_nhwc(gy, dgrad_weights, None, 1, (1, 1), flip_taps=True))


def test_training_step_with_sparse_rows_matches_dense_bit_for_bit(dev, monkeypatch):
    """One 256 x 320 training step with StandardRPNHead.SPARSE_ROWS on and off:
    every loss and every parameter gradient is equal bit for bit, the on arm
    ran the bitmap weight gradient and the row-list data gradient (p2: 10,240
    pixels against 9 x 512), the off arm made no bound at all."""
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.config import finalize, get_cfg
    from detectron2_tensorflow_amd.layers import handoff
    from detectron2_tensorflow_amd.modeling import build_model
    from detectron2_tensorflow_amd.modeling.proposal_generator.rpn import StandardRPNHead
    from detectron2_tensorflow_amd.utils.synthetic import (calibrate_rcnn_scores,
                                                           synthetic_train_batch)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-InstanceSegmentation",
                                     "mask_rcnn_R_50_FPN_1x.yaml"))
    cfg.MODEL.SEGMENTATION_OUTPUT.FORMAT = "raw"
    finalize(cfg, True, 1, CATS)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).train()
    batch = synthetic_train_batch(2, 256, 320, 6, dev)
    calibrate_rcnn_scores(model, batch)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    made = []

    class Spy(handoff.RowBound):
        __slots__ = ()

        def __init__(self, n, dilate=None):
            super().__init__(n, dilate)
            made.append(self)

    monkeypatch.setattr(handoff, "RowBound", Spy)
    # (at 256 x 320 the list is 45 % of p2's rows: let it through, to run the
    # row-list data gradient inside the model too)
    monkeypatch.setattr(Spy, "LIST_MAX_FRACTION", 1.0)
    grads, lossv = {}, {}
    for sparse in (True, False):
        monkeypatch.setattr(StandardRPNHead, "SPARSE_ROWS", sparse)
        made.clear()
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        losses = model(batch)
        sum(losses.values()).backward()
        _C.raise_on_errors(dev)  # (the declared bound held)
        if sparse:
            assert len(made) == 1 and made[0].declared and made[0].rows_per_image == 256
            assert made[0].sparse_launches >= 2  # p2: the bitmap wgrad and the row-list dgrad
        else:
            assert made == []
        lossv[sparse] = {k: v.detach().clone() for k, v in losses.items()}
        grads[sparse] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert lossv[True].keys() == lossv[False].keys()
    for k in lossv[True]:
        assert torch.equal(lossv[True][k], lossv[False][k]), k
    assert grads[True].keys() == grads[False].keys()
    assert any("rpn_head.conv." in n for n in grads[True]), sorted(grads[True])  # the shared 3x3
    for n in grads[True]:
        assert torch.equal(grads[True][n], grads[False][n]), n
