"""GPU tests of the four fused training-loss kernels -- ops.rpn_loss
(csrc/rpn_loss.hip), ops.fast_rcnn_loss and ops.mask_loss
(csrc/roi_losses.hip), ops.retina_loss (csrc/retina_loss.hip) -- against the
float64 restatement of the reference (tests/loss_reference.py, pinned on the
CPU by tests/test_loss_reference_cpu.py), at the smallest shapes that reach
each code path of the kernels (the tables in ``loss_reference._cases``).

Every case checks: each loss (float32) and every gradient tensor against
float64 and float64 autograd; exact zeros wherever no loss reaches (the
restatement must agree that nothing reaches them); the ``_bwd`` C entry
called directly into NaN-prefilled buffers (no NaN left, the bits of the
autograd path); for Fast R-CNN and mask the normaliser in ``stats``, exactly
max(1, #valid) and max(1, #fg * P).  Further tests: bit-identical reruns of
one large case per kernel, a missing upstream gradient (null pointer for
RPN / RetinaNet, zero for Fast R-CNN), the RPN's folded ``scale``, and the
dirty cases against the same layout holding ordinary numbers (bit-equal).

Tolerance of every floating-point comparison (``allowed``), the convention
of tests/test_gpu_yolo_train.py: the restatement is run once more in float32
on the CPU; its error against float64 -- per loss |l32 - l64| / |l64|, per
gradient tensor max|g32 - g64| / max|g64| -- is the reference's own float32
error for that input.  The kernel is allowed 4 x that, with a floor of 2 ulp
of the value (2 * 2^-23 relative).  No bound is sized from a kernel's error;
no case needed the d * 2^-24 summation bound.  Exact-zero and bit-equality
assertions carry no tolerance.  A loss or gradient tensor that is exactly 0
in float64 must be exactly 0 from the kernel.

gamma in (0, 1) is out of scope: gamma q^(gamma - 1) * 0 is NaN once
q = 1 - p_t rounds to 0, in the kernel, in torch's autograd and in the
reference's TF alike, and no shipped config uses such a gamma.

Measured on an MI355X (relative errors; each test prints its own figures;
the per-kernel table is in DESIGN.md section 5, "Training losses"):
kernel       losses: reference f32 / kernel / allowed          gradient tensors: reference f32 / kernel / allowed
Fast R-CNN   4.5e-9..2.6e-6 / 1.3e-9..2.6e-6 / 2.4e-7..1.1e-5   3.7e-8..5.8e-5 / 1.7e-8..5.8e-5 / 2.4e-7..2.3e-4
RPN          4.2e-11..1.1e-6 / 8.5e-10..1.1e-6 / 2.4e-7..4.4e-6 1.2e-8..1.1e-5 / 1.2e-8..1.1e-5 / 2.4e-7..4.4e-5
mask         1.2e-9..9.9e-8 / 2.8e-8..9.9e-8 / 2.4e-7..3.9e-7   1.7e-8..1.4e-7 / 1.7e-8..1.4e-7 / 2.4e-7..5.5e-7
RetinaNet    1.4e-8..1.5e-7 / 8.7e-9..9.7e-8 / 2.4e-7..5.9e-7   5.1e-9..1.7e-6 / 5.1e-9..1.7e-6 / 2.4e-7..6.9e-6
No kernel used more than 0.43 of its bound.  (frcn/kink-b0's box loss is a sum of
subnormals, 2.3e-45: float32 and the kernel both round it to 2 quanta, 0.2 relative.)
"""
import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu
ULP2 = 2.0 * 2.0 ** -23
UP = R.UPSTREAM
_ref = {}


def reference(name):
    """The case, its float64 losses and gradients, and the float32
    restatement's error against them: computed once, never modified."""
    if name not in _ref:
        c = R.CASES[name]()
        o64 = R.run(c)
        g64 = R.gradients(o64)
        o32 = R.run(c, torch.float32)
        g32 = R.gradients(o32)
        err = [rel(a, b) for a, b in zip(o32, o64)]
        gerr = [grel(a, b) for a, b in zip(g32, g64)]
        _ref[name] = dict(case=c, out=[l.detach() for l in o64], grads=g64, err=err, gerr=gerr,
                          masks=R.counted_masks(c))
    return _ref[name]


def rel(got, want):
    got, want = float(got.detach()), float(want.detach())
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def grel(got, want):
    m = float(want.abs().max())
    d = float((got.double() - want).abs().max())
    return d / m if m != 0 else d


def allowed(ref_err):
    return max(4.0 * ref_err, ULP2)


def same_bits(a, b):
    """Equal as bit patterns (torch.equal takes -0.0 for +0.0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def to_dev(x, dev):
    if isinstance(x, (list, tuple)):
        return type(x)(to_dev(v, dev) for v in x)
    return x.to(dev)


def run_op(case, dev, scale=None):
    """(leaves, losses) of the fused op on the device."""
    from detectron2_tensorflow_amd.layers import ops
    k, a, conf = case["kernel"], to_dev(case["args"], dev), case["conf"]
    if k == "rpn":
        leaves = [a[0].requires_grad_(True), a[1].requires_grad_(True)]
        extra = () if scale is None else (scale,)
        out = ops.rpn_loss(*leaves, *a[2:], *conf, *extra)
    elif k == "frcn":
        leaves = [a[0].requires_grad_(True), a[1].requires_grad_(True)]
        out = ops.fast_rcnn_loss(*leaves, *a[2:], *conf)
    elif k == "mask":
        leaves = [a[0].requires_grad_(True)]
        out = (ops.mask_loss(*leaves, *a[1:]),)
    else:
        cls = [x.requires_grad_(True) for x in a[0]]
        box = [x.requires_grad_(True) for x in a[1]]
        leaves = cls + box
        out = ops.retina_loss(cls, box, *a[2:], *conf)
    return leaves, tuple(out)


def backward(leaves, out, upstream=UP):
    total = sum(u * l for u, l in zip(upstream, out) if u is not None)
    return torch.autograd.grad(total, leaves)


# ------------------------------------------------ the C entries, called directly
def _up(dev, k):
    return torch.tensor(UP[k], dtype=torch.float32, device=dev)


def abi_backward(case, dev):
    """Each ``_bwd`` entry into NaN-prefilled buffers the test owns ->
    (buffers, normaliser in stats or None)."""
    from detectron2_tensorflow_amd import _C
    lib = _C.lib()
    k, a, conf = case["kernel"], to_dev(case["args"], dev), case["conf"]
    st = _C.stream_of(dev)
    nan = float("nan")
    f32 = lambda x: x.float().contiguous()              # noqa: E731
    u8 = lambda x: x.to(torch.uint8).contiguous()       # noqa: E731
    i64 = lambda x: x.to(torch.int64).contiguous()      # noqa: E731
    if k == "rpn":
        logits, deltas, anchors, gt = (f32(x) for x in a[:4])
        matches, pos, samp = i64(a[4]), u8(a[5]), u8(a[6])
        N, P = logits.shape
        bufs = [torch.full_like(logits, nan), torch.full_like(deltas, nan)]
        g0, g1 = _up(dev, 0), _up(dev, 1)
        rc = lib.d2mi_rpn_loss_bwd_ex(
            _C.ptr(logits), _C.ptr(deltas), _C.ptr(anchors), _C.ptr(gt), _C.ptr(matches), _C.ptr(pos),
            _C.ptr(samp), N, P, gt.shape[1], _C.host_array(_C.c_float, list(conf[0])), float(conf[1]),
            _C.ptr(g0), _C.ptr(g1), 1.0, _C.ptr(bufs[0]), _C.ptr(bufs[1]), st)
        _C.check(rc, "d2mi_rpn_loss_bwd_ex")
        return bufs, None
    if k == "frcn":
        logits, deltas, props = f32(a[0]), f32(a[1]), f32(a[2])
        cls, gtb, valid = i64(a[3]), f32(a[4]), u8(a[5])
        B, K1 = logits.shape
        nreg = deltas.shape[1] // 4
        w = _C.host_array(_C.c_float, list(conf[0]))
        stats = torch.full((4,), nan, dtype=torch.float32, device=dev)
        wsb = lib.d2mi_fast_rcnn_loss_workspace_size(B)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        rc = lib.d2mi_fast_rcnn_loss_fwd(_C.ptr(logits), _C.ptr(deltas), _C.ptr(props), _C.ptr(cls),
                                         _C.ptr(gtb), _C.ptr(valid), B, K1, nreg, w, float(conf[1]),
                                         _C.ptr(stats), _C.ptr(ws), wsb, st)
        _C.check(rc, "d2mi_fast_rcnn_loss_fwd")
        grads = torch.tensor(UP, dtype=torch.float32, device=dev)
        bufs = [torch.full_like(logits, nan), torch.full_like(deltas, nan)]
        rc = lib.d2mi_fast_rcnn_loss_bwd(_C.ptr(logits), _C.ptr(deltas), _C.ptr(props), _C.ptr(cls),
                                         _C.ptr(gtb), _C.ptr(valid), B, K1, nreg, w, float(conf[1]),
                                         _C.ptr(stats), _C.ptr(grads), _C.ptr(bufs[0]), _C.ptr(bufs[1]),
                                         st)
        _C.check(rc, "d2mi_fast_rcnn_loss_bwd")
        return bufs, float(stats[3])
    if k == "mask":
        logits, target, classes, fg = f32(a[0]), f32(a[1]), i64(a[2]), u8(a[3])
        B, Hm, Wm, C = logits.shape
        stats = torch.full((3,), nan, dtype=torch.float32, device=dev)
        wsb = lib.d2mi_mask_loss_workspace_size(B)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        rc = lib.d2mi_mask_loss_fwd(_C.ptr(logits), _C.ptr(target), _C.ptr(classes), _C.ptr(fg), B,
                                    Hm * Wm, C, _C.ptr(stats), _C.ptr(ws), wsb, st)
        _C.check(rc, "d2mi_mask_loss_fwd")
        grads = torch.tensor(UP[:1], dtype=torch.float32, device=dev)
        bufs = [torch.full_like(logits, nan)]
        rc = lib.d2mi_mask_loss_bwd(_C.ptr(logits), _C.ptr(target), _C.ptr(classes), _C.ptr(fg), B,
                                    Hm * Wm, C, _C.ptr(stats), _C.ptr(grads), _C.ptr(bufs[0]), st)
        _C.check(rc, "d2mi_mask_loss_bwd")
        return bufs, float(stats[2])
    cls, box = [f32(x) for x in a[0]], [f32(x) for x in a[1]]
    anchors, gt, gcls, matches, labels = f32(a[2]), f32(a[3]), i64(a[4]), i64(a[5]), i64(a[6])
    K, A, alpha, gamma, beta, weights = conf
    L, N = len(cls), cls[0].shape[0]
    lvl = [int(c.shape[1] * c.shape[2] * A) for c in cls]
    bufs = [torch.full_like(x, nan) for x in cls + box]
    g0, g1 = _up(dev, 0), _up(dev, 1)
    pa = lambda ts: _C.host_array(_C.c_void_p, [t.data_ptr() for t in ts])  # noqa: E731
    rc = lib.d2mi_retina_loss_bwd(
        pa(cls), pa(box), pa(bufs[:L]), pa(bufs[L:]), _C.host_array(_C.ctypes.c_longlong, lvl), L, N, K,
        A, _C.ptr(anchors), _C.ptr(gt), _C.ptr(gcls), gt.shape[1], _C.ptr(matches), _C.ptr(labels),
        float(alpha), float(gamma), float(beta), _C.host_array(_C.c_float, list(weights)), _C.ptr(g0),
        _C.ptr(g1), st)
    _C.check(rc, "d2mi_retina_loss_bwd")
    return bufs, None


def normaliser(case):
    a = case["args"]
    if case["kernel"] == "frcn":
        return float(max(1, int(a[5].sum())))
    if case["kernel"] == "mask":
        return float(max(1, int(a[3].sum()) * a[0].shape[1] * a[0].shape[2]))
    return None


# --------------------------------------------------- every case of the tables
def check_case(dev, name):
    from detectron2_tensorflow_amd import _C
    ref = reference(name)
    case = ref["case"]
    leaves, out = run_op(case, dev)
    got = backward(leaves, out)
    _C.raise_on_errors(dev)
    lines, bad = [], []
    # forward
    for k, (l, want) in enumerate(zip(out, ref["out"])):
        assert l.dtype == torch.float32 and l.dim() == 0
        e, tol = rel(l, want), allowed(ref["err"][k])
        lines.append(f"{name} loss[{k}] = {float(want):.6g}: reference f32 {ref['err'][k]:.3e}, "
                     f"kernel {e:.3e}, allowed {tol:.3e}")
        if float(want) == 0.0:
            if float(l.detach()) != 0.0:
                bad.append(f"loss[{k}] is {float(l.detach())!r}, not exactly 0")
        elif not e <= tol:     # (a NaN fails)
            bad.append(f"loss[{k}]: {e:.3e} > {tol:.3e}")
    # backward
    for k, (g, want, m) in enumerate(zip(got, ref["grads"], ref["masks"])):
        g = g.cpu()
        assert g.dtype == torch.float32 and g.shape == want.shape
        assert bool((want[~m] == 0).all())        # the restatement agrees that nothing reaches them
        if not bool((g[~m] == 0).all()):
            bad.append(f"grad[{k}]: an element no loss reaches is not exactly 0")
        e, tol = grel(g, want), allowed(ref["gerr"][k])
        lines.append(f"{name} grad[{k}] max {float(want.abs().max()):.4g}: reference f32 "
                     f"{ref['gerr'][k]:.3e}, kernel {e:.3e}, allowed {tol:.3e}")
        if not want.any():
            if g.any() or bool(torch.isnan(g).any()):
                bad.append(f"grad[{k}] is not exactly 0")
        elif not e <= tol:
            bad.append(f"grad[{k}]: {e:.3e} > {tol:.3e}")
    print("\n".join(lines))
    assert not bad, bad
    # the C entry writes EVERY element: buffers the test owns, pre-filled with NaN
    bufs, norm = abi_backward(case, dev)
    _C.raise_on_errors(dev)
    for k, (b, g) in enumerate(zip(bufs, got)):
        assert not bool(torch.isnan(b).any()), f"grad[{k}]: an element was not written"
        assert same_bits(b, g), f"grad[{k}]: not the bits of the autograd path"
    assert norm == normaliser(case)
    return ref, got


@pytest.mark.parametrize("name", R.names("frcn"))
def test_fast_rcnn_loss_against_float64(dev, name):
    """One wave per row, four rows per block, lanes stride K1 by 64; one
    256-thread block reduces the rows."""
    ref, got = check_case(dev, name)
    if "kink" in name:   # the gradient at t - p = 0 is exactly 0, on either side of it +-1/R or +-d/(beta R)
        logits, deltas, _, cls, _, _ = ref["case"]["args"]
        B = logits.shape[0]
        pred = deltas.reshape(B, -1, 4)[torch.arange(B), cls]
        g = got[1].cpu().reshape(B, -1, 4)[torch.arange(B), cls]
        assert bool((pred == 0).any()) and bool((g[pred == 0] == 0).all())
        assert bool((torch.sign(g[pred != 0]) == torch.sign(pred[pred != 0])).all())
    if name in ("frcn/dirty_padding", "frcn/saturated"):
        assert all(bool(torch.isfinite(g).all()) for g in got)


@pytest.mark.parametrize("name", R.names("rpn"))
def test_rpn_loss_against_float64(dev, name):
    """Forward: 256 blocks per image, grid-stride 65,536; backward:
    min(ceil(P / 256), 2048) blocks."""
    ref, got = check_case(dev, name)
    if name == "rpn/saturated":
        assert all(bool(torch.isfinite(g).all()) for g in got)


@pytest.mark.parametrize("name", R.names("mask"))
def test_mask_loss_against_float64(dev, name):
    """One wave per row strides P by 64 at channel stride C; the backward is
    float4 when C % 4 == 0, scalar otherwise, capped at 8192 blocks."""
    ref, got = check_case(dev, name)
    if name in ("mask/dirty_rows", "mask/saturated"):
        assert bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("name", R.names("retina"))
def test_retina_loss_against_float64(dev, name):
    """Forward 512 blocks per image, backward 1024, over float4 class quads;
    the level is looked up per element."""
    ref, got = check_case(dev, name)
    if name == "retina/saturated":
        assert all(bool(torch.isfinite(g).all()) for g in got)


# ------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("name", ["rpn/fwd_stride", "frcn/coco-80", "mask/cap_vec4", "retina/pyramid"])
def test_two_runs_are_bit_identical(dev, name):
    case = reference(name)["case"]
    runs = []
    for _ in range(2):
        leaves, out = run_op(case, dev)
        runs.append((out, backward(leaves, out)))
    (o1, g1), (o2, g2) = runs
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert all(same_bits(a, b) for a, b in zip(g1, g2))


@pytest.mark.parametrize("name", ["frcn/dirty_padding", "mask/dirty_rows"])
def test_dirty_excluded_rows_reach_no_output(dev, name):
    """The excluded rows' NaN, zero-area boxes and class -1 replaced by
    ordinary numbers in the same layout: the kernels skip those rows, so every
    loss and every gradient keeps its bits."""
    case = reference(name)["case"]
    runs = []
    for c in (case, R.cleaned(case)):
        leaves, out = run_op(c, dev)
        runs.append((out, backward(leaves, out)))
    (o1, g1), (o2, g2) = runs
    assert all(bool(torch.isfinite(a)) and torch.equal(a, b) for a, b in zip(o1, o2))
    assert all(bool(torch.isfinite(a).all()) and same_bits(a, b) for a, b in zip(g1, g2))


# ------------------------------------------------- a missing upstream gradient
def _groups(case, n):
    """Which gradient tensors belong to loss 0 / loss 1."""
    if case["kernel"] == "retina":
        return list(range(n // 2)), list(range(n // 2, n))
    return [0], [1]


@pytest.mark.parametrize("name", ["rpn/block_edge", "frcn/ragged_rows", "frcn/coco-1",
                                  "retina/single_level", "retina/tiny_top_level"])
def test_missing_upstream_gradient(dev, name):
    """Only one of the two losses is differentiated: RPN and RetinaNet get a
    null pointer for the other's upstream gradient, Fast R-CNN a zero.  The
    other loss's gradient tensors come back exactly 0, this one's unchanged
    to the bit."""
    case = reference(name)["case"]
    leaves, out = run_op(case, dev)
    full = backward(leaves, out)
    groups = _groups(case, len(full))
    for k in (0, 1):
        leaves, out = run_op(case, dev)
        got = backward(leaves, out, tuple(UP[j] if j == k else None for j in (0, 1)))
        assert any(bool(full[i].any()) for i in groups[k])
        for i in groups[k]:
            assert same_bits(got[i], full[i]), (k, i)
        for i in groups[1 - k]:
            assert not got[i].any() and not bool(torch.isnan(got[i]).any()), (k, i)


@pytest.mark.parametrize("name", [n for n in R.names("rpn") if "weights_beta" in n])
def test_rpn_scale_folds_the_normaliser(dev, name):
    """scale = 1 / 512 (the normaliser folded into the op): a power of two, so
    the scaled sums and every gradient are the unscaled ones times 2^-9 to the
    bit; with the upstream gradient of loc only, and of cls only, the other
    tensor is exactly 0 and this one keeps its bits."""
    s = 1.0 / 512
    case = reference(name)["case"]
    leaves, out = run_op(case, dev)
    full = backward(leaves, out)
    leaves, outs = run_op(case, dev, scale=s)
    fulls = backward(leaves, outs)
    assert all(torch.equal(a, b * s) for a, b in zip(outs, out))
    assert all(same_bits(a, b * s) and a.any() for a, b in zip(fulls, full))
    for k in (0, 1):
        leaves, outs = run_op(case, dev, scale=s)
        got = backward(leaves, outs, tuple(UP[j] if j == k else None for j in (0, 1)))
        assert same_bits(got[k], fulls[k]) and not got[1 - k].any()
