"""Every arm of the conv / multi-level conv / wgrad launch planner
(csrc/conv_plan.h) launched on the GPU and compared with float64.

A case names a shape, a math mode, an epilogue, the operands that are not
16-byte aligned, the tuning knobs it sets, and the ARM it claims: the plan
fields that select a kernel instantiation, a reduce or a masking rule.  The
knobs bring the arms of large shapes down to small ones.

test_case_table_reaches_every_arm needs no GPU: it asks the plan queries (256
CUs without a device) that every case's plan is the arm it claims, and that the
arms of all cases contain REQUIRED_ARMS.  A plan rule that moves a case to
another arm fails there before anything is launched.  The GPU tests repeat the
plan assertion with the launch's real pointers, so a card with another CU count
fails naming the arm it got.

GPU checks per case:
  * exact on integers: x, dy in [-8, 8], w / bias / residual / top-down in
    [-4, 4], the gate in {-1, 0, 1}.  All are bf16 values (the 3-term split is
    h = x, m = l = 0) and every partial sum is an integer of magnitude at most
    32 K + 12 < 2^24 (K = k k Cin forward, N OH OW wgrad): the f32 result is
    exact in any summation order, across split-K slabs and reduces, so the bar
    is torch.equal against float64;
  * the output lies inside a buffer with >= 64 guard floats of NaN on either
    side, which must keep their bits;
  * two runs are bit-equal;
  * random data at the bars of tests/test_gpu_ops.py (forward rtol = atol =
    1e-4; wgrad rtol 1e-4, atol 2e-5 max|want|), the split path's error at most
    4 x the f32 path's + 1e-6 on one shape per family;
  * gated == ungated masked afterwards, streaming == tiled, and an aligned and
    a mis-aligned launch of a stream-eligible K <= 128 shape round alike.
"""
import collections
import contextlib
import functools
import math

import pytest
import torch

F = torch.nn.functional
BIG = 1 << 30
NAN_BITS = 0x7FC00000
GUARD = 64


def ops():
    from detectron2_tensorflow_amd.layers import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (binds the HIP runtime torch ships)
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    return _C.load()


@contextlib.contextmanager
def knobs(kn):
    old = {k: ops().get_tuning(k) for k in kn}
    try:
        for k, v in kn.items():
            ops().set_tuning(k, v)
        yield
    finally:
        for k, v in old.items():
            ops().set_tuning(k, v)


REDUCE = ("none", "scalar", "float4")
FAMILIES = ("tiled128x128", "tiled128x64", "tiled128x32", "ws256x128", "stream1x1")
WGRAD_KERNELS = ("f32", "split", "split_occ3", "ws", "ws_inc")

# ---------------------------------------------------------------- forward
FwdArm = collections.namedtuple(
    "FwdArm", "family lds_epi main_splits main_reduce tail_tiles tail_reduce stream_tn stream_form",
    defaults=(0, 0))
FwdCase = collections.namedtuple("FwdCase", "id shape math epi unaligned knobs arm vs_f32")


def fwd(id, shape, arm, epi=("bias",), math="split", unaligned=(), knobs=None, vs_f32=False):
    """shape: (N, H, W, Cin, Cout, k, stride, (pad_beg, pad_end)); epi: of "bias",
    "relu", "relu_after_add", "residual", "gate", "topdown", "flip"; unaligned: of "y",
    "bias", "residual", "gate", "topdown"."""
    assert set(epi) <= {"bias", "relu", "relu_after_add", "residual", "gate", "topdown", "flip"}
    assert set(unaligned) <= {"y"} | (set(epi) & {"bias", "residual", "gate", "topdown"})
    return FwdCase(id, shape, math, frozenset(epi), frozenset(unaligned), dict(knobs or {}),
                   FwdArm(*arm), vs_f32)


NO_WS = {"conv_ws_mink": BIG}  # keeps the long-K split convs off the warp-specialised kernel
K1_512 = (1, 7, 9, 512, 128, 1, 1, (0, 0))
TAIL_F32 = (1, 97, 127, 256, 1024, 1, 1, (0, 0))
TAIL_SPLIT = (1, 97, 127, 64, 1024, 3, 1, (1, 1))
TAIL_64 = (1, 131, 252, 64, 66, 3, 1, (1, 1))
TAIL_WS = (1, 65, 128, 512, 1024, 1, 1, (0, 0))
FWD_CASES = [
    # tiled 128x128, split products, split-K with the float4 reduce
    fwd("t128-splitk", K1_512, ("tiled128x128", 1, 2, "float4", 0, "none"), knobs=NO_WS, vs_f32=True),
    fwd("t128-splitk-res-relu", K1_512, ("tiled128x128", 1, 2, "float4", 0, "none"),
        epi=("bias", "relu", "relu_after_add", "residual"), knobs=NO_WS),
    fwd("t128-splitk-gate-res", K1_512, ("tiled128x128", 1, 2, "float4", 0, "none"),
        epi=("residual", "gate"), knobs=NO_WS),
    # the same shape, output a view one float into its buffer: 128x64, no LDS epilogue, scalar reduce
    fwd("unal-y-splitk", K1_512, ("tiled128x64", 0, 2, "scalar", 0, "none"), unaligned=("y",),
        knobs=NO_WS),
    fwd("unal-res-gate-splitk", K1_512, ("tiled128x64", 0, 2, "scalar", 0, "none"),
        epi=("bias", "residual", "gate"), unaligned=("residual", "gate")),
    fwd("unal-topdown-splitk", K1_512, ("tiled128x64", 0, 2, "scalar", 0, "none"),
        epi=("bias", "topdown", "relu"), unaligned=("y", "topdown")),
    # only the bias unaligned: the LDS epilogue stays (WS), the float4 reduce is refused
    fwd("unal-bias-ws", K1_512, ("ws256x128", 1, 2, "scalar", 0, "none"), unaligned=("bias",)),
    fwd("unal-bias-t128", K1_512, ("tiled128x128", 1, 2, "scalar", 0, "none"),
        epi=("bias", "residual"), unaligned=("bias",), knobs=NO_WS),
    fwd("ws-splitk", K1_512, ("ws256x128", 1, 2, "float4", 0, "none"), vs_f32=True),
    fwd("ws-onepass", (1, 9, 11, 512, 128, 1, 1, (0, 0)), ("ws256x128", 1, 1, "none", 0, "none"),
        epi=("bias", "relu"), knobs={"conv_split_slots": 1}),
    # one pass without the LDS epilogue
    fwd("unal-y-onepass", (1, 20, 24, 64, 128, 1, 1, (0, 0)), ("tiled128x64", 0, 1, "none", 0, "none"),
        epi=("bias", "relu"), unaligned=("y",)),
    fwd("unal-y-onepass-32", (1, 9, 11, 128, 12, 1, 1, (0, 0)), ("tiled128x32", 0, 1, "none", 0, "none"),
        epi=("bias", "residual"), unaligned=("y", "residual")),
    fwd("cout15-splitk", (1, 7, 11, 512, 15, 1, 1, (0, 0)), ("tiled128x32", 0, 2, "scalar", 0, "none")),
    # tail launches
    fwd("tail-t128-f32", TAIL_F32, ("tiled128x128", 1, 1, "none", 8, "float4"), math="f32"),
    fwd("tail-t128-f32-topdown", TAIL_F32, ("tiled128x128", 1, 1, "none", 8, "float4"), math="f32",
        epi=("bias", "topdown", "relu", "relu_after_add")),
    fwd("tail-t128-split", TAIL_SPLIT, ("tiled128x128", 1, 1, "none", 8, "float4"), knobs=NO_WS),
    fwd("tail-t128-split-gate-res", TAIL_SPLIT, ("tiled128x128", 1, 1, "none", 8, "float4"),
        epi=("residual", "gate", "flip"), knobs=NO_WS),
    fwd("tail-t64-scalar", TAIL_64, ("tiled128x64", 0, 1, "none", 4, "scalar"),
        epi=("bias", "residual", "relu", "relu_after_add")),
    fwd("tail-ws", TAIL_WS, ("ws256x128", 1, 1, "none", 8, "float4"), epi=("bias", "relu")),
    # kernel sizes, pads
    fwd("k5-ws", (1, 11, 13, 64, 96, 5, 1, (2, 2)), ("ws256x128", 1, 6, "float4", 0, "none")),
    fwd("k7-t128", (1, 11, 13, 64, 160, 7, 1, (3, 3)), ("tiled128x128", 1, 11, "float4", 0, "none"),
        epi=("bias", "flip")),
    fwd("asym-pad-s2", (1, 12, 14, 64, 96, 3, 2, (0, 1)), ("ws256x128", 1, 2, "float4", 0, "none")),
    fwd("asym-pad-s2-t128", (1, 12, 14, 64, 96, 3, 2, (0, 1)), ("tiled128x128", 1, 2, "float4", 0, "none"),
        math="f32"),
    # ragged K (Cin % 32 != 0)
    fwd("raggedk-ws", (1, 9, 11, 520, 128, 1, 1, (0, 0)), ("ws256x128", 1, 2, "float4", 0, "none")),
    fwd("raggedk-ws-k3", (1, 9, 11, 72, 128, 3, 1, (1, 1)), ("ws256x128", 1, 3, "float4", 0, "none")),
    fwd("raggedk-t128", (1, 9, 11, 72, 128, 3, 1, (1, 1)), ("tiled128x128", 1, 3, "float4", 0, "none"),
        knobs=NO_WS),
    fwd("raggedk-t128-f32", (1, 9, 11, 72, 128, 3, 1, (1, 1)), ("tiled128x128", 1, 3, "float4", 0, "none"),
        math="f32"),
    fwd("raggedk-t64", (1, 9, 11, 36, 64, 3, 1, (1, 1)), ("tiled128x64", 1, 2, "float4", 0, "none"),
        vs_f32=True),
    fwd("raggedk-t32", (1, 9, 11, 36, 12, 3, 1, (1, 1)), ("tiled128x32", 1, 2, "float4", 0, "none"),
        vs_f32=True),
    # M % BM == 0
    fwd("m-exact-t128", (1, 16, 16, 64, 128, 1, 1, (0, 0)), ("tiled128x128", 1, 1, "none", 0, "none"),
        epi=("bias", "relu")),
    fwd("m-exact-t128-f32", (1, 16, 16, 64, 128, 1, 1, (0, 0)), ("tiled128x128", 1, 1, "none", 0, "none"),
        math="f32"),
    fwd("m-exact-ws", (1, 16, 16, 512, 128, 1, 1, (0, 0)), ("ws256x128", 1, 2, "float4", 0, "none")),
    # the top-down epilogue on the three tiled families
    fwd("topdown-t128", (1, 9, 11, 64, 160, 1, 1, (0, 0)), ("tiled128x128", 1, 1, "none", 0, "none"),
        epi=("bias", "topdown")),
    fwd("topdown-t128-splitk", (1, 9, 11, 64, 160, 3, 1, (1, 1)), ("tiled128x128", 1, 2, "float4", 0, "none"),
        epi=("bias", "topdown", "relu", "relu_after_add"), knobs=NO_WS),
    fwd("topdown-t64", (1, 9, 11, 64, 64, 3, 1, (1, 1)), ("tiled128x64", 1, 2, "float4", 0, "none"),
        epi=("bias", "topdown")),
    fwd("topdown-t64-onepass", (1, 9, 11, 64, 64, 1, 1, (0, 0)), ("tiled128x64", 1, 1, "none", 0, "none"),
        epi=("bias", "topdown", "relu")),
    fwd("topdown-t32", (1, 9, 11, 36, 12, 3, 1, (1, 1)), ("tiled128x32", 1, 2, "float4", 0, "none"),
        epi=("bias", "topdown")),
    fwd("topdown-t32-onepass", (1, 9, 11, 128, 12, 1, 1, (0, 0)), ("tiled128x32", 1, 1, "none", 0, "none"),
        epi=("bias", "topdown")),
    # streaming 1x1
    fwd("stream-tn2-few", (1, 8, 8, 64, 128, 1, 1, (0, 0)), ("stream1x1", 1, 1, "none", 0, "none", 2, 0),
        knobs={"conv_stream": 1}, vs_f32=True),
    fwd("stream-tn2-res-gate", (1, 9, 9, 128, 132, 1, 1, (0, 0)),
        ("stream1x1", 1, 1, "none", 0, "none", 2, 3), epi=("bias", "residual", "gate"),
        knobs={"conv_stream": 1}),
    fwd("stream-k256-forced", (1, 9, 9, 256, 68, 1, 1, (0, 0)), ("stream1x1", 1, 1, "none", 0, "none", 2, 1),
        epi=("bias", "residual", "relu", "relu_after_add"), knobs={"conv_stream": -1}),
    fwd("stream-k256-gate", (1, 9, 9, 256, 68, 1, 1, (0, 0)), ("stream1x1", 1, 1, "none", 0, "none", 2, 2),
        epi=("gate",), knobs={"conv_stream": -1}),
    fwd("stream-tn4", (1, 63, 65, 64, 2052, 1, 1, (0, 0)), ("stream1x1", 1, 1, "none", 0, "none", 4, 0),
        knobs={"conv_stream": 1}),
    fwd("stream-tn4-res", (1, 63, 65, 64, 2052, 1, 1, (0, 0)), ("stream1x1", 1, 1, "none", 0, "none", 4, 1),
        epi=("bias", "residual", "relu", "relu_after_add"), knobs={"conv_stream": 1}),
    # the stream-eligible shapes with an unaligned output: the tiled kernel, one pass
    fwd("unal-y-stream-shape", (1, 9, 9, 128, 132, 1, 1, (0, 0)), ("tiled128x64", 0, 1, "none", 0, "none"),
        epi=("bias", "residual"), unaligned=("y",), knobs={"conv_stream": 1}),
]


def fwd_dims(c):
    N, H, W, Cin, Cout, k, s, (pb, pe) = c.shape
    return N, (H + pb + pe - k) // s + 1, (W + pb + pe - k) // s + 1, Cout


def fwd_operands(c):
    o = ops()
    m = o.OP_WORKSPACE | o.OP_WS_ALIGNED
    m |= o.OP_TOPDOWN if "topdown" in c.epi else 0
    m |= o.OP_RESIDUAL if "residual" in c.epi else 0
    m |= o.OP_GATE if "gate" in c.epi else 0
    m |= 0 if c.unaligned & {"y", "residual", "gate", "topdown"} else o.OP_ALIGNED
    m |= 0 if "bias" in c.unaligned else o.OP_BIAS_ALIGNED
    return m


def fwd_arm_of(c, operands):
    """The arm the planner gives the case (knobs applied by the caller)."""
    N, H, W, Cin, Cout, k, s, pad = c.shape
    p = ops().conv_plan(N, H, W, Cin, Cout, k, s, pad, flags=4 if c.math == "split" else 0,
                        operands=operands)
    return FwdArm(FAMILIES[p["family"]], p["lds_epi"], p["main_splits"], REDUCE[p["main_reduce"]],
                  p["tail_tiles"], REDUCE[p["tail_reduce"]], p["stream_tn"], p["stream_form"])


def fwd_tags(c):
    """The arms a forward case stands for, from its claim and its shape."""
    N, H, W, Cin, Cout, k, s, (pb, pe) = c.shape
    a = c.arm
    M = math.prod(fwd_dims(c)[:3])
    if a.family == "stream1x1":
        tags = [f"stream1x1 tn{a.stream_tn} form{a.stream_form} k{Cin}"]
        if Cout % (32 * a.stream_tn):
            tags.append(f"stream1x1 tn{a.stream_tn} ragged slice")
        return tags
    launch = "one pass" if a.main_splits == 1 else f"split-K {a.main_reduce}"
    if a.tail_tiles:
        launch += f" + tail {a.tail_reduce}"
    fam = f"{a.family} {c.math}"
    tags = [f"{fam} {launch}" + ("" if a.lds_epi else " no-lds-epi")]
    if Cin % 32:
        tags.append(f"{fam} ragged K")
    if M % (256 if a.family == "ws256x128" else 128) == 0:
        tags.append(f"{fam} M % BM == 0")
    if pb != pe:
        tags.append(f"{fam} pad_beg != pad_end")
    if k > 3:
        tags.append(f"{fam} {k}x{k}")
    if "topdown" in c.epi:
        tags.append(f"{a.family} top-down" + (" in the reduce" if a.main_splits > 1 or a.tail_tiles else ""))
    if "bias" in c.unaligned:
        tags.append(f"{a.family} unaligned bias")
    if not a.lds_epi and Cout % 4 == 0:
        tags.append("unaligned output, Cout % 4 == 0")
    return tags


# ---------------------------------------------------------------- wgrad
WgradArm = collections.namedtuple("WgradArm", "kernel TM TN splits reduce")
WgradCase = collections.namedtuple("WgradCase", "id shape math accumulate unaligned knobs arm")


def wg(id, shape, arm, math="split", accumulate=False, unaligned=False, knobs=None):
    """shape: (N, H, W, Cin, Cout, k, stride); same-size pads.  accumulate: the
    gradient is added into a guarded (dw, db); unaligned: that dw is a view
    one float into its buffer."""
    assert accumulate or not unaligned
    return WgradCase(id, shape, math, accumulate, unaligned, dict(knobs or {}), WgradArm(*arm))


MINCH1 = {"wgrad_minch": 1}
WGRAD_CASES = [
    # the incremental-cursor rule at its boundary: OW >= 4 and 32 / OW + 1 <= OH
    wg("ws-inc-min", (1, 9, 4, 256, 128, 3, 1), ("ws_inc", 2, 2, 1, "none")),
    wg("ws-oh-short", (1, 8, 4, 256, 128, 3, 1), ("ws", 2, 2, 1, "none")),
    wg("ws-ow3", (2, 9, 3, 256, 128, 3, 1), ("ws", 2, 2, 1, "none")),
    wg("ws-inc-wrap", (3, 9, 4, 256, 128, 3, 1), ("ws_inc", 2, 2, 1, "none")),
    wg("ws-inc-min-split", (1, 9, 4, 256, 128, 3, 1), ("ws_inc", 2, 2, 2, "float4"), knobs=MINCH1),
    wg("ws-ow3-split", (2, 9, 3, 256, 128, 3, 1), ("ws", 2, 2, 2, "float4"), knobs=MINCH1),
    wg("ws-inc-wrap-split", (3, 9, 4, 256, 128, 3, 1), ("ws_inc", 2, 2, 4, "float4"), knobs=MINCH1),
    wg("ws-inc-wrap-maxsplit", (3, 9, 4, 256, 128, 3, 1), ("ws_inc", 2, 2, 2, "float4"),
       knobs={"wgrad_minch": 1, "wgrad_maxsplit": 2}),
    wg("ws-inc-wrap-accum-unal", (3, 9, 4, 256, 128, 3, 1), ("ws_inc", 2, 2, 4, "scalar"),
       accumulate=True, unaligned=True, knobs=MINCH1),
    wg("ws-s2", (1, 17, 21, 256, 128, 3, 2), ("ws", 2, 2, 4, "float4"), knobs=MINCH1),
    # 128x128 split kernel at three workgroups per CU
    wg("occ3", (2, 9, 11, 128, 192, 3, 1), ("split_occ3", 2, 2, 1, "none"),
       knobs={"wgrad_occ3_min_p": 64}),
    wg("occ3-split", (2, 9, 11, 128, 192, 3, 1), ("split_occ3", 2, 2, 7, "float4"),
       knobs={"wgrad_occ3_min_p": 64, "wgrad_minch": 1}),
    wg("occ3-accum", (2, 9, 11, 128, 192, 3, 1), ("split_occ3", 2, 2, 3, "float4"), accumulate=True,
       knobs={"wgrad_occ3_min_p": 64, "wgrad_minch": 1, "wgrad_slots": 54}),
    # the split kernel's four tile forms, more than one split
    wg("split11", (2, 9, 11, 36, 20, 3, 1), ("split", 1, 1, 7, "float4"), knobs=MINCH1),
    wg("split11-accum-unal", (2, 9, 11, 36, 20, 3, 1), ("split", 1, 1, 7, "scalar"), accumulate=True,
       unaligned=True, knobs=MINCH1),
    wg("split11-accum-unal-1", (2, 9, 11, 36, 20, 3, 1), ("split", 1, 1, 1, "scalar"), accumulate=True,
       unaligned=True),
    wg("split21", (2, 9, 11, 128, 64, 3, 1), ("split", 2, 1, 7, "float4"), knobs=MINCH1),
    wg("split12-s2", (2, 9, 11, 64, 128, 3, 2), ("split", 1, 2, 2, "float4"), knobs=MINCH1),
    wg("split22", (2, 9, 11, 128, 128, 3, 1), ("split", 2, 2, 1, "none")),
    # the f32 kernel
    wg("f32-11", (2, 9, 11, 64, 64, 1, 1), ("f32", 1, 1, 7, "float4"), math="f32", knobs=MINCH1),
    wg("f32-22-accum-unal", (2, 9, 11, 128, 132, 3, 1), ("f32", 2, 2, 7, "scalar"), math="f32",
       accumulate=True, unaligned=True, knobs=MINCH1),
    wg("f32-21", (2, 9, 11, 72, 20, 3, 1), ("f32", 2, 1, 1, "none"), math="f32"),
]


def wg_geom(c):
    N, H, W, Cin, Cout, k, s = c.shape
    p = (k - 1) // 2
    return N, H, W, Cin, Cout, k, s, p, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def wg_arm_of(c, aligned):
    N, H, W, Cin, Cout, k, s, p, OH, OW = wg_geom(c)
    o = ops()
    from detectron2_tensorflow_amd import _C
    wsb = _C.lib().d2mi_conv2d_wgrad_workspace_size(N, H, W, Cin, Cout, k, k, s, p, p)
    if c.accumulate:  # (as conv2d_wgrad: the reduce adds, one slab at least)
        wsb = max(wsb, (k * k * Cin * Cout + Cout) * 4)
    operands = o.OP_WS_ALIGNED | (o.OP_WORKSPACE if wsb else 0) | (o.OP_ALIGNED if aligned else 0)
    pl = o.wgrad_plan(N, H, W, Cin, Cout, k, s, (p, p),
                      flags=(4 if c.math == "split" else 0) | (8 if c.accumulate else 0),
                      operands=operands, workspace_bytes=wsb)
    return WgradArm(WGRAD_KERNELS[pl["kernel"]], pl["TM"], pl["TN"], pl["splits"], REDUCE[pl["reduce"]])


def wg_tags(c):
    a = c.arm
    N, H, W, Cin, Cout, k, s, p, OH, OW = wg_geom(c)
    kern = a.kernel if a.kernel.startswith("ws") or a.kernel == "split_occ3" else f"{a.kernel}<{a.TM},{a.TN}>"
    tags = [f"wgrad {kern} " + ("one split" if a.splits == 1 else "splits") + f" reduce {a.reduce}"]
    # the incremental-cursor rule (OW >= 4, 32 / OW + 1 <= OH), met or missed by one
    if a.kernel == "ws_inc" and OW == 4 and 32 // OW + 1 == OH:
        tags.append("wgrad ws_inc at the cursor rule's edge")
    if a.kernel == "ws_inc" and N > 1:
        tags.append("wgrad ws_inc across image wraps")
    if a.kernel == "ws" and s == 1 and (OW == 3 or (OW >= 4 and 32 // OW + 1 == OH + 1)):
        tags.append("wgrad ws at the cursor rule's edge")
    return tags


# ---------------------------------------------------------------- multi-level
LevelsArm = collections.namedtuple("LevelsArm", "family lds_epi splits")
LevelsCase = collections.namedtuple("LevelsCase", "id dims Cin Cout k math arm")
LEVELS_CASES = [
    LevelsCase("lv3-t128-splitk", ((1, 9, 11), (1, 5, 6), (1, 3, 3)), 64, 256, 3, "split",
               LevelsArm("tiled128x128", 1, 2)),
    LevelsCase("lv3-t128-splitk-f32", ((1, 9, 11), (1, 5, 6), (1, 3, 3)), 64, 256, 3, "f32",
               LevelsArm("tiled128x128", 1, 2)),
    LevelsCase("lv2-t32-splitk", ((1, 9, 11), (1, 5, 6)), 64, 12, 3, "split",
               LevelsArm("tiled128x32", 1, 2)),
    LevelsCase("lv2-mixed-n-1x1", ((1, 9, 11), (2, 5, 6)), 256, 80, 1, "split",
               LevelsArm("tiled128x128", 1, 1)),
    LevelsCase("lv2-t64-ragged-k", ((2, 5, 6), (1, 9, 11)), 36, 64, 3, "split",
               LevelsArm("tiled128x64", 1, 2)),
    LevelsCase("lv1-cout15", ((1, 9, 11),), 64, 15, 3, "split", LevelsArm("tiled128x32", 0, 1)),
]


def levels_arm_of(c):
    pad = ((c.k - 1) // 2,) * 2
    p = ops().conv_levels_plan(c.dims, c.Cin, c.Cout, c.k, 1, pad, flags=4 if c.math == "split" else 0)
    return LevelsArm(FAMILIES[p["family"]], p["lds_epi"], p["splits"])


def levels_tags(c):
    a = c.arm
    tags = [f"levels {a.family} {c.math} " + ("one pass" if a.splits == 1 else "split-K")
            + ("" if a.lds_epi else " no-lds-epi")]
    if len({d[0] for d in c.dims}) > 1:
        tags.append("levels with different N")
    if (c.k, c.Cin) != (3, 256):
        tags.append(f"levels {c.k}x{c.k} over Cin {c.Cin}")
    return tags


# The arms the table must reach: the planner arms that tests/test_gpu_ops.py
# does not launch, then those it does (so that this module alone runs them all).
REQUIRED_ARMS = [
    # forward tiled 128x128 with split products and split-K
    "tiled128x128 split split-K float4",
    # forward tiled 128x128 with a tail launch, f32 or split math
    "tiled128x128 f32 one pass + tail float4",
    "tiled128x128 split one pass + tail float4",
    # tail launch with the scalar reduce, tail of the 128x64 family
    "tiled128x64 split one pass + tail scalar no-lds-epi",
    # output / residual / gate / top-down not 16-byte aligned with Cout % 4 == 0
    "unaligned output, Cout % 4 == 0",
    "tiled128x64 split split-K scalar no-lds-epi",
    "tiled128x64 split one pass no-lds-epi",
    "tiled128x32 split one pass no-lds-epi",
    # unaligned bias: float4 reduce refused, LDS epilogue kept
    "ws256x128 unaligned bias",
    "tiled128x128 unaligned bias",
    "ws256x128 split split-K scalar",
    "tiled128x128 split split-K scalar",
    # ragged K on the 128x128, WS and 128x32 kernels
    "tiled128x128 split ragged K",
    "tiled128x128 f32 ragged K",
    "ws256x128 split ragged K",
    "tiled128x32 split ragged K",
    # M % BM == 0
    "tiled128x128 split M % BM == 0",
    "tiled128x128 f32 M % BM == 0",
    "ws256x128 split M % BM == 0",
    # pad_beg != pad_end
    "ws256x128 split pad_beg != pad_end",
    "tiled128x128 f32 pad_beg != pad_end",
    # 5x5 (WS) and 7x7 (kept off WS)
    "ws256x128 split 5x5",
    "tiled128x128 split 7x7",
    # top-down on the families but WS
    "tiled128x128 top-down",
    "tiled128x128 top-down in the reduce",
    "tiled128x64 top-down",
    "tiled128x64 top-down in the reduce",
    "tiled128x32 top-down",
    "tiled128x32 top-down in the reduce",
    # streaming 1x1: TN 2 by the few-strips rule; ragged slice with residual and gate; K = 256 forced
    "stream1x1 tn2 form0 k64",
    "stream1x1 tn2 form3 k128",
    "stream1x1 tn2 ragged slice",
    "stream1x1 tn2 form1 k256",
    "stream1x1 tn2 form2 k256",
    # wgrad split_occ3
    "wgrad split_occ3 one split reduce none",
    "wgrad split_occ3 splits reduce float4",
    # wgrad ws versus ws_inc at the boundary of the incremental-cursor rule
    "wgrad ws_inc at the cursor rule's edge",
    "wgrad ws at the cursor rule's edge",
    "wgrad ws_inc across image wraps",
    "wgrad ws_inc splits reduce float4",
    "wgrad ws splits reduce float4",
    # wgrad scalar reduce, and the f32 / split <1,1> kernels with more than one split
    "wgrad ws_inc splits reduce scalar",
    "wgrad split<1,1> splits reduce scalar",
    "wgrad split<1,1> one split reduce scalar",
    "wgrad f32<2,2> splits reduce scalar",
    "wgrad split<1,1> splits reduce float4",
    "wgrad f32<1,1> splits reduce float4",
    # multi-level conv: 128x32 with split-K, levels with different N, other than 3x3 over 256
    "levels tiled128x32 split split-K",
    "levels with different N",
    "levels 3x3 over Cin 64",
    "levels 1x1 over Cin 256",
    "levels tiled128x128 split split-K",
    "levels tiled128x128 f32 split-K",
    "levels tiled128x64 split split-K",
    "levels tiled128x32 split one pass no-lds-epi",
    # ---- reached by tests/test_gpu_ops.py as well
    "ws256x128 split split-K float4",
    "ws256x128 split one pass",
    "ws256x128 split one pass + tail float4",
    "tiled128x128 split one pass",
    "tiled128x128 f32 one pass",
    "tiled128x128 f32 split-K float4",
    "tiled128x64 split split-K float4",
    "tiled128x64 split one pass",
    "tiled128x64 split ragged K",
    "tiled128x32 split split-K float4",
    "tiled128x32 split one pass",
    "tiled128x32 split split-K scalar no-lds-epi",
    "stream1x1 tn4 form0 k64",
    "stream1x1 tn4 form1 k64",
    "stream1x1 tn4 ragged slice",
    "wgrad ws_inc one split reduce none",
    "wgrad ws one split reduce none",
    "wgrad split<2,2> one split reduce none",
    "wgrad split<2,1> splits reduce float4",
    "wgrad split<1,2> splits reduce float4",
    "wgrad f32<2,1> one split reduce none",
]


def test_case_table_reaches_every_arm(lib):
    """No GPU: the plan of every case (256 CUs) is the arm it claims, and the
    claimed arms contain REQUIRED_ARMS."""
    ids = [c.id for c in FWD_CASES + WGRAD_CASES + LEVELS_CASES]
    assert len(ids) == len(set(ids))
    reached = set()
    for c in FWD_CASES:
        with knobs(c.knobs):
            got = fwd_arm_of(c, fwd_operands(c))
        assert got == c.arm, (c.id, got)
        reached.update(fwd_tags(c))
    for c in WGRAD_CASES:
        with knobs(c.knobs):
            got = wg_arm_of(c, not c.unaligned)
        assert got == c.arm, (c.id, got)
        reached.update(wg_tags(c))
    for c in LEVELS_CASES:
        got = levels_arm_of(c)
        assert got == c.arm, (c.id, got)
        reached.update(levels_tags(c))
    missing = [a for a in REQUIRED_ARMS if a not in reached]
    assert not missing, missing
    assert len(set(REQUIRED_ARMS)) == len(REQUIRED_ARMS)


# ---------------------------------------------------------------- GPU helpers
def guarded(n, dev, unaligned):
    """(buf, view): n floats with >= GUARD NaN floats on either side; the view
    starts 16-byte aligned, or one float past that."""
    off = GUARD + (1 if unaligned else 0)
    buf = torch.full((n + 2 * GUARD + 1,), float("nan"), dtype=torch.float32, device=dev)
    v = buf[off:off + n]
    assert (v.data_ptr() % 16 != 0) == bool(unaligned)
    return buf, v


def assert_guards_intact(buf, view, what):
    bits = buf.view(torch.int32)
    off = (view.data_ptr() - buf.data_ptr()) // 4
    lo, hi = bits[:off], bits[off + view.numel():]
    assert lo.numel() >= GUARD and hi.numel() >= GUARD
    assert bool((lo == NAN_BITS).all()) and bool((hi == NAN_BITS).all()), f"{what}: wrote outside its output"


def put(t, dev, unaligned=False):
    """t on the device; unaligned: as a contiguous view one float into a buffer."""
    if t is None:
        return None
    if not unaligned:
        d = t.to(dev)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def first_diff(got, want):
    d = (got != want).nonzero()
    i = tuple(d[0].tolist())
    return f"{d.shape[0]} differ, first at {i}: got {float(got[i])} want {float(want[i])}"


def draw(g, shape, kind, lo_hi=4, scale=1.0):
    if kind == "int":
        return torch.randint(-lo_hi, lo_hi + 1, shape, generator=g).float()
    return torch.randn(shape, generator=g) * scale


@functools.lru_cache(maxsize=2)
def fwd_data(shape, kind):
    """Operands of a forward shape (integers, or randn with w / sqrt(K)) and its
    float64 convolution, plain and with flipped taps: shared by the shape's cases."""
    N, H, W, Cin, Cout, k, s, (pb, pe) = shape
    g = torch.Generator().manual_seed(1000 + sum(shape[:7]) + (kind == "int"))
    OH, OW = (H + pb + pe - k) // s + 1, (W + pb + pe - k) // s + 1
    d = {"x": draw(g, (N, H, W, Cin), kind, 8),
         "w": draw(g, (k, k, Cin, Cout), kind, 4, 1 / math.sqrt(k * k * Cin)),
         "bias": draw(g, (Cout,), kind), "residual": draw(g, (N, OH, OW, Cout), kind),
         "topdown": draw(g, (N, (OH + 1) // 2, (OW + 1) // 2, Cout), kind)}
    gate = torch.randint(-1, 2, (N, OH, OW, Cout), generator=g).float()
    d["gate"] = gate if kind == "int" else torch.relu(gate * torch.rand(gate.shape, generator=g))
    d["conv"] = {}
    return d


def fwd_conv64(d, shape, flip):
    if flip not in d["conv"]:
        k, s, (pb, pe) = shape[5:]
        x = F.pad(d["x"].double().permute(0, 3, 1, 2), (pb, pe, pb, pe))
        w = d["w"].flip(0, 1) if flip else d["w"]
        d["conv"][flip] = F.conv2d(x, w.double().permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
    return d["conv"][flip]


def fwd_want(c, d):
    N, OH, OW, Cout = fwd_dims(c)
    r = fwd_conv64(d, c.shape, "flip" in c.epi)
    if "bias" in c.epi:
        r = r + d["bias"].double()
    after = "relu_after_add" in c.epi
    if "relu" in c.epi and not after:
        r = r.clamp_min(0)
    if "topdown" in c.epi:
        r = r + d["topdown"].double().repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :OH, :OW]
    if "residual" in c.epi:
        r = r + d["residual"].double()
    if "relu" in c.epi and after:
        r = r.clamp_min(0)
    if "gate" in c.epi:
        r = torch.where(d["gate"] > 0, r, torch.zeros_like(r))
    return r


class FwdLaunch:
    """The device operands of a forward case, and its launches into guarded outputs."""

    def __init__(self, c, d, dev):
        self.c, self.dev = c, dev
        self.x = put(d["x"], dev)
        self.wp = ops().pack_conv_weights(d["w"].to(dev))
        self.t = {n: put(d[n], dev, n in c.unaligned) if n in c.epi else None
                  for n in ("bias", "residual", "gate", "topdown")}

    def operands(self, y):
        o = ops()
        al = all(p is None or p.data_ptr() % 16 == 0
                 for p in (y, self.t["residual"], self.t["gate"], self.t["topdown"]))
        b = self.t["bias"]
        m = o.OP_WORKSPACE | o.OP_WS_ALIGNED | (o.OP_ALIGNED if al else 0)
        m |= o.OP_BIAS_ALIGNED if b is None or b.data_ptr() % 16 == 0 else 0
        m |= o.OP_TOPDOWN if self.t["topdown"] is not None else 0
        m |= o.OP_RESIDUAL if self.t["residual"] is not None else 0
        m |= o.OP_GATE if self.t["gate"] is not None else 0
        return m

    def run(self, math_mode=None, gate=True, check_arm=True):
        """One launch (the case's knobs set by the caller); returns the output,
        its guards checked."""
        c = self.c
        N, OH, OW, Cout = fwd_dims(c)
        buf, v = guarded(N * OH * OW * Cout, self.dev, "y" in c.unaligned)
        y = v.view(N, OH, OW, Cout)
        if check_arm:
            got = fwd_arm_of(c, self.operands(y))
            assert got == c.arm, f"{c.id}: this device plans {got}, the case claims {c.arm}"
        _, _, _, _, _, k, s, pad = c.shape
        out = ops().conv2d_nhwc(self.x, self.wp, self.t["bias"], s, pad, relu="relu" in c.epi,
                                topdown=self.t["topdown"], residual=self.t["residual"],
                                relu_after_add="relu_after_add" in c.epi,
                                math_mode=math_mode or c.math, flip_taps="flip" in c.epi,
                                relu_gate=self.t["gate"] if gate else None, out=y)
        assert out.data_ptr() == y.data_ptr()
        assert_guards_intact(buf, v, c.id)
        return y


FWD_IDS = [c.id for c in FWD_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("c", FWD_CASES, ids=FWD_IDS)
def test_forward_arm_is_exact_on_integers(dev, c):
    """The case's arm (asserted from the launch's own pointers) on integer
    operands: torch.equal to float64, guards intact, two runs bit-equal."""
    N, H, W, Cin, Cout, k, s, pad = c.shape
    assert 32 * k * k * Cin + 12 < 2 ** 24
    d = fwd_data(c.shape, "int")
    want = fwd_want(c, d)
    with knobs(c.knobs):
        L = FwdLaunch(c, d, dev)
        y = L.run()
        y2 = L.run()
    assert torch.equal(y, y2), c.id
    got = y.cpu().double()
    assert torch.equal(got, want), f"{c.id} {c.arm}: {first_diff(got, want)}"


@pytest.mark.gpu
@pytest.mark.parametrize("c", FWD_CASES, ids=FWD_IDS)
def test_forward_arm_random_data(dev, c):
    """randn operands, w / sqrt(K): 1e-4 of float64; gated == ungated masked
    afterwards; streaming == tiled; the split error <= 4 x the f32 path's + 1e-6."""
    d = fwd_data(c.shape, "rand")
    want = fwd_want(c, d)
    with knobs(c.knobs):
        L = FwdLaunch(c, d, dev)
        y = L.run()
        assert torch.equal(y, L.run()), c.id
        if "gate" in c.epi:  # gated == the ungated result masked afterwards
            plain = L.run(gate=False, check_arm=False)
            assert torch.equal(y, torch.where(L.t["gate"] > 0, plain, torch.zeros_like(plain))), c.id
        yf = L.run(math_mode="f32", check_arm=False) if c.vs_f32 else None
    got = y.cpu().double()
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4, msg=lambda m: f"{c.id} {c.arm}: {m}")
    if c.arm.family == "stream1x1":  # streaming == tiled for the same launch
        with knobs({"conv_stream": 0}):
            tiled = L.run(check_arm=False)
        assert torch.equal(y, tiled), f"{c.id}: {first_diff(y.cpu(), tiled.cpu())}"
    if c.vs_f32:
        es, ef = float((got - want).abs().max()), float((yf.cpu().double() - want).abs().max())
        assert es <= 4 * ef + 1e-6, (c.id, es, ef)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,epi", [
    ((1, 9, 9, 128, 132, 1, 1, (0, 0)), ("bias", "residual")),
    ((1, 20, 24, 64, 128, 1, 1, (0, 0)), ("bias", "relu")),
    ((1, 11, 13, 64, 96, 1, 1, (0, 0)), ("residual", "gate")),
])
def test_aligned_and_unaligned_launch_of_a_stream_shape_round_alike(dev, shape, epi):
    """plan_conv: a launch the streaming kernel cannot take because an operand
    is not 16-byte aligned sums K in the streaming kernel's order -- for
    K <= 128 the tiled plan has neither split-K nor a tail split."""
    al = fwd("al", shape, ("stream1x1", 1, 1, "none", 0, "none", 2, ("residual" in epi) + 2 * ("gate" in epi)),
             epi=epi)
    un = fwd("un", shape, ("tiled128x64", 0, 1, "none", 0, "none"), epi=epi, unaligned=("y",))
    d = fwd_data(shape, "rand")
    with knobs({"conv_stream": 1}):
        ya = FwdLaunch(al, d, dev).run()
        yu = FwdLaunch(un, d, dev).run()
    assert torch.equal(ya, yu), first_diff(ya.cpu(), yu.cpu())
    torch.testing.assert_close(ya.cpu().double(), fwd_want(al, d), rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------- wgrad on the GPU
@functools.lru_cache(maxsize=4)
def wg_data(shape, kind):
    N, H, W, Cin, Cout, k, s = shape
    p = (k - 1) // 2
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(2000 + sum(shape) + (kind == "int"))
    d = {"x": draw(g, (N, H, W, Cin), kind, 8), "dy": draw(g, (N, OH, OW, Cout), kind, 8),
         "dw0": draw(g, (k, k, Cin, Cout), kind), "db0": draw(g, (Cout,), kind)}
    d["dw"] = torch.nn.grad.conv2d_weight(d["x"].double().permute(0, 3, 1, 2), (Cout, Cin, k, k),
                                          d["dy"].double().permute(0, 3, 1, 2), s, p).permute(2, 3, 1, 0)
    d["db"] = d["dy"].double().sum((0, 1, 2))
    return d


def wg_run(c, d, dev):
    """One launch of a wgrad case (knobs set by the caller): (dw, db)."""
    N, H, W, Cin, Cout, k, s, p, OH, OW = wg_geom(c)
    x, dy = put(d["x"], dev), put(d["dy"], dev)
    kw = dict(with_bias=True, math_mode=c.math)
    if not c.accumulate:
        assert wg_arm_of(c, True) == c.arm, f"{c.id}: this device plans {wg_arm_of(c, True)}"
        return ops().conv2d_wgrad(x, dy, k, s, (p, p), **kw)
    wbuf, wv = guarded(k * k * Cin * Cout, dev, c.unaligned)
    bbuf, bv = guarded(Cout, dev, False)
    dw, db = wv.view(k, k, Cin, Cout), bv
    dw.copy_(d["dw0"])
    db.copy_(d["db0"])
    got = wg_arm_of(c, dw.data_ptr() % 16 == 0)
    assert got == c.arm, f"{c.id}: this device plans {got}, the case claims {c.arm}"
    out = ops().conv2d_wgrad(x, dy, k, s, (p, p), accumulate_into=(dw, db), **kw)
    assert out[0].data_ptr() == dw.data_ptr() and out[1].data_ptr() == db.data_ptr()
    assert_guards_intact(wbuf, wv, c.id + " dw")
    assert_guards_intact(bbuf, bv, c.id + " db")
    return dw, db


def wg_want(c, d):
    if c.accumulate:
        return d["dw0"].double() + d["dw"], d["db0"].double() + d["db"]
    return d["dw"], d["db"]


WG_IDS = [c.id for c in WGRAD_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("c", WGRAD_CASES, ids=WG_IDS)
def test_wgrad_arm_is_exact_on_integers(dev, c):
    """dw and db of the case's arm on integer operands: torch.equal to float64
    (an accumulating case: onto non-zero integer contents, inside guards)."""
    N, H, W, Cin, Cout, k, s, p, OH, OW = wg_geom(c)
    assert 32 * N * OH * OW + 12 < 2 ** 24
    d = wg_data(c.shape, "int")
    want_w, want_b = wg_want(c, d)
    with knobs(c.knobs):
        dw, db = wg_run(c, d, dev)
        dw2, db2 = wg_run(c, d, dev)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), c.id
    gw, gb = dw.cpu().double(), db.cpu().double()
    assert torch.equal(gw, want_w), f"{c.id} {c.arm} dw: {first_diff(gw, want_w)}"
    assert torch.equal(gb, want_b), f"{c.id} {c.arm} db: {first_diff(gb, want_b)}"


@pytest.mark.gpu
@pytest.mark.parametrize("c", WGRAD_CASES, ids=WG_IDS)
def test_wgrad_arm_random_data(dev, c):
    """randn operands at the bar of test_conv2d_wgrad_kernel_with_bias; two runs bit-equal."""
    d = wg_data(c.shape, "rand")
    want_w, want_b = wg_want(c, d)
    with knobs(c.knobs):
        dw, db = wg_run(c, d, dev)
        dw2, db2 = wg_run(c, d, dev)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), c.id
    scale = float(want_w.abs().max())
    torch.testing.assert_close(dw.cpu().double(), want_w, rtol=1e-4, atol=2e-5 * scale,
                               msg=lambda m: f"{c.id} {c.arm}: {m}")
    torch.testing.assert_close(db.cpu().double(), want_b, rtol=1e-4, atol=1e-3)


# ---------------------------------------------------------------- multi-level on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("c", LEVELS_CASES, ids=[c.id for c in LEVELS_CASES])
def test_levels_arm_every_level_matches_float64(dev, c, kind):
    """conv2d_nhwc_levels: every level against float64 (exact on integers,
    1e-4 on random data), with and without the ReLU, two runs bit-equal."""
    assert 32 * c.k * c.k * c.Cin + 12 < 2 ** 24
    assert levels_arm_of(c) == c.arm, f"{c.id}: this device plans {levels_arm_of(c)}"
    g = torch.Generator().manual_seed(3000 + c.Cin + c.Cout + (kind == "int"))
    p = (c.k - 1) // 2
    xs = [draw(g, (n, h, w, c.Cin), kind, 8) for n, h, w in c.dims]
    w = draw(g, (c.k, c.k, c.Cin, c.Cout), kind, 4, 1 / math.sqrt(c.k * c.k * c.Cin))
    b = draw(g, (c.Cout,), kind)
    wp = ops().pack_conv_weights(w.to(dev))
    for relu in (False, True):
        run = lambda: ops().conv2d_nhwc_levels([x.to(dev) for x in xs], wp, b.to(dev), 1, (p, p),
                                               relu=relu, math_mode=c.math)
        ys, ys2 = run(), run()
        for lvl, (x, y, y2) in enumerate(zip(xs, ys, ys2)):
            assert torch.equal(y, y2)
            want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double(),
                            padding=p).permute(0, 2, 3, 1)
            want = want.clamp_min(0) if relu else want
            got = y.cpu().double()
            if kind == "int":
                assert torch.equal(got, want), f"{c.id} level {lvl}: {first_diff(got, want)}"
            else:
                torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4,
                                           msg=lambda m: f"{c.id} level {lvl}: {m}")
