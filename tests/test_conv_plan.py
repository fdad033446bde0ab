"""CPU tests of the conv / multi-level conv / wgrad launch plans (csrc/conv_plan.h)
through the plan queries of the C ABI: no launch, no device memory.

tests/conv_plans.json is the plan of every conv and wgrad shape of the
training step (profiles/r6_train_conv_shapes.txt; split math, f32 math,
unaligned operands, no workspace) and of the RetinaNet / SOLOv2 / RPN level
sets, recorded from the planning code as it was BEFORE the planners moved into
conv_plan.h (that code's own make_plan, fallback, streaming rule,
levels_splits, wplan and kernel if-chain, called from query exports added to
a scratch copy).  A change of the plan rules shows up as a diff of that file."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AL, WS = 8 | 16 | 64, 32  # operands: everything 16-byte aligned; a workspace is passed


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (binds the HIP runtime torch ships)
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    return _C.load()


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "conv_plans.json")) as f:
        t = json.load(f)
    assert t["columns"] == ["shape", "flags", "operands", "workspace_bytes", "plan"]
    assert len(t["rows"]) == 504
    return t["rows"]


def parse(shape):
    """('conv' | 'wgrad' | 'levels', the query's leading arguments) of a table shape string."""
    w = shape.split()
    if w[0] == "levels":
        dims = [int(d) for lv in w[3].split("+") for d in lv.split("x")]
        cin, cout = map(int, w[4].split("->"))
        k, s, pb, pe = int(w[5][1:]), int(w[6][1:]), int(w[7][1]), int(w[7][2])
        return "levels", ((ctypes.c_int32 * len(dims))(*dims), len(dims) // 3, cin, cout, k, k, s, pb, pe)
    N, H, W, Cin, Cout = map(int, re.match(r"(\d+)x(\d+)x(\d+)x(\d+)->(\d+)$", w[1]).groups())
    k, s = int(w[2][1:]), int(w[3][1:])
    pb, pe = (int(w[4][1]), int(w[4][2])) if w[0] == "conv" else ((k - 1) // 2, k - 1 - (k - 1) // 2)
    return w[0], (N, H, W, Cin, Cout, k, k, s, pb, pe)


def query(lib, kind, args, flags, operands, wsb, n=40):
    fn = {"conv": lib.d2mi_conv2d_plan, "wgrad": lib.d2mi_conv2d_wgrad_plan,
          "levels": lib.d2mi_conv2d_levels_plan}[kind]
    out = (ctypes.c_int32 * 40)()
    rc = fn(*args, flags, operands, wsb, out, n)
    return rc, list(out)[:max(rc, 0)]


def size_of(lib, kind, args):
    return {"conv": lib.d2mi_conv2d_workspace_size, "wgrad": lib.d2mi_conv2d_wgrad_workspace_size,
            "levels": lib.d2mi_conv2d_levels_workspace_size}[kind](*args)


def fields(kind, v):
    """The fields the checks below read: (splits of every launch, tail tiles, bytes, family)."""
    if kind == "conv":
        return dict(family=v[0], splits=v[12], tail_tiles=v[19], bytes=v[31] | v[32] << 31)
    if kind == "levels":
        return dict(family=v[0], splits=v[9], tail_tiles=0, bytes=v[27] | v[28] << 31)
    return dict(family=None, splits=v[9], tail_tiles=0, bytes=v[14] | v[15] << 31)


def test_plans_reproduce_the_recorded_table(lib, table):
    kinds = {}
    for shape, flags, operands, wsb, want in table:
        kind, args = parse(shape)
        rc, got = query(lib, kind, args, flags, operands, wsb)
        assert rc == len(want) and got == want, (shape, flags, operands, wsb, got, want)
        kinds[kind] = kinds.get(kind, 0) + 1
    # 98 profile lines: 74 convs x 4 cases, 24 wgrads x 5; 22 level sets x 4
    assert kinds == {"conv": 296, "wgrad": 120, "levels": 88}
    # the table holds every decision: split-K, tail split, each family, four wgrad kernels
    convs = [r[4] for r in table if r[0].startswith("conv ")]
    assert {p[0] for p in convs} == {0, 1, 2, 3, 4}
    assert any(p[12] > 1 for p in convs) and any(p[19] > 0 for p in convs)
    assert {r[4][0] for r in table if r[0].startswith("wgrad ")} >= {0, 1, 3, 4}
    assert any(r[4][9] > 1 for r in table if r[0].startswith("levels "))


def test_plan_fits_the_queried_workspace_and_uses_all_of_it_when_it_splits(lib, table):
    split_seen = 0
    for shape in sorted({r[0] for r in table}):
        kind, args = parse(shape)
        wsb = size_of(lib, kind, args)
        for flags in (4, 0):
            rc, v = query(lib, kind, args, flags, AL | WS, wsb)
            p = fields(kind, v)
            assert rc > 0 and p["bytes"] <= wsb, (shape, flags, p, wsb)
            # the size export assumes split math (wgrad: the larger of both maths)
            if flags == 4 and kind != "wgrad" and (p["splits"] > 1 or p["tail_tiles"] > 0):
                assert p["bytes"] == wsb, (shape, p, wsb)
                split_seen += 1
        if kind == "wgrad":
            both = [fields(kind, query(lib, kind, args, f, AL | WS, wsb)[1])["bytes"] for f in (4, 0)]
            assert max(both) == wsb, (shape, both, wsb)
    assert split_seen >= 10


def test_workspace_one_byte_short_gives_the_one_pass_plan(lib, table):
    n = 0
    for shape in sorted({r[0] for r in table}):
        kind, args = parse(shape)
        wsb = size_of(lib, kind, args)
        if wsb == 0:
            continue
        full = fields(kind, query(lib, kind, args, 4, AL | WS, wsb)[1])
        rc, v = query(lib, kind, args, 4, AL | WS, wsb - 1)
        p = fields(kind, v)
        if kind == "wgrad" and full["bytes"] < wsb:  # (the f32 plan is the larger one)
            continue
        assert rc > 0 and p["splits"] == 1 and p["tail_tiles"] == 0 and p["bytes"] == 0, (shape, p)
        n += 1
    assert n >= 20


def test_streaming_shapes_have_a_tiled_plan_without_split_or_tail(lib, table):
    """The tiled kernels sum K in the streaming kernel's order only when their
    plan has neither split-K nor a tail split: a launch of the same shape whose
    operands are not 16-byte aligned must round like an aligned one."""
    n = 0
    for shape, flags, operands, wsb, plan in table:
        if not shape.startswith("conv ") or plan[0] != 4:
            continue
        kind, args = parse(shape)
        rc, v = query(lib, kind, args, flags, operands & ~(8 | 16), wsb)
        assert rc > 0 and v[0] in (0, 1, 2, 3) and v[12] == 1 and v[19] == 0, (shape, v)
        assert plan[12] == 1 and plan[19] == 0  # (and so does the plan it does not launch)
        n += 1
    assert n >= 5


def test_former_environment_knobs_steer_the_plans_in_process(lib):
    from detectron2_tensorflow_amd.layers import ops
    p3 = (2, 100, 168, 256, 256, 3)  # FPN p3 3x3: 526 tiles + a split-K tail
    before = ops.conv_plan(*p3, pad=(1, 1))
    assert before["tail_tiles"] > 0 and before["tail_splits"] > 1
    wshape = (2, 200, 336, 256, 256, 3)
    wbefore = ops.wgrad_plan(*wshape, pad=(1, 1))
    assert wbefore["splits"] > 4
    try:
        ops.set_tuning("conv_tail", 0)
        off = ops.conv_plan(*p3, pad=(1, 1))
        assert off["tail_tiles"] == 0 and off["main_tiles"] == before["nM"] * before["nN"]
        assert off["workspace_bytes"] == 0
        ops.set_tuning("wgrad_maxsplit", 4)
        capped = ops.wgrad_plan(*wshape, pad=(1, 1))
        assert 1 < capped["splits"] <= 4 and capped["kernel"] == wbefore["kernel"]
    finally:
        ops.set_tuning("conv_tail", 1)
        ops.set_tuning("wgrad_maxsplit", 128)
    assert ops.conv_plan(*p3, pad=(1, 1)) == before
    assert ops.wgrad_plan(*wshape, pad=(1, 1)) == wbefore
    # set_tuning drops the cached workspace sizes: they depend on the knobs
    # (written and checked where conv2d_nhwc / conv2d_wgrad look them up)
    ops.conv._CONV_WS["stale"] = 1
    ops.conv._WGRAD_WS["stale"] = 1
    ops.set_tuning("conv_tail", 1)
    assert not ops.conv._CONV_WS and not ops.conv._WGRAD_WS


def test_plan_dicts_name_the_fields(lib):
    from detectron2_tensorflow_amd.layers import ops
    p = ops.conv_plan(2, 200, 336, 64, 256, 1, operands=ops.OP_ALL_ALIGNED | ops.OP_RESIDUAL)
    assert ops.CONV_FAMILIES[p["family"]] == "stream1x1" and p["stream_kmax"] == 64
    assert p["stream_form"] == 1 and p["stream_grid"] > 0 and p["workspace_bytes"] == 0
    lv = ops.conv_levels_plan([(1, 13, 21), (1, 7, 11)], 256, 256, 3, pad=(1, 1))
    assert lv["nlev"] == 2 and lv["splits"] > 1 and lv["tile0"][2] == lv["tiles"]
    assert lv["moff"][6] == 13 * 21 + 7 * 11
    assert lv["workspace_bytes"] == lv["splits"] * lv["moff"][6] * 256 * 4
    w = ops.wgrad_plan(2, 50, 84, 256, 256, 3, pad=(1, 1))
    assert ops.WGRAD_KERNELS[w["kernel"]] == "ws_inc" and w["part"] == 1
    assert w["workspace_bytes"] == w["splits"] * (9 * 256 * 256 + 256) * 4


def test_plan_queries_refuse_what_the_launchers_refuse(lib):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers import ops
    args = (2, 50, 84, 256, 256, 3, 3, 1, 1, 1)
    dims = (ctypes.c_int32 * 3)(2, 50, 84)
    largs = (dims, 1, 256, 256, 3, 3, 1, 1, 1)
    for kind, a, n in (("conv", args, 33), ("wgrad", args, 16), ("levels", largs, 29)):
        rc, v = query(lib, kind, a, 4, AL | WS, 1 << 30, n)
        assert rc == n and len(v) == n
        rc, _ = query(lib, kind, a, 4, AL | WS, 1 << 30, n - 1)
        assert rc < 0 and f"out_len {n - 1} is short of the plan's {n}" in _C.last_error(), kind
    rc, _ = query(lib, "conv", (2, 50, 84, 3, 256, 3, 3, 1, 1, 1), 4, AL, 0)
    assert rc < 0 and "multiple of 4" in _C.last_error()
    rc, _ = query(lib, "conv", (2, 2, 2, 64, 64, 3, 3, 1, 0, 0), 4, AL, 0)
    assert rc < 0 and "conv output is empty" in _C.last_error()
    rc, _ = query(lib, "wgrad", (2, 50, 84, 256, 6, 3, 3, 1, 1, 1), 4, AL, 0)
    assert rc < 0 and "multiples of 4" in _C.last_error()
    rc, _ = query(lib, "wgrad", args, 12, AL, 0)  # accumulating without a slab
    assert rc < 0 and "accumulating wgrad: workspace must hold 1 slab(s)" in _C.last_error()
    rc, _ = query(lib, "levels", ((ctypes.c_int32 * 3)(2, 0, 84),) + largs[1:], 4, AL, 0)
    assert rc < 0 and "level 0: bad or empty conv geometry" in _C.last_error()
    rc, _ = query(lib, "levels", (dims, 7) + largs[2:], 4, AL, 0)
    assert rc < 0 and "nlev=7" in _C.last_error()
    with pytest.raises(_C.D2MIError, match="multiple of 4"):
        ops.conv_plan(2, 50, 84, 3, 256, 3)
