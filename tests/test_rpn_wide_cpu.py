"""The 15-anchor single-level RPN (the C4 / DC5 families) without a GPU: the
host-side bounds of the entries it widened -- 15 anchors per cell in the
RPN / RetinaNet cell table, the skinny weight gradient's 80 output columns,
the pre-NMS top-k above 8,192 -- through the loaded library."""
import ctypes

import numpy as np

WGRAD_MAX_COUT = 80   # csrc/wgrad_skinny.hip kMaxCoutWide: five blocks of 16 columns
CHUNK = 128           # pixels per chunk partial


def _lib():
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    return _C, _C.load()


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_sixteen_anchors_per_cell_are_refused_with_the_bound_of_15():
    _C, lib = _lib()
    cell = (ctypes.c_float * (16 * 4))(*np.arange(64, dtype=np.float32))
    assert lib.d2mi_grid_anchors(5, 7, 16.0, cell, 16, None, None) < 0
    assert "A=16 out of range [1,15]" in _C.last_error()


def test_wgrad_skinny_refuses_one_column_past_its_ceiling():
    _C, lib = _lib()
    ws, big = ctypes.c_void_p(256), 1 << 40
    bad = WGRAD_MAX_COUT + 1
    assert lib.d2mi_wgrad_skinny_ex(None, None, 300, 64, bad, None, None, 0, ws, big, None) < 0
    assert f"Cout={bad}" in _C.last_error() and f"1..{WGRAD_MAX_COUT})" in _C.last_error()
    ptr = (ctypes.c_void_p * 1)(256)
    assert lib.d2mi_wgrad_skinny_levels(ptr, ptr, _i32([300]), 1, 64, bad, None, None, 0, ws, big,
                                        None) < 0
    assert f"Cout={bad}" in _C.last_error() and f"1..{WGRAD_MAX_COUT})" in _C.last_error()


def test_wgrad_skinny_workspace_is_the_chunk_partials_at_76_columns():
    """One layout for every width: [chunks][Cin + 1][Cout] floats, the chunks
    of the levels one after another."""
    _C, lib = _lib()
    Ps, Cin, Cout = [8400, 129], 1024, 76
    chunks = sum((p + CHUNK - 1) // CHUNK for p in Ps)
    assert lib.d2mi_wgrad_skinny_levels_workspace_size(_i32(Ps), 2, Cin, Cout) == \
        chunks * (Cin + 1) * Cout * 4
    assert lib.d2mi_wgrad_skinny_workspace_size(Ps[0], Cin, Cout) == 66 * (Cin + 1) * Cout * 4


def test_rpn_proposals_workspace_grows_with_the_wide_top_k():
    _C, lib = _lib()
    lhw = _i32([24, 24])
    wide = lib.d2mi_rpn_proposals_workspace_size(2, 1, lhw, 15, 12000, 2000)
    narrow = lib.d2mi_rpn_proposals_workspace_size(2, 1, lhw, 15, 8192, 2000)
    assert wide > narrow > 0
    # the wide route's own share: every candidate's key twice (unsorted,
    # sorted) and the segmented sort's ping-pong copy, 2 x 8,640 keys each
    assert wide - narrow >= 3 * 2 * 24 * 24 * 15 * 8
