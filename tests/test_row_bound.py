"""CPU tests of handoff.RowBound (the declared bound on a gradient's non-zero
rows, from the RPN loss to the head's backwards) and of the host side of the
row-census exports."""
import ctypes

import pytest

from detectron2_tensorflow_amd.layers import handoff
from detectron2_tensorflow_amd.layers.handoff import HandoffError, Links, RowBound


def test_undeclared_bound_is_dense_everywhere():
    b = RowBound(5)
    assert not b.declared and b.capacity(2) is None
    for M in (546, 2100, 8400, 33600, 134400, 10 ** 9):
        assert not b.wants_census(2, M)
    # the 1x1's backward then publishes "dense" and the 3x3's takes it
    b.publish(4, None)
    assert b.take(4) is None
    assert b.sparse_launches == 0


def test_declared_bound_capacity_arithmetic():
    b = RowBound(5)
    with pytest.raises(ValueError):
        b.declare(0)
    b.declare(256)
    assert b.declared and b.rows_per_image == 256
    assert b.capacity(1) == 256 and b.capacity(2) == 512
    # a census pays where even the 3x3-dilated rows (9 per non-zero row) are a
    # minority: batch 2 at 800 x 1333 -> p2, p3, p4 yes; p5, p6 no
    assert [b.wants_census(2, M) for M in (134400, 33600, 8400, 2100, 546)] == \
        [True, True, True, False, False]
    assert not b.wants_census(2, 9 * 2 * 256)      # the threshold itself: dense
    assert b.wants_census(2, 9 * 2 * 256 + 1)


def test_publish_and_take_per_level_in_backward_order():
    b = RowBound(3)
    b.declare(256)
    census = [object(), None, object()]
    for level in (2, 1, 0):  # the backward runs the levels last to first
        b.publish(level, census[level])
        assert b.take(level) is census[level]
    # a second backward of the same graph starts clean
    b.publish(0, census[0])
    assert b.take(0) is census[0]


def test_taking_twice_or_unpublished_raises():
    b = RowBound(2)
    b.declare(256)
    with pytest.raises(HandoffError, match="level 1 was not published"):
        b.take(1)
    b.publish(1, None)
    assert b.take(1) is None
    with pytest.raises(HandoffError, match="taken twice"):
        b.take(1)
    with pytest.raises(HandoffError):
        b.take(0)


def test_links_carry_the_bound_as_a_trailing_argument():
    b = RowBound(5)
    assert Links().rows is None
    assert Links(False, None, None, None, None, None).rows is None  # the positional callers
    assert Links(rows=(b, 3)).rows == (b, 3)
    assert handoff.ROW_BOUND != handoff.LEVEL_PAIR


def test_list_capacity_arithmetic():
    b = RowBound(5, dilate=(3, 1))
    assert b.list_capacity(2) is None
    b.declare(256)
    assert b.capacity(2) == 512 and b.list_capacity(2) == 9 * 512
    assert RowBound(5).dilate is None
    # the list only where it is a small fraction of the level (batch 2 at
    # 800 x 1333: p2 yes; p3, p4 census without a list; p5, p6 dense)
    assert [b.wants_list(2, M) for M in (134400, 33600, 8400, 2100, 546)] == \
        [True, False, False, False, False]
    assert b.wants_list(2, 16 * 9 * 512) and not b.wants_list(2, 16 * 9 * 512 - 1)
    plain = RowBound(5)
    plain.declare(256)
    assert plain.wants_census(2, 134400) and not plain.wants_list(2, 134400)


def test_census_workspace_sizes_and_one_byte_short_is_refused_without_gpu():
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    # without a list: the head of the layout alone
    size = lib.d2mi_row_census_workspace_size(2, 20, 26, 512, 0)
    out = (ctypes.c_int64 * 7)()
    assert lib.d2mi_row_census_layout(2, 20, 26, 512, 0, out, 7) == 0
    bitmap_off, words, rows_off, count_off, nrows_off, list_off, cap = out
    # 1,040 pixels = 32.5 chunks of 32 -> 33 bits -> 2 words
    assert words == 2 and bitmap_off == 0 and (nrows_off, list_off, cap) == (-1, -1, 0)
    assert bitmap_off + 4 * words <= rows_off and rows_off + 4 * words <= count_off
    assert size == count_off + 4
    # with a 3x3 list: capacity min(9 * capacity, pixels), at least 1; the head is unchanged
    for capacity, want in ((4, 36), (512, 1040), (0, 1)):
        full = lib.d2mi_row_census_workspace_size(2, 20, 26, capacity, 3)
        assert lib.d2mi_row_census_layout(2, 20, 26, capacity, 3, out, 7) == 0
        assert tuple(out[:4]) == (bitmap_off, words, rows_off, count_off)
        assert out[6] == want and count_off + 4 <= out[4] and out[4] + 4 <= out[5]
        assert full == out[5] + 4 * want
    assert lib.d2mi_row_census_workspace_size(2, 200, 336, 512, 0) >= 4 * ((134400 // 32 + 31) // 32)
    assert lib.d2mi_row_census_workspace_size(0, 20, 26, 512, 3) == 0
    ws = ctypes.c_void_p(256)  # non-null, never dereferenced: the carve is refused first
    full = lib.d2mi_row_census_workspace_size(2, 20, 26, 4, 3)
    rc = lib.d2mi_row_census(None, 2, 20, 26, 16, 4, 3, 1, ws, full - 1, None)
    msg = _C.last_error()
    assert rc < 0 and "too small" in msg and f"{full - 1} < {full}" in msg, (rc, msg)
    rc = lib.d2mi_conv2d_wgrad_rows(None, None, None, None, 2, 20, 26, 256, 256, 3, 3, 1, 1, 1, 4,
                                    ws, size - 1, None, 0, None)
    msg = _C.last_error()
    assert rc < 0 and "too small" in msg and f"{size - 1} < {size}" in msg, (rc, msg)
    x = ctypes.c_void_p(4096)  # (16-byte aligned, never dereferenced)
    rc = lib.d2mi_conv2d_nhwc_rows(x, x, None, None, x, 2, 20, 26, 256, 256, 3, 3, 1, 1, 1, 12,
                                   ws, full - 1, 4, 3, 1, None, 0, None)
    msg = _C.last_error()
    assert rc < 0 and "too small" in msg and f"{full - 1} < {full}" in msg, (rc, msg)
    rc = lib.d2mi_row_census(None, 2, 20, 26, 15, 512, 0, 0, ws, size, None)
    assert rc < 0 and "multiple of 4" in _C.last_error()
