"""Which rows of the frame a context holds, on the CPU (wc-path-tracer_amd/csrc/screen_layout.h, compiled here with g++
from the product header through tests/screen_layout_shim.cpp -- the functions the runtime asks on wcpt_create_screen /
wcpt_resize, wcpt_set_row_range, wcpt_set_row_stripes and the group's frame block, and the splits behind wcpt_row_block /
wcpt_row_stripes). Every transition at its boundaries; the expected layouts are written out here, from include/wcpt.h's
description of the calls, not read back from the header."""
import ctypes
import os
import subprocess

import pytest

from wcpt import dist as wdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, NO_ROWS, BAD_STRIPES, PAST_FRAME, PAST_ROW32 = 0, 1, 2, 3, 4
NO_SCREEN = (0, 0, 0, 0, 0, 0, 0)          # (width, height, y0, rows, stripe, period, sharded) of a new context


def whole(w, h):
    return (w, h, 0, h, 0, 0, 0)


@pytest.fixture(scope="module")
def sl(tmp_path_factory):
    out = tmp_path_factory.mktemp("sl") / "libscreen_layout_shim.so"
    src = os.path.join(ROOT, "tests", "screen_layout_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    u32, p = ctypes.c_uint32, ctypes.c_void_p
    lib.sl_range.argtypes = [p, u32, u32, p]
    lib.sl_stripes.argtypes = [p, u32, u32, u32, u32, p]
    lib.sl_resize.argtypes = [p, u32, u32, p]
    lib.sl_frame_block.argtypes = [p, u32, u32, u32, u32, u32, u32, p]
    lib.sl_last_row.argtypes = [p]
    lib.sl_last_row.restype = ctypes.c_uint64
    lib.sl_row_map.argtypes = [p, p]
    lib.sl_frame_row.argtypes = [p, u32]
    lib.sl_frame_row.restype = u32
    lib.sl_split.argtypes = [u32, u32, u32, u32, p]
    lib.sl_stripe_pow2.argtypes = [u32]
    lib.sl_tiles.argtypes = [p]
    lib.sl_tiles.restype = ctypes.c_uint64
    lib.sl_renderable.argtypes = [p]
    return lib


def _words(layout):
    return (ctypes.c_uint32 * 7)(*layout)


def _call(fn, old, *args):
    """(refusal, new layout or None)"""
    out = (ctypes.c_uint32 * 7)(*([0xDEAD] * 7))
    rc = fn(_words(old), *args, out)
    return rc, (tuple(int(v) for v in out) if rc == OK else None)


def _rows(sl, layout):
    """the frame rows of the layout's local rows 0, 1, ..."""
    w = _words(layout)
    return [int(sl.sl_frame_row(w, ly)) for ly in range(layout[3])]


def test_row_map_of_a_layout(sl):
    """Local row ly is frame row y0 + ly + (ly / stripe) * (period - stripe): shift log2(stripe), gap period - stripe; a
    block has shift 31 and no gap."""
    for layout, want in (((16, 20, 4, 6, 0, 0, 1), (4, 31, 0)), (whole(16, 20), (0, 31, 0)),
                         ((16, 20, 5, 15, 1, 1, 1), (5, 0, 0)), ((16, 20, 0, 10, 2, 4, 1), (0, 1, 2)),
                         ((8, 70000, 3, 9, 32768, 65536, 1), (3, 15, 32768))):
        out = (ctypes.c_uint32 * 3)()
        sl.sl_row_map(_words(layout), out)
        assert tuple(out) == want, layout
    assert _rows(sl, (16, 20, 0, 10, 2, 4, 1)) == [0, 1, 4, 5, 8, 9, 12, 13, 16, 17]
    assert _rows(sl, (16, 10, 0, 6, 4, 8, 1)) == [0, 1, 2, 3, 8, 9]        # a short last stripe
    assert sl.sl_last_row(_words((16, 20, 0, 10, 2, 4, 1))) == 17
    assert sl.sl_last_row(_words((0, 0, 0xFFFFFFF0, 32, 1, 1, 1))) == 0xFFFFFFF0 + 31   # 64 bits: no wrap


def test_rows_a_render_can_address(sl):
    """include/wcpt.h, "Frame sizes": a context's rows may cover at most 2^26 - 1 tiles of 8x8 pixels (2^32 - 64 lanes),
    whatever the size of the frame around them; counted in 64 bits, so no product wraps into the accepted range."""
    def tiles(layout):
        return int(sl.sl_tiles(_words(layout)))

    def ok(layout):
        return sl.sl_renderable(_words(layout)) == 1
    assert tiles(whole(1, 1)) == 1 and tiles(whole(9, 9)) == 4 and tiles(whole(70, 1)) == 9 and ok(whole(1, 1))
    band = (65521, 65599, 65548, 8, 0, 0, 1)                  # 8 rows of a frame of more than 2^32 pixels
    assert tiles(band) == 8191 and ok(band)
    assert tiles(whole(65521, 65599)) == 8191 * 8200 and not ok(whole(65521, 65599))
    # the boundary: 2^26 - 1 tiles fit, 2^26 do not
    for layout in (whole(65536, 65528), whole(65528, 65536)):
        assert tiles(layout) == 2 ** 26 - 8192 and ok(layout)
    row = ((2 ** 26 - 1) * 8, 8, 0, 8, 0, 0, 0)
    assert tiles(row) == 2 ** 26 - 1 and ok(row)
    assert tiles(whole(65536, 65536)) == 2 ** 26 and not ok(whole(65536, 65536))
    assert tiles(whole(65529, 65536)) == 2 ** 26 and not ok(whole(65529, 65536))      # partial tiles count whole
    big = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0, 0, 0)
    assert tiles(big) == 2 ** 58 and not ok(big)                                       # no wrap in 64 bits
    assert not ok((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFF0, 8, 0, 0, 1))                    # 2^29 tiles in one tile row


def test_set_row_stripes(sl):
    scr = whole(16, 20)
    # stripes of 1, 2 and 32768 rows
    assert _call(sl.sl_stripes, scr, 5, 15, 1, 1) == (OK, (16, 20, 5, 15, 1, 1, 1))
    assert _call(sl.sl_stripes, scr, 0, 10, 2, 4) == (OK, (16, 20, 0, 10, 2, 4, 1))
    assert _call(sl.sl_stripes, whole(8, 70000), 3, 32769, 32768, 65536) == (OK, (8, 70000, 3, 32769, 32768, 65536, 1))
    assert _call(sl.sl_stripes, scr, 0, 4, 32768, 32768) == (OK, (16, 20, 0, 4, 32768, 32768, 1))
    # no power of two, more than 32768 rows, period < stripe, no rows
    assert _call(sl.sl_stripes, scr, 0, 4, 3, 8)[0] == BAD_STRIPES
    assert _call(sl.sl_stripes, scr, 0, 4, 65536, 65536)[0] == BAD_STRIPES
    assert _call(sl.sl_stripes, scr, 0, 4, 8, 4)[0] == BAD_STRIPES
    assert _call(sl.sl_stripes, scr, 0, 0, 8, 16)[0] == NO_ROWS
    # the last row is height - 1 (kept) or height (refused)
    assert _call(sl.sl_stripes, scr, 2, 10, 2, 4) == (OK, (16, 20, 2, 10, 2, 4, 1))       # rows 2,3, 6,7, ... 18,19
    assert _call(sl.sl_stripes, scr, 3, 10, 2, 4)[0] == PAST_FRAME                        # ... 19,20
    assert _call(sl.sl_stripes, scr, 0, 11, 2, 4)[0] == PAST_FRAME                        # the 11th row is row 20
    assert _call(sl.sl_stripes, scr, 8, 9, 8, 16)[0] == PAST_FRAME                        # row 24
    # a short last stripe
    assert _call(sl.sl_stripes, whole(16, 10), 0, 6, 4, 8) == (OK, (16, 10, 0, 6, 4, 8, 1))  # rows 0..3, 8,9
    assert _call(sl.sl_stripes, whole(16, 9), 0, 6, 4, 8)[0] == PAST_FRAME
    # it replaces a block; the frame's size stays
    assert _call(sl.sl_stripes, (16, 20, 4, 6, 0, 0, 1), 0, 8, 4, 8) == (OK, (16, 20, 0, 8, 4, 8, 1))


def test_stripes_before_a_screen_and_past_row_2_32(sl):
    # with no screen the frame's height is not known: held unchecked ...
    assert _call(sl.sl_stripes, NO_SCREEN, 1000, 5000, 8, 64) == (OK, (0, 0, 1000, 5000, 8, 64, 1))
    # ... but for a last row that 32 bits cannot hold
    assert _call(sl.sl_stripes, NO_SCREEN, 0xFFFFFFE0, 32, 1, 1) == (OK, (0, 0, 0xFFFFFFE0, 32, 1, 1, 1))  # row 2^32 - 1
    assert _call(sl.sl_stripes, NO_SCREEN, 0xFFFFFFE1, 32, 1, 1)[0] == PAST_ROW32                        # row 2^32
    assert _call(sl.sl_stripes, NO_SCREEN, 0, 8, 2, 1 << 31)[0] == PAST_ROW32          # 3 gaps of 2^31 - 2 rows
    # with a screen the height is checked first
    assert _call(sl.sl_stripes, whole(16, 20), 0, 8, 2, 1 << 31)[0] == PAST_FRAME


def test_set_row_range(sl):
    scr = whole(16, 20)
    assert _call(sl.sl_range, scr, 4, 6) == (OK, (16, 20, 4, 6, 0, 0, 1))
    assert _call(sl.sl_range, scr, 14, 6) == (OK, (16, 20, 14, 6, 0, 0, 1))        # its last row is row 19
    assert _call(sl.sl_range, scr, 15, 6)[0] == PAST_FRAME                          # ... row 20
    assert _call(sl.sl_range, scr, 20, 1)[0] == PAST_FRAME
    assert _call(sl.sl_range, scr, 0xFFFFFFFF, 2)[0] == PAST_FRAME                  # y0 + rows does not wrap
    assert _call(sl.sl_range, (16, 20, 0, 8, 4, 8, 1), 4, 6) == (OK, (16, 20, 4, 6, 0, 0, 1))   # clears the stripes
    # rows == 0: the whole frame again, stripes cleared
    assert _call(sl.sl_range, (16, 20, 4, 6, 0, 0, 1), 0, 0) == (OK, scr)
    assert _call(sl.sl_range, (16, 20, 0, 8, 4, 8, 1), 9, 0) == (OK, scr)
    # ... with no screen there is no frame to return to: y0 / rows stay as they are
    assert _call(sl.sl_range, (0, 0, 7, 3, 0, 0, 1), 0, 0) == (OK, (0, 0, 7, 3, 0, 0, 0))
    assert _call(sl.sl_range, (0, 0, 7, 3, 4, 8, 1), 0, 0) == (OK, (0, 0, 7, 3, 0, 0, 0))
    assert _call(sl.sl_range, NO_SCREEN, 0, 0) == (OK, NO_SCREEN)
    # a range before the first screen is held unchecked
    assert _call(sl.sl_range, NO_SCREEN, 7, 3) == (OK, (0, 0, 7, 3, 0, 0, 1))
    assert _call(sl.sl_range, NO_SCREEN, 1000, 5000) == (OK, (0, 0, 1000, 5000, 0, 0, 1))


def test_resize_keeps_clips_or_falls_back(sl):
    assert _call(sl.sl_resize, NO_SCREEN, 0, 8)[0] == NO_ROWS
    assert _call(sl.sl_resize, whole(16, 20), 8, 0)[0] == NO_ROWS
    assert _call(sl.sl_resize, NO_SCREEN, 16, 12) == (OK, whole(16, 12))
    assert _call(sl.sl_resize, whole(16, 12), 40, 52) == (OK, whole(40, 52))
    # a block: kept while it fits, clipped by a shrinking frame, dropped when its first row is past the frame
    blk = (16, 12, 4, 6, 0, 0, 1)
    assert _call(sl.sl_resize, blk, 32, 10) == (OK, (32, 10, 4, 6, 0, 0, 1))       # rows 4..9 of 10
    assert _call(sl.sl_resize, blk, 16, 8) == (OK, (16, 8, 4, 4, 0, 0, 1))         # rows 4..7
    assert _call(sl.sl_resize, blk, 16, 5) == (OK, (16, 5, 4, 1, 0, 0, 1))
    assert _call(sl.sl_resize, blk, 16, 4) == (OK, whole(16, 4))                   # y0 == height
    assert _call(sl.sl_resize, blk, 16, 3) == (OK, whole(16, 3))
    # a range set before the first screen meets the same rule at that screen
    assert _call(sl.sl_resize, (0, 0, 7, 3, 0, 0, 1), 16, 12) == (OK, (16, 12, 7, 3, 0, 0, 1))
    assert _call(sl.sl_resize, (0, 0, 7, 3, 0, 0, 1), 16, 9) == (OK, (16, 9, 7, 2, 0, 0, 1))
    assert _call(sl.sl_resize, (0, 0, 7, 3, 0, 0, 1), 16, 7) == (OK, whole(16, 7))
    assert _call(sl.sl_resize, (0, 0, 1, 0xFFFFFFFF, 0, 0, 1), 16, 10) == (OK, (16, 10, 1, 9, 0, 0, 1))  # no 32-bit wrap
    assert _call(sl.sl_resize, (0, 0, 7, 3, 0, 0, 0), 16, 12) == (OK, whole(16, 12))    # after rows == 0 with no screen
    # stripes: kept whole while their last row lies in the new frame, else the whole frame -- never clipped
    st = (16, 20, 4, 8, 4, 8, 1)                                                   # rows 4..7 and 12..15
    assert _call(sl.sl_resize, st, 24, 16) == (OK, (24, 16, 4, 8, 4, 8, 1))        # last row 15 == height - 1
    assert _call(sl.sl_resize, st, 16, 15) == (OK, whole(16, 15))                  # last row == height
    assert _call(sl.sl_resize, st, 16, 12) == (OK, whole(16, 12))
    assert _call(sl.sl_resize, (0, 0, 4, 8, 4, 8, 1), 16, 16) == (OK, (16, 16, 4, 8, 4, 8, 1))   # set before the screen
    assert _call(sl.sl_resize, (0, 0, 4, 8, 4, 8, 1), 16, 15) == (OK, whole(16, 15))
    assert _call(sl.sl_resize, (16, 20, 4, 0, 4, 8, 1), 16, 20) == (OK, whole(16, 20))           # stripes of no rows
    # a group's rank that holds the whole frame is a block like any other
    assert _call(sl.sl_resize, (16, 12, 0, 12, 0, 0, 1), 16, 20) == (OK, (16, 20, 0, 12, 0, 0, 1))


def test_frame_block(sl):
    for old in (NO_SCREEN, whole(40, 52), (40, 52, 8, 16, 8, 24, 1)):
        assert _call(sl.sl_frame_block, old, 16, 12, 0, 12, 0, 0) == (OK, (16, 12, 0, 12, 0, 0, 1))   # sharded all the same
        assert _call(sl.sl_frame_block, old, 16, 12, 4, 8, 0, 99) == (OK, (16, 12, 4, 8, 0, 0, 1))    # last row 11; no period
        assert _call(sl.sl_frame_block, old, 16, 12, 4, 9, 0, 0)[0] == PAST_FRAME                      # last row 12
        assert _call(sl.sl_frame_block, old, 0, 12, 0, 12, 0, 0)[0] == NO_ROWS
        assert _call(sl.sl_frame_block, old, 16, 12, 0, 0, 0, 0)[0] == NO_ROWS
        assert _call(sl.sl_frame_block, old, 16, 17, 16, 1, 8, 24) == (OK, (16, 17, 16, 1, 8, 24, 1))  # a short stripe alone
        assert _call(sl.sl_frame_block, old, 16, 16, 16, 1, 8, 24)[0] == PAST_FRAME
        assert _call(sl.sl_frame_block, old, 16, 40, 0, 16, 8, 24) == (OK, (16, 40, 0, 16, 8, 24, 1))  # rows 0..7, 24..31
        assert _call(sl.sl_frame_block, old, 16, 31, 0, 16, 8, 24)[0] == PAST_FRAME
        assert _call(sl.sl_frame_block, old, 16, 40, 0, 16, 3, 24)[0] == BAD_STRIPES
        assert _call(sl.sl_frame_block, old, 16, 40, 0, 16, 65536, 1 << 20)[0] == BAD_STRIPES
        assert _call(sl.sl_frame_block, old, 16, 40, 0, 16, 8, 4)[0] == BAD_STRIPES
        assert _call(sl.sl_frame_block, old, 16, 40, 0, 0, 3, 24)[0] == BAD_STRIPES                   # the stripes come first


def test_the_ranks_rows_partition_the_frame(sl):
    """wcpt_row_block / wcpt_row_stripes: for every height, rank count and stripe the ranks' rows are the frame's rows,
    each once; every rank's layout is one wcpt_set_row_stripes accepts; and wcpt.dist computes the same."""
    assert [s for s in range(1, 70) if sl.sl_stripe_pow2(s)] == [1, 2, 4, 8, 16, 32, 64]
    for stripe in (0, 1, 2, 4, 8):
        for n in range(1, 6):
            for height in range(1, 41):
                seen = []
                for rank in range(n):
                    out = (ctypes.c_uint32 * 2)()
                    sl.sl_split(height, n, rank, stripe, out)
                    y, rows = int(out[0]), int(out[1])
                    assert (y, rows) == wdist.row_stripes(height, n, rank, stripe), (height, n, rank, stripe)
                    if stripe == 0:
                        assert (y, rows) == (rank * height // n, (rank + 1) * height // n - rank * height // n)
                    else:
                        assert y == rank * stripe
                    layout = (1, height, y, rows, stripe, n * stripe if stripe else 0, 1)
                    mine = _rows(sl, layout)
                    assert mine == wdist.frame_rows(height, n, rank, stripe)
                    if rows:
                        assert _call(sl.sl_stripes if stripe else sl.sl_range, whole(1, height), y, rows,
                                     *((stripe, n * stripe) if stripe else ())) == (OK, layout)
                    seen += mine
                assert sorted(seen) == list(range(height)), (height, n, stripe)
                assert len(set(seen)) == height
