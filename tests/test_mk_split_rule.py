"""The split-render rule and queue layout on the CPU (wc-path-tracer_amd/csrc/mk_split_rule.h, compiled here with g++
from the product header through tests/mk_split_rule_shim.cpp): every condition that keeps a render whole, the cut never
past maxBounceCount, and queues that hold every pixel of their launch for row blocks, stripes and both pipes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO = -1
SLOTS = 16 * 256          # 4 waves per SIMD on 256 compute units
BIG = 32400               # the tiles of a 1920x1080 frame


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("mks") / "libmk_split_rule_shim.so"
    src = os.path.join(ROOT, "tests", "mk_split_rule_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    lib.mks_cut.argtypes = [ctypes.c_int, ctypes.c_int, u32, u32, u64, u64, u64]
    lib.mks_cut.restype = u32
    lib.mks_layout.argtypes = [u32, ctypes.c_int, ctypes.c_void_p]
    lib.mks_layout.restype = None
    for name in ("mks_sub_first", "mks_sub_cap"):
        getattr(lib, name).argtypes = [u32, u32]
        getattr(lib, name).restype = u32
    return lib


def _cut(shim, option=AUTO, splittable=1, samples=1, bounces=4, waves=BIG, slots=SLOTS, triangles=34):
    return shim.mks_cut(option, splittable, samples, bounces, waves, slots, triangles)


def _layout(shim, tiles, piped):
    out = np.zeros(5, np.uint64)
    shim.mks_layout(tiles, 1 if piped else 0, out.ctypes.data)
    return [int(v) for v in out]


def test_constants(shim):
    assert shim.mks_entry_bytes() == 56           # 14 u32: 1920 x 1080 x 56 B = 116 MB
    assert 2 <= shim.mks_auto_cut() <= 4
    assert shim.mks_max_cut() == 15


def test_automatic_rule_on_the_headline(shim):
    assert _cut(shim) == shim.mks_auto_cut()
    assert _cut(shim, waves=BIG // 2) == shim.mks_auto_cut()     # a 2-way row block: 4 rounds


@pytest.mark.parametrize("kw", [dict(option=0), dict(splittable=0), dict(samples=0), dict(samples=2), dict(samples=4),
                                dict(bounces=0), dict(bounces=1), dict(waves=0), dict(waves=BIG // 8),
                                dict(waves=BIG // 4), dict(waves=SLOTS), dict(waves=3 * SLOTS - 1),
                                dict(triangles=65), dict(triangles=10 ** 6), dict(triangles=2 ** 40)])
def test_every_off_condition_of_the_automatic_rule(shim, kw):
    """The option at 0, a counting / scratch-stack launch, samples != 1, maxBounceCount < 2, and launches of less than
    3 rounds of resident waves (the 8- and 4-way blocks of 1080p are one and two rounds: both measured a loss), and a
    mesh of more than 64 triangles (the reference's scene measured a loss at every cut)."""
    assert _cut(shim, **kw) == 0


def test_small_meshes_and_sphere_scenes_split(shim):
    for triangles in (0, 1, 34, 64):
        assert _cut(shim, triangles=triangles) == shim.mks_auto_cut()
    assert _cut(shim, option=3, triangles=10 ** 6) == 3       # a forced cut ignores the mesh


def test_threshold_is_three_rounds(shim):
    assert _cut(shim, waves=3 * SLOTS) == shim.mks_auto_cut()
    assert _cut(shim, waves=3 * SLOTS - 1) == 0


@pytest.mark.parametrize("option", [1, 2, 3, 4, 7, 15])
def test_forced_cut(shim, option):
    """A forced cut ignores the launch's size, but not what has no head and tail builds."""
    for bounces in range(0, 17):
        want = option if option <= bounces else 0
        assert _cut(shim, option=option, bounces=bounces, waves=1) == want
    assert _cut(shim, option=option, samples=2, bounces=16) == 0
    assert _cut(shim, option=option, samples=0, bounces=16) == 0
    assert _cut(shim, option=option, splittable=0, bounces=16) == 0
    assert _cut(shim, option=option, bounces=16, waves=0) == 0


def test_cut_never_exceeds_max_bounce(shim):
    for option in range(-1, 16):
        for bounces in range(0, 20):
            for waves in (1, SLOTS, BIG):
                c = _cut(shim, option=option, bounces=bounces, waves=waves)
                assert c <= bounces
                assert c == 0 or c >= 1
    assert _cut(shim, bounces=2) == 2 and _cut(shim, bounces=3) == 3 and _cut(shim, bounces=12) == shim.mks_auto_cut()


def _tiles(w, rows):
    return ((w + 7) // 8) * ((rows + 7) // 8)


@pytest.mark.parametrize("w,rows", [(1920, 1080), (1920, 544), (1920, 136), (64, 40), (8, 8), (80, 72), (80, 36),
                                    (1920, 270), (1920, 135)])
def test_capacity_is_the_launch_s_pixels(shim, w, rows):
    """Whole-tile frames, their row blocks and the rows of a striped rank (a stripe of 8 rows is a tile row): the
    unpiped queue holds exactly the launch's pixels, the two pipes' queues exactly theirs, back to back in an
    allocation of the frame's pixels. Where the last tile row is partial (36 rows, the 270- and 135-row blocks of
    1080p) the queue holds the launch's lanes, which bound its pixels."""
    tiles = _tiles(w, rows)
    whole = w % 8 == 0 and rows % 8 == 0
    cap0, cap1, first0, first1, entries = _layout(shim, tiles, False)
    assert (cap0, cap1, first0) == (64 * tiles, 0, 0) and entries == 64 * tiles
    assert cap0 == w * rows if whole else cap0 >= w * rows
    cap0, cap1, first0, first1, entries = _layout(shim, tiles, True)
    half = (tiles + 1) // 2                      # launch_megakernel: pipe 0 takes the order's even positions
    assert (cap0, cap1) == (64 * half, 64 * (tiles - half))
    assert first0 == 0 and first1 == cap0 and first1 + cap1 == entries == 64 * tiles
    if whole:
        assert cap0 + cap1 == w * rows


@pytest.mark.parametrize("blocks", [0, 1, 2, 63, 64, 65, 127, 128, 4050, 16200, 32400, 32401])
def test_sub_queues_tile_the_queue(shim, blocks):
    """The sub-queues' shares lie back to back and add up to the queue; sub-queue j holds 64 entries per head block
    b with b mod 64 == j, which is also the number of tail blocks that finish it."""
    subs = shim.mks_sub_queues()
    at = 0
    for j in range(subs):
        assert shim.mks_sub_first(blocks, j) == at
        cap = shim.mks_sub_cap(blocks, j)
        assert cap == 64 * len(range(j, blocks, subs))
        at += cap
    assert at == 64 * blocks
    assert shim.mks_counter_words() >= subs


@pytest.mark.parametrize("w,rows", [(70, 45), (1, 1), (9, 17), (1921, 1081)])
def test_partial_tiles_never_overflow(shim, w, rows):
    """A pipe's launch has at most 64 pixels per tile, whichever tiles the cost order deals it."""
    tiles = _tiles(w, rows)
    for piped in (False, True):
        cap0, cap1, first0, first1, entries = _layout(shim, tiles, piped)
        assert cap0 + cap1 == 64 * tiles >= w * rows
        assert entries * 56 >= (first1 + cap1) * 56
