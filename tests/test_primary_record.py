"""The primary cache's entry on the CPU (wc-path-tracer_amd/csrc/primary_record.h, compiled here with g++ from the product
header through tests/primary_record_shim.cpp): eight words per pixel, nothing narrowed, `front` in t's sign bit, a miss
as kInfinity, and the tile-major layout that launch_megakernel allocates.

kInfinity is the project's (pt_math.h): 3.402823466e+38, the largest finite binary32. An Intersect accepts t only when
0 < t < rec.t with rec.t starting at kInfinity, so the largest t a hit can have is the value below it, 0x7F7FFFFE, and the
largest finite value itself is the miss: both are cases here."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K_INFINITY = 0x7F7FFFFF          # bits of pt_math.h kInfinity
DENORMAL_MIN = 0x00000001
ONE = 0x3F800000
LARGEST_HIT = 0x7F7FFFFE         # the largest t below kInfinity
NEG_ZERO = 0x80000000
NAN_PAYLOAD = 0x7FC12345
NEG_NAN_PAYLOAD = 0xFFA00001


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("prec") / "libprimary_record_shim.so"
    src = os.path.join(ROOT, "tests", "primary_record_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P = ctypes.c_void_p
    lib.prec_pack.argtypes = [P, P]
    lib.prec_pack.restype = None
    lib.prec_unpack.argtypes = [P, P]
    lib.prec_unpack.restype = None
    lib.prec_words.restype = ctypes.c_uint32
    lib.prec_miss_bits.restype = ctypes.c_uint32
    lib.prec_bytes.argtypes = [ctypes.c_uint64]
    lib.prec_bytes.restype = ctypes.c_uint64
    lib.prec_word.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    lib.prec_word.restype = ctypes.c_uint64
    return lib


def _roundtrip(shim, dir_, normal, t, material, front):
    src = np.array(list(dir_) + list(normal) + [t, material, 1 if front else 0], np.uint32)
    words = np.zeros(shim.prec_words(), np.uint32)
    shim.prec_pack(src.ctypes.data, words.ctypes.data)
    out = np.zeros(10, np.uint32)
    shim.prec_unpack(words.ctypes.data, out.ctypes.data)
    return src, words, out


def _f(x):
    return int(np.float32(x).view(np.uint32))


DIR = [_f(0.25), _f(-0.5), _f(0.8291562)]
NORMAL = [_f(0.0), _f(1.0), _f(0.0)]


def test_eight_words_and_the_miss_value(shim):
    assert shim.prec_words() == 8
    assert shim.prec_miss_bits() == K_INFINITY == _f(3.402823466e+38)


def test_pack_then_unpack_is_the_identity(shim):
    rng = np.random.default_rng(3)
    for _ in range(200):
        d = rng.integers(0, 2 ** 32, 3, dtype=np.uint64).tolist()
        n = rng.integers(0, 2 ** 32, 3, dtype=np.uint64).tolist()
        t = int(rng.integers(1, K_INFINITY))             # 0 < t < kInfinity as bits: every accepted t
        m = int(rng.integers(0, 2 ** 32))
        front = bool(rng.integers(0, 2))
        src, words, out = _roundtrip(shim, d, n, t, m, front)
        assert np.array_equal(out[:9], src)
        assert out[9] == 1                               # a hit


@pytest.mark.parametrize("front,t", list(itertools.product([True, False], [DENORMAL_MIN, ONE, LARGEST_HIT, K_INFINITY])))
def test_front_and_t(shim, front, t):
    """`front` rides in t's sign bit: both values with t the smallest denormal, 1.0, the largest t a hit can have and the
    largest finite value (kInfinity: t and front still come back as they went in; it reads as a miss)."""
    src, words, out = _roundtrip(shim, DIR, NORMAL, t, 5, front)
    assert out[6] == t and out[8] == (1 if front else 0)
    assert np.array_equal(out[:9], src)
    assert out[9] == (0 if t == K_INFINITY else 1)
    assert words[3] == (t | (0x80000000 if front else 0))


def test_miss(shim):
    """What a write frame stores for a miss (resolve_hit: t = kInfinity, front false, zero normal, material 0)."""
    src, words, out = _roundtrip(shim, DIR, [0, 0, 0], K_INFINITY, 0, False)
    assert out[9] == 0 and out[8] == 0
    assert out[6] == K_INFINITY
    assert np.array_equal(out[:3], np.array(DIR, np.uint32))      # the miss branch shades with the direction
    assert np.array_equal(out[3:6], np.zeros(3, np.uint32)) and out[7] == 0


@pytest.mark.parametrize("material", [0, 0xFFFFFFFF, 0x80000000, 0x00010000])
def test_material_is_a_full_word(shim, material):
    for front in (True, False):
        src, words, out = _roundtrip(shim, DIR, NORMAL, ONE, material, front)
        assert out[7] == material and words[7] == material
        assert out[6] == ONE and out[8] == (1 if front else 0)


@pytest.mark.parametrize("special", [NEG_ZERO, NAN_PAYLOAD, NEG_NAN_PAYLOAD])
@pytest.mark.parametrize("slot", range(3))
def test_normal_and_direction_keep_their_bits(shim, special, slot):
    """-0.0 and NaN payloads in a normal (and a direction) component come back bit for bit."""
    n, d = list(NORMAL), list(DIR)
    n[slot] = special
    d[(slot + 1) % 3] = special
    src, words, out = _roundtrip(shim, d, n, ONE, 1, True)
    assert np.array_equal(out[:9], src)
    assert np.array_equal(words[4:7], np.array(n, np.uint32))
    assert np.array_equal(words[0:3], np.array(d, np.uint32))


@pytest.mark.parametrize("w,h", [(70, 44), (1920, 1080), (8, 8), (1, 1)])
def test_layout_matches_the_allocation(shim, w, h):
    """Tile-major: entry (ty * tilesX + tx) * 64 + lane, 8 words each; the entries of a frame's tiles fill exactly what
    launch_megakernel allocates (primary_record_bytes of the tile count, partial tiles included), none overlapping, each
    16-byte aligned (two 16-byte accesses per lane), a wave's 64 one contiguous 2 KiB run."""
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    words = shim.prec_words()
    assert shim.prec_bytes(tiles) == tiles * 64 * 32
    assert shim.prec_word(0, 0) == 0
    for tile in {0, 1, tiles // 2, tiles - 1}:
        offs = [shim.prec_word(tile, lane) for lane in range(64)]
        assert offs == [tile * 64 * words + lane * words for lane in range(64)]
        assert all(o * 4 % 16 == 0 for o in offs)
        assert (offs[-1] + words - offs[0]) * 4 == 2048
    assert (shim.prec_word(tiles - 1, 63) + words) * 4 == shim.prec_bytes(tiles)
    # past 2^32 bytes the offsets stay 64-bit
    assert shim.prec_word(1 << 24, 1) == (1 << 24) * 512 + 8
    assert shim.prec_bytes(1 << 24) == (1 << 24) * 2048
