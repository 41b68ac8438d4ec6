"""The primary cache's key and rule on the CPU (wc-path-tracer_amd/csrc/primary_cache_key.h, compiled here with g++ from
the product header through tests/primary_cache_key_shim.cpp): every field the primary Intersect record depends on flips
the match; maxBounceCount, samples, renderedFramesCount and boxID do not; frame 0 never uses the cache."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import wcpt  # noqa: E402  (the SceneData layout; loads no GPU)

SD = wcpt._lib.SCENE_DATA_DTYPE
GEOM = ["W", "H", "y0", "rows", "row_shift", "row_gap", "spheres", "draws", "tri_records", "pair_records", "generation"]
NONE, WRITE, READ = 0, 1, 2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("pck") / "libprimary_cache_key_shim.so"
    src = os.path.join(ROOT, "tests", "primary_cache_key_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P = ctypes.c_void_p
    lib.pck_equal.argtypes = [P, P, P, P]
    lib.pck_equal.restype = ctypes.c_int
    lib.pck_decide.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P]
    lib.pck_decide.restype = ctypes.c_int
    lib.pck_scene_data_bytes.restype = ctypes.c_int
    assert lib.pck_scene_data_bytes() == SD.itemsize == 164
    return lib


def _base():
    rng = np.random.default_rng(11)
    sd = np.zeros(1, SD)
    sd["inverseProjection"] = rng.standard_normal(16).astype(np.float32)
    sd["inverseView"] = rng.standard_normal(16).astype(np.float32)
    sd["position"] = rng.standard_normal(3).astype(np.float32)
    sd["maxBounceCount"], sd["samples"], sd["sphereCount"], sd["drawCommandCount"] = 4, 1, 4, 1
    sd["renderedFramesCount"], sd["boxID"] = 100, 7
    geom = np.array([1920, 1080, 270, 270, 31, 0, 0x7F0000001000, 0x7F0000002000, 0x7F0000003000, 1, 42], np.uint64)
    return sd, geom


def _ptr(a):
    return a.ctypes.data


def _equal(shim, a, b):
    return bool(shim.pck_equal(_ptr(a[0]), _ptr(a[1]), _ptr(b[0]), _ptr(b[1])))


def _decide(shim, stored, cur, enabled=1, valid=1):
    return shim.pck_decide(enabled, valid, _ptr(stored[0]), _ptr(stored[1]), _ptr(cur[0]), _ptr(cur[1]))


def test_equal_keys_match(shim):
    assert _equal(shim, _base(), _base())
    assert _decide(shim, _base(), _base()) == READ


@pytest.mark.parametrize("field,index", [("inverseProjection", i) for i in range(16)] +
                         [("inverseView", i) for i in range(16)] + [("position", i) for i in range(3)])
def test_every_camera_word_flips_the_match(shim, field, index):
    a, b = _base(), _base()
    w = b[0][field].view(np.uint32).reshape(-1)
    w[index] ^= 1                                   # one ulp
    assert not _equal(shim, a, b)
    assert _decide(shim, a, b) == WRITE


def test_camera_compares_bit_patterns(shim):
    """-0.0 against +0.0 and two NaN payloads are changes: the key compares bytes, as the issue asks."""
    a, b = _base(), _base()
    a[0]["position"][0, 0] = 0.0
    b[0]["position"][0, 0] = -0.0
    assert not _equal(shim, a, b)
    a[0]["position"].view(np.uint32)[0, 0] = 0x7FC00000
    b[0]["position"].view(np.uint32)[0, 0] = 0x7FC00000
    assert _equal(shim, a, b)                       # the same NaN bits match (memcmp, not ==)


@pytest.mark.parametrize("field", ["sphereCount", "drawCommandCount"])
def test_counts_flip_the_match(shim, field):
    a, b = _base(), _base()
    b[0][field] += 1
    assert not _equal(shim, a, b)
    assert _decide(shim, a, b) == WRITE


@pytest.mark.parametrize("name", GEOM)
def test_every_geometry_field_flips_the_match(shim, name):
    a, b = _base(), _base()
    i = GEOM.index(name)
    b[1][i] = 0 if name == "pair_records" else b[1][i] + np.uint64(1)
    assert not _equal(shim, a, b)
    assert _decide(shim, a, b) == WRITE


@pytest.mark.parametrize("name", ["spheres", "draws", "tri_records", "generation"])
def test_high_address_bits_count(shim, name):
    a, b = _base(), _base()
    b[1][GEOM.index(name)] ^= np.uint64(1 << 40)
    assert not _equal(shim, a, b)


@pytest.mark.parametrize("field,value", [("maxBounceCount", 0), ("samples", 4), ("renderedFramesCount", 299),
                                         ("boxID", 0)])
def test_fields_outside_the_key(shim, field, value):
    a, b = _base(), _base()
    b[0][field] = value
    assert _equal(shim, a, b)
    assert _decide(shim, a, b) == READ


def test_rule(shim):
    a, b = _base(), _base()
    assert _decide(shim, a, b, valid=0) == WRITE            # nothing stored yet
    assert _decide(shim, a, b, enabled=0) == NONE           # the option off, or a counting run
    b[0]["renderedFramesCount"] = 0
    assert _decide(shim, a, b) == NONE                      # frame 0 renders plainly whatever is stored
    assert _decide(shim, a, b, valid=0) == NONE
