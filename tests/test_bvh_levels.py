"""The level-synchronous midpoint build on the CPU: wc-path-tracer_amd/csrc/bvh_midpoint.h -- the functions the kernels of
pt_bvh_build.hip call once per thread -- compiled with g++ through tests/bvh_levels_shim.cpp, which runs each step as a
loop, against wcpt_bvh_build byte for byte (nodes, node count, index permutation) on the cases of bvh_build_cases.py, in
three visiting orders of every step. Then the partition's closed form alone against the reference's loop, the refusals,
and the same under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program
(tests/bvh_levels_asan_driver.cpp). CPU only."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from wcpt._lib import NODE_DTYPE

import bvh_build_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_INDEX, NOT_FINITE = 1, 2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("bvhl") / "libbvh_levels_shim.so"
    src = os.path.join(ROOT, "tests", "bvh_levels_shim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o",
                    str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    lib.bvh_levels_build.argtypes = [vp, u32, vp, u32, vp, ctypes.POINTER(u32), ctypes.c_int]
    lib.bvh_levels_partition.argtypes = [vp, u32, vp, vp]
    lib.bvh_levels_partition.restype = None
    return lib


def build(shim, mesh, order=0, indices=None):
    pos = np.ascontiguousarray(mesh.positions, dtype=np.float32)
    idx = np.ascontiguousarray(mesh.indices if indices is None else indices, dtype=np.uint32).copy()
    nodes = np.zeros(max(1, 2 * (idx.size // 3)), dtype=NODE_DTYPE)
    used = ctypes.c_uint32(0xFFFFFFFF)
    rc = shim.bvh_levels_build(pos.ctypes.data, pos.shape[0], idx.ctypes.data, idx.size, nodes.ctypes.data,
                               ctypes.byref(used), order)
    return rc, idx, nodes, used.value


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_levels_equal_the_host_builder(shim, name, order):
    mesh, ref = cases.case(name)
    rc, idx, nodes, used = build(shim, mesh, order)
    assert rc == 0
    assert used == len(ref.nodes)
    assert np.array_equal(idx, ref.indices)
    assert nodes[:used].tobytes() == ref.nodes.tobytes()


def test_cases_are_what_they_claim():
    """The crafted inputs reach the paths they are named for, in the host builder's own tree."""
    for name, moved in (("all_right_rotation", True), ("all_left_no_move", False)):
        mesh, ref = cases.case(name)
        assert len(ref.nodes) == 1 and ref.nodes[0]["triangleCount"] == 15  # a leaf of more than two triangles
        assert (not np.array_equal(ref.indices, mesh.indices)) == moved
    _, ref = cases.case("all_right_rotation")
    assert ref.indices.reshape(-1, 3)[:, 0].tolist() == [3, 6, 9, 12, 0]  # rotated by one
    _, ref = cases.case("budget_chain")
    assert ref.depth() == 33
    fat = [n for n in ref.nodes if n["triangleCount"] > 6]
    assert len(fat) == 1 and fat[0]["triangleCount"] == 3 * (46 - 32)
    for a, b in cases.SEGMENT_SIZES:
        _, ref = cases.case(f"segments_{a}_{b}")
        assert cases.level_segments(ref, 1) == sorted((a, b))
    for name in ("signed_zero_a", "signed_zero_b"):
        mesh, ref = cases.case(name)
        x = mesh.positions[:, 0]
        assert (x[x == 0].view(np.uint32) == 0).any() and (x[x == 0].view(np.uint32) != 0).any()
        assert ref.nodes[0]["min"][0] == 0 and ref.nodes[0]["max"][1] == 0
    _, ref = cases.case("centroid_on_split")
    assert ref.nodes[0]["min"][0] == 0 and ref.nodes[0]["max"][0] == 4


def _partition(shim, flags):
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    closed = np.zeros(flags.size, np.uint32)
    loop = np.zeros(flags.size, np.uint32)
    shim.bvh_levels_partition(flags.ctypes.data, flags.size, closed.ctypes.data, loop.ctypes.data)
    return closed, loop


def test_closed_form_equals_the_loop_exhaustively_to_12(shim):
    for n in range(1, 13):
        for flags in itertools.product((0, 1), repeat=n):
            closed, loop = _partition(shim, flags)
            assert np.array_equal(closed, loop), flags


def test_closed_form_equals_the_loop_on_random_segments(shim):
    rng = np.random.default_rng(7)
    for _ in range(3000):
        n = int(rng.integers(1, 400))
        flags = rng.random(n) < rng.random()
        closed, loop = _partition(shim, flags)
        assert np.array_equal(closed, loop)
        assert sorted(closed.tolist()) == list(range(n))


def test_already_permuted_indices_give_the_host_builders_tree(shim):
    mesh, ref = cases.case("suzanita")
    again = cases.wscene.bvh_build(cases.wscene.HostMesh(mesh.positions, ref.indices))
    rc, idx, nodes, used = build(shim, mesh, indices=ref.indices)
    assert rc == 0 and used == len(again.nodes)
    assert np.array_equal(idx, again.indices) and nodes[:used].tobytes() == again.nodes.tobytes()


@pytest.mark.parametrize("what", ["index", "nan", "inf"])
def test_refusals_write_nothing(shim, what):
    mesh, _ = cases.case("tri7")
    pos, idx = mesh.positions.copy(), mesh.indices.copy()
    if what == "index":
        idx[10] = pos.shape[0]
    else:
        pos[int(idx[10]), 1] = np.nan if what == "nan" else -np.inf
    rc, out_idx, nodes, used = build(shim, cases.wscene.HostMesh(pos, idx))
    assert rc == (BAD_INDEX if what == "index" else NOT_FINITE)
    assert np.array_equal(out_idx, idx) and not nodes.tobytes().strip(b"\0") and used == 0xFFFFFFFF


def test_unreferenced_non_finite_vertex_is_accepted(shim):
    mesh, ref = cases.case("tri7")
    pos = np.vstack([mesh.positions, np.full((1, 3), np.nan, np.float32)])
    rc, idx, nodes, used = build(shim, cases.wscene.HostMesh(pos, mesh.indices))
    assert rc == 0 and nodes[:used].tobytes() == ref.nodes.tobytes()


def test_entry_point_fails_with_a_code_without_a_context():
    import wcpt
    used = ctypes.c_uint32(5)
    assert wcpt.lib.wcpt_bvh_build_device(None, 1, 3, 2, 3, 3, ctypes.byref(used)) == wcpt._lib.WCPT_ERROR_INVALID_HANDLE
    assert used.value == 5


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_levels_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "bvh_levels_asan_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "bvh_levels_asan_driver.cpp"),
           os.path.join(ROOT, "tests", "bvh_levels_shim.cpp"),
           os.path.join(ROOT, "wc-path-tracer_amd", "host", "wcpt_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "0 failed checks" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
