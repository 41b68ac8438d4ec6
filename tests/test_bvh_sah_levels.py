"""The level-synchronous binned-SAH build on the CPU: wc-path-tracer_amd/csrc/bvh_sah.h -- the functions the kernels of
pt_bvh_sah.hip call once per thread -- compiled with g++ through tests/bvh_sah_levels_shim.cpp, which runs each step as a
loop, against wcpt_bvh_build_sah byte for byte (nodes, node count, index permutation) on the cases of bvh_sah_cases.py,
in three visiting orders of every step. Then the refusals, and the same under AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program (tests/bvh_sah_asan_driver.cpp). CPU only."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from wcpt._lib import NODE_DTYPE

import bvh_sah_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("bvhsah") / "libbvh_sah_levels_shim.so"
    src = os.path.join(ROOT, "tests", "bvh_sah_levels_shim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o",
                    str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    lib.bvh_sah_levels_build.argtypes = [vp, u32, vp, u32, vp, ctypes.POINTER(u32), ctypes.c_int, ctypes.c_int]
    return lib


def build(shim, mesh, order=0, indices=None, private_spans=1):
    pos = np.ascontiguousarray(mesh.positions, dtype=np.float32)
    idx = np.ascontiguousarray(mesh.indices if indices is None else indices, dtype=np.uint32).copy()
    nodes = np.zeros(max(1, 2 * (idx.size // 3)), dtype=NODE_DTYPE)
    used = ctypes.c_uint32(0xFFFFFFFF)
    rc = shim.bvh_sah_levels_build(pos.ctypes.data, pos.shape[0], idx.ctypes.data, idx.size, nodes.ctypes.data,
                                   ctypes.byref(used), order, private_spans)
    return rc, idx, nodes, used.value


@pytest.mark.parametrize("private_spans", [0, 1])
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_levels_equal_the_host_builder(shim, name, order, private_spans):
    """private_spans: the bin step by global updates alone, or with spans of 1024 positions inside one node binned
    privately and merged (the kernel's second path): the bytes do not depend on the path"""
    mesh, ref = cases.case(name)
    rc, idx, nodes, used = build(shim, mesh, order, private_spans=private_spans)
    assert rc == 0
    assert used == len(ref.nodes)
    assert np.array_equal(idx, ref.indices)
    assert nodes[:used].tobytes() == ref.nodes.tobytes()


def test_cases_are_what_they_claim():
    cases.check_cases()


def test_already_permuted_indices_give_the_host_builders_tree(shim):
    mesh, ref = cases.case("suzanita")
    again = cases.wscene.bvh_build(cases.wscene.HostMesh(mesh.positions, ref.indices), "sah")
    rc, idx, nodes, used = build(shim, mesh, indices=ref.indices)
    assert rc == 0 and used == len(again.nodes)
    assert np.array_equal(idx, again.indices) and nodes[:used].tobytes() == again.nodes.tobytes()


@pytest.mark.parametrize("what", ["index", "nan", "inf", "centroid_overflow", "scale_not_finite", "infinite_extent",
                                  "no_finite_cost"])
def test_refusals_write_nothing(shim, what):
    mesh, status = cases.refusal_meshes()[what]
    rc, out_idx, nodes, used = build(shim, mesh)
    assert rc == status
    assert np.array_equal(out_idx, mesh.indices) and not nodes.tobytes().strip(b"\0") and used == 0xFFFFFFFF


def test_unreferenced_non_finite_vertex_is_accepted(shim):
    mesh, ref = cases.case("tri7")
    pos = np.vstack([mesh.positions, np.full((1, 3), np.nan, np.float32)])
    rc, idx, nodes, used = build(shim, cases.wscene.HostMesh(pos, mesh.indices))
    assert rc == 0 and nodes[:used].tobytes() == ref.nodes.tobytes()


def test_entry_point_fails_with_a_code_without_a_context():
    import wcpt
    used = ctypes.c_uint32(5)
    assert wcpt.lib.wcpt_bvh_build_sah_device(None, 1, 3, 2, 3, 3, ctypes.byref(used)) == wcpt._lib.WCPT_ERROR_INVALID_HANDLE
    assert used.value == 5


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_levels_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "bvh_sah_asan_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "bvh_sah_asan_driver.cpp"),
           os.path.join(ROOT, "tests", "bvh_sah_levels_shim.cpp"),
           os.path.join(ROOT, "wc-path-tracer_amd", "host", "wcpt_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "0 failed checks" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
