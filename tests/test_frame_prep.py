"""Frame preparation's rules on the CPU (wc-path-tracer_amd/csrc/frame_prep.h, compiled here with g++ from the product
header through tests/frame_prep_shim.cpp -- the functions the runtime's prepare_tri_records calls per draw and per
frame): the record layout, a draw's table words, the argument check and the frame plan, on the repository's own scenes
and at every boundary of the rules. The expected values are written out here, from the table contract's description,
not read back from the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from wcpt import scene as wscene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEGAKERNEL, AUTO, WAVEFRONT = 0, 1, 2                      # wcpt.h WCPT_KERNEL_*
PACKED, INDEX24, SMALL, LEAFREC, TINY = 1, 2, 4, 8, 16     # table word 3
BIG_LEAF, OFF_RECORDS, TINY_TREE = 1, 2, 4                 # the leaf scan's bits
UNKNOWN = 0xFFFFFFFFFFFFFFFF                               # node count of a BVH buffer the context does not know
ALL_VERTS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def fp(tmp_path_factory):
    out = tmp_path_factory.mktemp("fp") / "libframe_prep_shim.so"
    src = os.path.join(ROOT, "tests", "frame_prep_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    i, u32, u64, p = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.fp_constants.argtypes = [p]
    lib.fp_record_layout.argtypes = [u32, p]
    lib.fp_vertex_bound.argtypes = [i, u64]
    lib.fp_vertex_bound.restype = u32
    lib.fp_bvh_node_count.argtypes = [i, u64]
    lib.fp_bvh_node_count.restype = u64
    lib.fp_leaf_estimate.argtypes = [i, u64, u32]
    lib.fp_leaf_estimate.restype = u64
    lib.fp_needs_scan.argtypes = [i, i, u64, u32]
    lib.fp_draw_words.argtypes = [i, i, u64, u32, u32, i, u32, p]
    lib.fp_check_draw_args.argtypes = [u32, u64, u64, i, u64]
    lib.fp_frame_plan.argtypes = [u32, u64, u64, u64, u64, u64, i, i, p]
    lib.fp_tiny_leaves.argtypes = [p, u64, u32]
    lib.fp_tiny_leaves.restype = u32
    return lib


def _layout(fp, ntri):
    out = (ctypes.c_uint64 * 4)()
    fp.fp_record_layout(ntri, out)
    return tuple(int(v) for v in out)


def _words(fp, index_count, nodes, scan=0, packed=1, cache=1, tiny=-1, nvert=ALL_VERTS):
    """(word 2, flags, vertex bound) of a draw"""
    out = (ctypes.c_uint64 * 2)()
    fp.fp_draw_words(packed, cache, nodes, index_count, scan, tiny, nvert, out)
    return int(out[0]), int(out[1]) & 0xFFFFFFFF, int(out[1]) >> 32


def _plan(fp, n, word2, flags, tris_all, leaves_all, tris_max, pair=-1, kernel=AUTO):
    out = (ctypes.c_uint64 * 6)()
    fp.fp_frame_plan(n, word2, flags, tris_all, leaves_all, tris_max, pair, kernel, out)
    return dict(pair_records=bool(out[0]), wf_fast=bool(out[1]), tiny_tree=bool(out[2]), triangles=int(out[3]),
                kernel_run=int(out[4]), want_primary=bool(out[5]))


def _scan(fp, bvh):
    """what the device scan reports of a mesh's BVH, from its host nodes"""
    lim3, bits = int(bvh.indices.size), 0
    for nd in bvh.nodes:
        first, count = int(nd["leftNodeOrTriangleIndex"]), int(nd["triangleCount"])
        if count == 0:
            continue
        if count >= 255:
            bits |= BIG_LEAF
        if first % 3 or first + count > lim3:
            bits |= OFF_RECORDS
    nodes = np.ascontiguousarray(bvh.nodes)
    if fp.fp_tiny_leaves(nodes.ctypes.data, len(nodes), lim3):
        bits |= TINY_TREE
    return bits


def _prepare(fp, meshes, pair=-1, kernel=AUTO, cache=1, tiny=-1):
    """One frame's preparation of a scene's meshes, every buffer uploaded whole (as wcpt.DeviceScene does): the per-draw
    words and the plan."""
    tris_all = leaves_all = tris_max = 0
    words = []
    for m in meshes:
        ic, nbytes = int(m.indices.size), 32 * len(m.nodes)
        nodes = fp.fp_bvh_node_count(1, nbytes)
        scan = _scan(fp, m) if fp.fp_needs_scan(1, cache, nodes, ic) else 0
        words.append(_words(fp, ic, nodes, scan, cache=cache, tiny=tiny, nvert=fp.fp_vertex_bound(1, m.positions.nbytes)))
        tris_all += ic // 3
        tris_max = max(tris_max, ic // 3)
        leaves_all += fp.fp_leaf_estimate(1, nbytes, ic // 3)
    w0 = words[0] if words else (0, 0, 0)
    return words, _plan(fp, len(meshes), w0[0], w0[1] | w0[2] << 32, tris_all, leaves_all, tris_max, pair, kernel)


def test_the_contract_is_the_documented_one(fp):
    out = (ctypes.c_uint64 * 20)()
    fp.fp_constants(out)
    assert [int(v) for v in out] == [5, 0, 1, 2, 3, 4, PACKED, INDEX24, SMALL, LEAFREC, TINY, BIG_LEAF, OFF_RECORDS,
                                     TINY_TREE, 48, 80, 112, 1 << 26, 4, UNKNOWN]


# ---- the repository's scenes -----------------------------------------------------------------------------------------
def test_cornell_takes_pair_records_the_megakernel_and_every_flag(fp):
    meshes = wscene.generate("cornell").meshes
    assert len(meshes) == 1 and meshes[0].indices.size == 102 and len(meshes[0].nodes) == 3
    assert fp.fp_leaf_estimate(1, 3 * 32, 34) == 2            # 17 triangles per leaf
    words, plan = _prepare(fp, meshes)
    assert words[0][0] == 34 | 3 << 32
    assert words[0][1] == PACKED | INDEX24 | SMALL | LEAFREC | TINY
    assert words[0][2] == meshes[0].positions.size // 3
    assert plan == dict(pair_records=True, wf_fast=True, tiny_tree=True, triangles=34, kernel_run=MEGAKERNEL,
                        want_primary=True)


def test_the_atrium_takes_single_records_and_the_wavefront_kernel(fp):
    meshes = wscene.generate("atrium").meshes
    ntri = sum(m.indices.size // 3 for m in meshes)
    leaves = sum((len(m.nodes) + 1) // 2 for m in meshes)
    assert ntri < 4 * leaves                                   # thin leaves
    words, plan = _prepare(fp, meshes)
    assert not plan["pair_records"] and plan["kernel_run"] == WAVEFRONT and not plan["want_primary"]
    assert plan["triangles"] == ntri and not plan["tiny_tree"]
    assert all(w[1] & TINY == 0 for w in words)
    # an explicit kernel option overrides the rule, and pair records stay the rule's
    assert _prepare(fp, meshes, kernel=MEGAKERNEL)[1]["kernel_run"] == MEGAKERNEL
    assert not _prepare(fp, meshes, kernel=MEGAKERNEL)[1]["want_primary"]
    forced = _prepare(fp, meshes, pair=1)[1]
    assert forced["pair_records"] and forced["kernel_run"] == MEGAKERNEL and forced["want_primary"]
    assert _prepare(fp, wscene.generate("cornell").meshes, kernel=WAVEFRONT)[1] == dict(
        pair_records=True, wf_fast=True, tiny_tree=True, triangles=34, kernel_run=WAVEFRONT, want_primary=False)


# ---- a draw's words --------------------------------------------------------------------------------------------------
def test_index_count_boundary(fp):
    below, at = (1 << 24) - 1, 1 << 24
    assert _words(fp, below, 3)[:2] == (below // 3 | 3 << 32, PACKED | INDEX24 | SMALL | LEAFREC)
    assert _words(fp, at, 3)[:2] == (at // 3, 0)               # no packed refs: no node count in word 2 either
    assert fp.fp_needs_scan(1, 1, 3, below) == 1 and fp.fp_needs_scan(1, 1, 3, at) == 0


def test_node_count_boundary(fp):
    below, at = (1 << 24) - 1, 1 << 24
    assert _words(fp, 102, below)[:2] == (34 | below << 32, PACKED | INDEX24 | SMALL | LEAFREC)
    assert _words(fp, 102, at)[:2] == (34, INDEX24)
    assert _words(fp, 102, UNKNOWN)[:2] == (34, INDEX24)
    assert [fp.fp_needs_scan(1, 1, n, 102) for n in (below, at, UNKNOWN)] == [1, 0, 0]
    assert fp.fp_bvh_node_count(0, 1 << 40) == UNKNOWN
    assert fp.fp_bvh_node_count(1, 95) == 2 and fp.fp_bvh_node_count(1, 96) == 3


def test_packed_refs_option_off(fp):
    assert _words(fp, 102, 3, scan=TINY_TREE, packed=0)[:2] == (34, INDEX24)
    assert fp.fp_needs_scan(0, 1, 3, 102) == 0


def test_cache_off_never_scans_and_never_sets_the_scanned_flags(fp):
    for scan in range(8):
        for tiny in (-1, 0, 1):
            assert _words(fp, 102, 3, scan=scan, cache=0, tiny=tiny)[:2] == (34 | 3 << 32, PACKED | INDEX24)
    assert fp.fp_needs_scan(1, 0, 3, 102) == 0


def test_each_scan_bit_alone(fp):
    base = PACKED | INDEX24
    assert _words(fp, 102, 3, scan=0)[1] == base | SMALL | LEAFREC
    assert _words(fp, 102, 3, scan=BIG_LEAF)[1] == base | LEAFREC
    assert _words(fp, 102, 3, scan=OFF_RECORDS)[1] == base | SMALL
    assert _words(fp, 102, 3, scan=TINY_TREE)[1] == base | SMALL | LEAFREC | TINY
    assert _words(fp, 102, 3, scan=BIG_LEAF | OFF_RECORDS)[1] == base


def test_tiny_option(fp):
    for option, expect in ((-1, TINY), (0, 0), (1, TINY)):
        assert _words(fp, 102, 3, scan=TINY_TREE, tiny=option)[1] & TINY == expect
        assert _words(fp, 102, 3, scan=0, tiny=option)[1] & TINY == 0


def test_vertex_bound(fp):
    assert fp.fp_vertex_bound(0, 0) == ALL_VERTS and fp.fp_vertex_bound(0, 120) == ALL_VERTS
    assert [fp.fp_vertex_bound(1, b) for b in (0, 11, 12, 35, 36)] == [0, 0, 1, 2, 3]
    assert fp.fp_vertex_bound(1, 12 * 0xFFFFFFFE) == 0xFFFFFFFE
    assert fp.fp_vertex_bound(1, 12 * 0xFFFFFFFF) == ALL_VERTS and fp.fp_vertex_bound(1, 1 << 60) == ALL_VERTS
    assert _words(fp, 102, 3, nvert=24) == (34 | 3 << 32, PACKED | INDEX24 | SMALL | LEAFREC, 24)


def test_leaf_estimate_takes_the_whole_buffer(fp):
    assert [fp.fp_leaf_estimate(1, 32 * n, 1000) for n in (0, 1, 2, 3, 4, 5)] == [0, 1, 1, 2, 2, 3]
    assert fp.fp_leaf_estimate(0, 32 * 99, 1000) == 1000       # unknown buffer: one triangle per leaf


# ---- the frame plan ----------------------------------------------------------------------------------------------------
ALL = PACKED | INDEX24 | SMALL | LEAFREC | TINY


def test_largest_draw_boundary_with_pairs_forced(fp):
    at, above = 1 << 26, (1 << 26) + 1
    assert _plan(fp, 1, at, INDEX24, at, 1, at, pair=1)["pair_records"]
    assert not _plan(fp, 1, above, INDEX24, above, 1, above, pair=1)["pair_records"]
    # the largest draw decides, not the sum
    assert _plan(fp, 2, at, INDEX24, 2 * at, 2, at, pair=1)["pair_records"]
    assert not _plan(fp, 2, 5, INDEX24, above + 5, 2, above, pair=1)["pair_records"]
    assert _plan(fp, 1, above, INDEX24, above, 1, above, pair=1)["kernel_run"] == WAVEFRONT


def test_triangles_per_leaf_boundary(fp):
    for leaves in (1, 2, 1000):
        assert _plan(fp, 1, 4 * leaves, INDEX24, 4 * leaves, leaves, 4 * leaves)["pair_records"]
        assert not _plan(fp, 1, 4 * leaves - 1, INDEX24, 4 * leaves - 1, leaves, 4 * leaves - 1)["pair_records"]
    assert not _plan(fp, 1, 0, INDEX24, 0, 0, 0)["pair_records"]                  # no leaves at all
    assert not _plan(fp, 1, 40, INDEX24, 40, 1, 40, pair=0)["pair_records"]       # singles forced
    assert _plan(fp, 1, 1, INDEX24, 1, 1, 1, pair=1)["pair_records"]              # pairs forced


def test_wf_fast_needs_every_layout_flag_and_a_node_count(fp):
    fast = PACKED | INDEX24 | SMALL | LEAFREC
    assert _plan(fp, 1, 34 | 3 << 32, fast, 34, 2, 34)["wf_fast"]
    assert _plan(fp, 1, 34 | 3 << 32, fast | 24 << 32, 34, 2, 34)["wf_fast"]      # the vertex bound is not a flag
    assert not _plan(fp, 1, 34, fast, 34, 2, 34)["wf_fast"]                       # word 2 without a node count
    for missing in (PACKED, INDEX24, SMALL, LEAFREC):
        assert not _plan(fp, 1, 34 | 3 << 32, fast & ~missing, 34, 2, 34)["wf_fast"]
    assert not _plan(fp, 1, 34 | 3 << 32, fast, 34, 2, 34)["tiny_tree"]
    assert _plan(fp, 1, 34 | 3 << 32, TINY, 34, 2, 34)["tiny_tree"]


def test_two_draws_take_neither_fast_path(fp):
    for flags in (ALL, ALL | ALL_VERTS << 32, TINY, 0):
        plan = _plan(fp, 2, 34 | 3 << 32, flags, 68, 4, 34)
        assert not plan["wf_fast"] and not plan["tiny_tree"]
        assert plan["pair_records"] and plan["kernel_run"] == MEGAKERNEL and plan["triangles"] == 68
    words, plan = _prepare(fp, wscene.generate("cornell").meshes * 2)
    assert [w[1] for w in words] == [ALL, ALL]
    assert plan == dict(pair_records=True, wf_fast=False, tiny_tree=False, triangles=68, kernel_run=MEGAKERNEL,
                        want_primary=True)


@pytest.mark.parametrize("pair", [-1, 0, 1])
def test_no_draws(fp, pair):
    none = dict(pair_records=False, wf_fast=False, tiny_tree=False, triangles=0, want_primary=False)
    assert _plan(fp, 0, 0, 0, 0, 0, 0, pair, AUTO) == dict(none, kernel_run=MEGAKERNEL)
    assert _plan(fp, 0, 0, 0, 0, 0, 0, pair, MEGAKERNEL) == dict(none, kernel_run=MEGAKERNEL)
    assert _plan(fp, 0, 0, 0, 0, 0, 0, pair, WAVEFRONT) == dict(none, kernel_run=WAVEFRONT)
    # whatever a stale table holds
    assert _plan(fp, 0, 34 | 3 << 32, ALL, 34, 2, 34, pair, AUTO) == dict(none, kernel_run=MEGAKERNEL)
    assert _prepare(fp, [], pair=pair)[1] == dict(none, kernel_run=MEGAKERNEL)


def test_an_explicit_kernel_overrides_the_rule(fp):
    fat = (1, 34 | 3 << 32, ALL, 34, 2, 34)
    thin = (1, 34 | 35 << 32, ALL & ~TINY, 34, 18, 34)
    assert _plan(fp, *fat)["kernel_run"] == MEGAKERNEL and _plan(fp, *thin)["kernel_run"] == WAVEFRONT
    for args in (fat, thin):
        for k in (MEGAKERNEL, WAVEFRONT):
            plan = _plan(fp, *args, kernel=k)
            assert plan["kernel_run"] == k
            assert plan["pair_records"] == (args is fat)
            assert plan["want_primary"] == (args is fat and k == MEGAKERNEL)


# ---- record layout and the argument check ------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [0, 1, 2, 5, 6, 1 << 26])
def test_record_layout(fp, ntri):
    singles = (ntri * 48 + 255) & ~255
    assert _layout(fp, ntri) == (singles, singles + (ntri // 2 + 1) * 80, (ntri + 1) // 2, ((ntri + 1) // 2) * 112)


def test_draw_argument_check(fp):
    OK, PAST, NULL = 0, 1, 2
    vb, ib = 0x7000_0000_0020, 0x7000_0001_0020
    assert fp.fp_check_draw_args(30, vb, ib, 1, 120) == OK          # 10 triangles exactly fill 120 bytes
    assert fp.fp_check_draw_args(31, vb, ib, 1, 120) == OK          # a count that is no multiple of 3: 10 triangles
    assert fp.fp_check_draw_args(33, vb, ib, 1, 120) == PAST
    assert fp.fp_check_draw_args(33, vb, ib, 1, 131) == PAST and fp.fp_check_draw_args(33, vb, ib, 1, 132) == OK
    # an offset into the buffer: the bytes from the draw's address to the buffer's end count
    size, off = 240, 120
    assert fp.fp_check_draw_args(30, vb, ib + off, 1, size - off) == OK
    assert fp.fp_check_draw_args(33, vb, ib + off, 1, size - off) == PAST
    assert fp.fp_check_draw_args(60, vb, ib, 1, size) == OK
    # a buffer the context does not know bounds nothing
    assert fp.fp_check_draw_args(0xFFFFFFFF, vb, ib, 0, 0) == OK
    for v, i in ((0, ib), (vb, 0), (0, 0)):
        assert fp.fp_check_draw_args(0, v, i, 0, 0) == OK           # no triangle: nothing is read
        assert fp.fp_check_draw_args(2, v, i, 0, 0) == OK
        assert fp.fp_check_draw_args(3, v, i, 0, 0) == NULL         # one triangle
    assert fp.fp_check_draw_args(33, 0, ib, 1, 120) == PAST         # the bound is reported first
