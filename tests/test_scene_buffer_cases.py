"""What tests/test_gpu_scene_buffers.py leans on, proved on the CPU: the oracle's frame and counters do not depend on
where a tree's nodes and a leaf's indices lie in their buffers (so the compact twin of a tree spread over 2^24 nodes is
its reference); every case reaches the layout it is named for by the product's own rules (frame_prep.h and
mk_tiny_rule.h through their shims); every leaf placed at an extreme position is visible; the fat leaf is fat."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from wcpt import scene as wscene

import scene_buffer_cases as sbc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED, INDEX24, TINY = 1, 2, 16
ALL_VERTS = 0xFFFFFFFF


def _shim(tmp_path_factory, name):
    out = tmp_path_factory.mktemp(name) / f"lib{name}.so"
    src = os.path.join(ROOT, "tests", f"{name}.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    return ctypes.CDLL(str(out))


@pytest.fixture(scope="module")
def fp(tmp_path_factory):
    lib = _shim(tmp_path_factory, "frame_prep_shim")
    i, u32, u64, p = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.fp_vertex_bound.argtypes = [i, u64]
    lib.fp_vertex_bound.restype = u32
    lib.fp_bvh_node_count.argtypes = [i, u64]
    lib.fp_bvh_node_count.restype = u64
    lib.fp_draw_words.argtypes = [i, i, u64, u32, u32, i, u32, p]
    lib.fp_leaf_estimate.argtypes = [i, u64, u32]
    lib.fp_leaf_estimate.restype = u64
    lib.fp_frame_plan.argtypes = [u32, u64, u64, u64, u64, u64, i, i, p]
    return lib


@pytest.fixture(scope="module")
def mkt(tmp_path_factory):
    lib = _shim(tmp_path_factory, "mk_tiny_rule_shim")
    lib.mkt_leaves.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
    lib.mkt_leaves.restype = ctypes.c_uint32
    return lib


def flags_of(fp, node_bytes_left, index_count, scan=0):
    """the table flags of a draw whose BVH address has node_bytes_left bytes of a context buffer behind it"""
    out = (ctypes.c_uint64 * 2)()
    fp.fp_draw_words(1, 1, fp.fp_bvh_node_count(1, node_bytes_left), index_count, scan, -1, ALL_VERTS, out)
    return int(out[1]) & 0xFFFFFFFF, int(out[0]) >> 32


def _scene(mesh):
    s = wscene.generate("default")
    s.meshes = [wscene.HostBVH(*m) for m in (mesh if isinstance(mesh, list) else [mesh])]
    return s


def _render(mesh, frames=1):
    s, acc, cnt = _scene(mesh), None, None
    for f in range(frames):
        acc, cnt = oracle.render_scene(s, sbc.W, sbc.H, max_bounce=sbc.BOUNCES, frame=f, image=acc, threads=4)
    return acc, cnt


# ---- renumbering invariance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", sbc.small_twins(), ids=lambda t: t.name)
def test_the_oracle_does_not_see_node_numbers_or_index_positions(tree):
    """children at nodes 5 and 6 of an 8-node buffer whose other nodes are 0xA5 bytes, leaves a few hundred index
    positions apart with filler indices between them: the bits and the counters of the compact twin"""
    assert tree.left == 5 and tree.node_count == 8
    nodes = tree.node_buffer()
    assert all(nodes[k].tobytes() == bytes([sbc.FILL]) * 32 for k in (1, 2, 3, 4, 7))
    spread, cs = _render(tree.spread(), frames=2)
    compact, cc = _render(tree.compact(), frames=2)
    assert np.array_equal(spread.view(np.uint32), compact.view(np.uint32))
    assert cs == cc and cs["triangle_tests"] > 0 and cs["interior_visits"] > 0


def test_a_filler_index_other_than_zero_changes_nothing():
    tree = sbc.small_twins()[0]
    a, ca = _render(tree.spread(filler=0))
    b, cb = _render(tree.spread(filler=5))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ca == cb


# ---- each large case reaches the layout it is named for ----------------------------------------------------------------
def test_the_large_cases_cross_the_thresholds_by_the_rule(fp):
    cases = sbc.big_cases()
    assert set(cases) == {"below", "nodes_at", "nodes_above", "index_at", "index_above", "both_above"}
    seen = set()
    for name, (tree, expect) in cases.items():
        # the draw's BVH address is (BIG_NODES - node_count) nodes into the one node buffer
        left_bytes = 32 * sbc.BIG_NODES - 32 * (sbc.BIG_NODES - tree.node_count)
        flags, nodes_word = flags_of(fp, left_bytes, tree.index_count)
        assert flags & (PACKED | INDEX24) == expect, name
        assert nodes_word == (tree.node_count if expect & PACKED else 0), name
        assert tree.left == tree.node_count - 2                      # the children are the draw's last two nodes
        assert tree.index_count <= sbc.BIG_INDICES
        seen.add((tree.node_count, tree.index_count))
    assert {n for n, _ in seen} == {sbc.N24 - 1, sbc.N24, sbc.N24 + 1}
    assert {i for _, i in seen} == {sbc.N24 - 1, sbc.N24 + 2, sbc.BIG_INDICES}
    # one below the node threshold and the index threshold: packed and 24-bit; at either: not packed
    assert flags_of(fp, 32 * (sbc.N24 - 1), sbc.N24 - 1)[0] & 3 == PACKED | INDEX24
    assert flags_of(fp, 32 * sbc.N24, sbc.N24 - 1)[0] & 3 == INDEX24
    assert flags_of(fp, 32 * (sbc.N24 - 1), sbc.N24)[0] & 3 == 0


def test_the_extreme_positions_are_the_largest_the_packed_forms_hold():
    below = sbc.big_cases()["below"][0]
    assert below.node_count == sbc.N24 - 1 and below.left + 1 == sbc.N24 - 2       # (node_index << 8) | 255
    assert ((below.left + 1) << 8 | 255) < 1 << 32
    first, n = below.firsts[0], below.leaf_indices[0].size
    assert first % 3 == 0 and first + n == below.index_count == sbc.N24 - 1      # ends at the draw's last triangle
    assert n < 255 and (first << 8 | n) < 1 << 32                                 # (left << 8) | count
    cross = sbc.big_cases()["index_above"][0]
    assert cross.firsts[0] < sbc.N24 < cross.firsts[0] + cross.leaf_indices[0].size
    assert cross.firsts[1] > sbc.N24 and cross.firsts[1] + cross.leaf_indices[1].size == sbc.BIG_INDICES
    assert all(f % 3 == 0 for f in cross.firsts)
    # with the first count past 2^24 both leaves lie off the derived records (the index path)
    at = sbc.big_cases()["index_at"][0]
    assert all(f + ix.size > at.index_count for f, ix in zip(at.firsts, at.leaf_indices))
    # both parities of the first triangle: a pair-record leaf starts in slot 0 and in slot 1
    starts = {(f // 3) % 2 for t in (below, cross) for f in t.firsts}
    assert starts == {0, 1}
    assert [(f // 3) % 2 for f in below.firsts] == [0, 1] and [(f // 3) % 2 for f in cross.firsts] == [1, 0]


def test_the_fat_leaf_is_fat():
    below = sbc.big_cases()["below"][0]
    nodes = below.sparse_nodes()
    assert nodes[2]["triangleCount"] >= 255 and nodes[1]["triangleCount"] < 255
    assert nodes[2]["triangleCount"] == below.leaf_indices[1].size == 3 * sbc.T_FAT


def test_the_one_index_buffer_holds_every_large_tree():
    cases = sbc.big_cases()
    buf = sbc.big_index_buffer(cases)
    assert buf.size == sbc.BIG_INDICES and buf.nbytes > 64 << 20
    named = np.zeros(buf.size, bool)
    for tree, _ in cases.values():
        for f, ix in zip(tree.firsts, tree.leaf_indices):
            assert np.array_equal(buf[f:f + ix.size], ix)
            named[f:f + ix.size] = True
    assert not buf[~named].any()                                      # filler 0 everywhere else
    pos, base = sbc.big_positions(cases)
    for name, (tree, _) in cases.items():
        assert np.array_equal(pos[base[name]:base[name] + len(tree.positions)], tree.positions)


# ---- every extreme leaf is visible -------------------------------------------------------------------------------------
def _trees_under_test():
    big = sbc.big_cases()
    return [big["below"][0], big["index_above"][0], sbc.tiny_arena_tree()]


@pytest.mark.parametrize("tree", _trees_under_test(), ids=lambda t: t.name)
@pytest.mark.parametrize("leaf", [0, 1])
def test_every_extreme_leaf_is_visible(tree, leaf):
    """a kernel that never reached the leaf would not render the oracle's frame"""
    full, _ = _render(tree.compact())
    without, _ = _render(tree.compact(drop=leaf))
    assert (full.view(np.uint32) != without.view(np.uint32)).any()


def test_both_child_orders_occur():
    """the leaves' boxes overlap, and of the primary rays inside the root's box many enter the left child first and many
    the right (so either leaf is the deferred one, whose stack entry is the form under test), also within one wave"""
    from test_gpu_tiny_tree import _primary_orders
    for tree in _trees_under_test():
        n = tree.sparse_nodes()
        assert (n[1]["min"] < n[2]["max"]).all() and (n[2]["min"] < n[1]["max"]).all()
        tiles = _primary_orders(_scene(tree.compact()), sbc.W, sbc.H)
        assert sum(a for a, _ in tiles) > 200 and sum(b for _, b in tiles) > 200, tiles
        assert any(a > 0 and b > 0 for a, b in tiles)


# ---- the arena --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_records", [True, False])
def test_the_arena_tiny_tree_is_tiny_by_the_rule(mkt, fp, on_records):
    """root at node 0, leaves at nodes 4 and 5 of an 8-node sub-allocation, the arena's bytes behind it read as nodes"""
    tree = sbc.tiny_arena_tree(on_records)
    pos, idx, nodes = tree.spread()
    assert tree.left == 4 and len(nodes) == 8
    s = wscene.generate("default")
    arrays = dict(materials=s.materials, spheres=s.spheres, vertices=pos, indices=idx, nodes=nodes)
    for order in (sbc.ORDER_NODES_LAST, sbc.ORDER_NODES_FIRST):
        buf, off, total = sbc.arena_bytes(arrays, order)
        assert off["nodes"] % 16 == 0 and all(o % 4 == 0 for o in off.values())
        view = np.ascontiguousarray(buf[off["nodes"]:])
        n = fp.fp_bvh_node_count(1, total - off["nodes"])
        assert n == (total - off["nodes"]) // 32 and n >= 8
        lim3 = 3 * (tree.index_count // 3)
        assert mkt.mkt_leaves(view.ctypes.data, n, lim3) == (2 if on_records else 0)
        if order is sbc.ORDER_NODES_LAST:
            assert n == 8                                             # the scan sees exactly the tree's sub-allocation
    # the oracle's frame is the same either way: it never reads indexCount
    assert np.array_equal(_render(sbc.tiny_arena_tree(True).compact())[0], _render(tree.spread())[0])


def test_arena_layout_keeps_the_gaps_filled():
    s = wscene.generate("cornell")
    m = s.meshes[0]
    arrays = dict(materials=s.materials, spheres=s.spheres, vertices=m.positions, indices=m.indices, nodes=m.nodes)
    for order in (sbc.ORDER_NODES_LAST, sbc.ORDER_NODES_FIRST):
        buf, off, total = sbc.arena_bytes(arrays, order)
        used = np.zeros(total, bool)
        for name, a in arrays.items():
            assert not used[off[name]:off[name] + a.nbytes].any()
            used[off[name]:off[name] + a.nbytes] = True
            assert buf[off[name]:off[name] + a.nbytes].tobytes() == np.ascontiguousarray(a).tobytes()
        used[off["draws"]:off["draws"] + 32] = True
        assert (buf[~used] == sbc.FILL).all() and (~used).sum() >= 64 * 5
        assert off[order[0]] >= 64                                    # no sub-allocation at the arena's start
    last = sbc.arena_bytes(arrays, sbc.ORDER_NODES_LAST)
    assert last[1]["nodes"] + m.nodes.nbytes == last[2]               # nodes last: the arena ends with the tree


def test_the_triangle_with_the_index_past_the_bound_is_visible():
    pos, idx, nodes, bad = sbc.one_leaf_mesh()
    full, _ = _render((pos, idx, nodes))
    pos_nan, idx_nan = sbc.with_nan_vertex(pos, idx, bad)
    without, _ = _render((pos_nan, idx_nan, nodes))
    assert (full.view(np.uint32) != without.view(np.uint32)).any(axis=2).sum() > 50


def test_the_vertex_bound_counts_from_the_offset(fp):
    assert fp.fp_vertex_bound(1, 1200 - 240) == 80 and fp.fp_vertex_bound(1, 1200) == 100


def test_two_shared_meshes_are_two_valid_draws():
    a, b = sbc.two_shared_meshes()
    for pos, idx, nodes in (a, b):
        assert idx.max() < len(pos) and len(nodes) == 3 and idx.size == 129
    both, cb = _render([a, b])
    only_a, _ = _render([a])
    only_b, _ = _render([b])
    assert (both != only_a).any() and (both != only_b).any()          # each mesh is visible
    assert cb["draw_fetches"] == 2 * cb["segments"]
