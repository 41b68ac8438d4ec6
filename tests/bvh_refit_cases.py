"""Trees and moves for the refit tests (test input, no product code). Shared by tests/test_bvh_refit.py (host) and
tests/test_gpu_bvh_refit.py (device): the builders' trees of bvh_build_cases.py and bvh_sah_cases.py, one hand-made tree,
seeded moves of the vertices, the inputs a refit refuses, and an independent numpy restatement of the rule."""
import functools

import numpy as np

from wcpt import scene as wscene
from wcpt._lib import NODE_DTYPE

import bvh_build_cases as midpoint_cases
import bvh_sah_cases as sah_cases

# bvh_refit.h's status bits
BAD_INDEX, BAD_CHILD, BAD_LEAF, BAD_PARENTS, NOT_FINITE = 1, 2, 4, 8, 16

BUILDERS = {"midpoint": midpoint_cases, "sah": sah_cases}
TREES = [(kind, name) for kind, mod in BUILDERS.items() for name in mod.CASES] + [("handmade", "handmade")]


@functools.lru_cache(maxsize=None)
def handmade():
    """Nine nodes, children after their parents but not in the builders' numbering (node 1's children are 5 and 6, node
    2's are 3 and 4, node 6's are 7 and 8); leaf 3 starts at the odd index 1 and holds 20 triangles; the indices 0 and
    67..69 belong to no leaf; vertices are shared between triangles."""
    rng = np.random.default_rng(77)
    pos = rng.uniform(-3.0, 3.0, (31, 3)).astype(np.float32)
    pos[5] = (0.0, -0.0, 1.0)
    idx = rng.integers(0, 31, 75).astype(np.uint32)
    nodes = np.zeros(9, NODE_DTYPE)
    for i, (left, count) in enumerate([(1, 0), (5, 0), (3, 0), (1, 60), (61, 3), (64, 6), (7, 0), (70, 3), (72, 3)]):
        nodes[i]["leftNodeOrTriangleIndex"], nodes[i]["triangleCount"] = left, count
    nodes["min"], nodes["max"] = 123.0, -123.0  # stale boxes: a refit must not depend on them
    return wscene.HostBVH(pos, idx, nodes)


@functools.lru_cache(maxsize=None)
def tree(kind, name):
    """the tree `name` of builder `kind` as its builder left it (shared, never modified by a test)"""
    if kind == "handmade":
        return handmade()
    return BUILDERS[kind].case(name)[1]


def moved(positions, seed, amount=0.5):
    """every coordinate moved by a seeded offset of up to `amount`"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    return (pos + rng.uniform(-amount, amount, pos.shape).astype(np.float32)).astype(np.float32)


def fold_zero(nodes):
    """a copy of `nodes` with -0 folded onto +0 in the six floats"""
    out = np.array(nodes, dtype=NODE_DTYPE, copy=True)
    for field in ("min", "max"):
        bits = out[field].view(np.uint32)
        bits[bits == 0x80000000] = 0
    return out


@functools.lru_cache(maxsize=None)
def host_refit(kind, name, move):
    """(positions, wcpt_bvh_refit's nodes) of tree (kind, name) under move None | a seed | "scale3": computed once"""
    bvh = tree(kind, name)
    pos = positions_for(bvh, move)
    return pos, wscene.bvh_refit(bvh, pos).nodes


def positions_for(bvh, move):
    if move is None:
        return np.ascontiguousarray(bvh.positions, np.float32).reshape(-1, 3)
    if move == "scale3":
        return (np.asarray(bvh.positions, np.float32).reshape(-1, 3) * np.float32(3.0)).astype(np.float32)
    return moved(bvh.positions, move)


def restated(bvh, positions):
    """The rule restated with numpy, independently of the library: a leaf takes np.min / np.max over its vertices, an
    interior node over its two children, in reverse node order (children come after their parents)."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    out = np.array(bvh.nodes, dtype=NODE_DTYPE, copy=True)
    for i in range(len(out) - 1, -1, -1):
        left, count = int(out[i]["leftNodeOrTriangleIndex"]), int(out[i]["triangleCount"])
        if count:
            v = pos[bvh.indices[left:left + count]]
            out[i]["min"], out[i]["max"] = v.min(axis=0), v.max(axis=0)
        else:
            out[i]["min"] = np.minimum(out[left]["min"], out[left + 1]["min"])
            out[i]["max"] = np.maximum(out[left]["max"], out[left + 1]["max"])
    return out


def ancestors(nodes):
    """parent[i] of every node (-1 for the root)"""
    parent = np.full(len(nodes), -1, np.int64)
    for i in np.flatnonzero(nodes["triangleCount"] == 0):
        left = int(nodes[i]["leftNodeOrTriangleIndex"])
        parent[left] = parent[left + 1] = i
    return parent


def refusals():
    """name -> (positions, indices, nodes, the status bvh_refit.h gives, a word of the message): the hand-made tree with
    one thing wrong. Every one is stopped by a read-only pass before a read that depends on the wrong value."""
    base = handmade()

    def with_node(i, left=None, count=None):
        nodes = base.nodes.copy()
        if left is not None:
            nodes[i]["leftNodeOrTriangleIndex"] = left
        if count is not None:
            nodes[i]["triangleCount"] = count
        return base.positions, base.indices, nodes

    def with_index(at, value):
        idx = base.indices.copy()
        idx[at] = value
        return base.positions, idx, base.nodes.copy()

    def with_coordinate(value):
        pos = base.positions.copy()
        pos[int(base.indices[40]), 1] = value  # inside the 20-triangle leaf
        return pos, base.indices, base.nodes.copy()

    return {
        "child_is_the_node_itself": with_node(2, left=2) + (BAD_CHILD, "children"),
        "child_before_the_node": with_node(6, left=3) + (BAD_CHILD, "children"),
        "right_child_outside": with_node(6, left=8) + (BAD_CHILD, "children"),
        "child_number_wraps_32_bits": with_node(6, left=0xFFFFFFFF) + (BAD_CHILD, "children"),
        "two_parents_and_orphans": with_node(2, left=5) + (BAD_PARENTS, "exactly one"),
        "leaf_count_not_a_multiple_of_3": with_node(5, count=5) + (BAD_LEAF, "leaf"),
        "leaf_range_past_the_indices": with_node(8, left=73) + (BAD_LEAF, "leaf"),
        "leaf_range_wraps_32_bits": with_node(8, left=0xFFFFFFFF) + (BAD_LEAF, "leaf"),
        "index_equal_to_vertex_count": with_index(30, 31) + (BAD_INDEX, "index"),
        "index_all_ones_in_no_leaf": with_index(68, 0xFFFFFFFF) + (BAD_INDEX, "index"),
        "coordinate_nan": with_coordinate(np.nan) + (NOT_FINITE, "finite"),
        "coordinate_inf": with_coordinate(-np.inf) + (NOT_FINITE, "finite"),
    }
