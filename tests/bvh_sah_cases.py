"""Meshes for the binned-SAH builders (test input, no product code): each aims at one place where a level-synchronous
build can part from wcpt_bvh_build_sah. Shared by tests/test_bvh_sah_levels.py (host) and tests/test_gpu_bvh_build_sah.py
(device). check_cases() asserts, on the host builder's own tree, that each crafted case reaches the path it is named for."""
import functools
import os

import numpy as np

from wcpt import scene as wscene

import bvh_build_cases as base

SEGMENT_SIZES = base.SEGMENT_SIZES


def _mesh(tris):
    """(n, 3, 3) vertex coordinates -> a mesh of n triangles on vertices of their own"""
    pos = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 3))
    return wscene.HostMesh(pos, np.arange(pos.shape[0], dtype=np.uint32))


def coincident(n):
    """n copies of one triangle: no axis has a positive centroid extent"""
    return _mesh(np.tile(np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], np.float32), (n, 1, 1)))


def nearly_equal(n):
    """n near-copies of one large triangle, moved as a whole by -0.01 (the odd ones) or +0.01 in x: the only split
    parts the two groups and costs about n, more than the n - 1 a leaf may cost at most -- so up to 8 triangles stay one
    leaf, and 9 must split, [4, 5], although the cost says leaf"""
    tri = np.array([[0, 0, 0], [10, 0, 3], [0, 10, 6]], np.float32)
    tris = np.tile(tri, (n, 1, 1))
    tris[:, :, 0] += np.where(np.arange(n) % 2 == 1, np.float32(-0.01), np.float32(0.01))[:, None]
    return _mesh(tris)


def on_bin_edges():
    """x in [k - 0.25, k + 0.25] for k = 0..16, three triangles each, shuffled: 0.5f * (lo + hi) = k exactly, the centroid
    extent is 16 and the scale 1, so every centroid sits on the lower edge of its bin and the last on the clamp"""
    rng = np.random.default_rng(51)
    k = np.repeat(np.arange(17, dtype=np.float32), 3)
    tris = rng.uniform(0.0, 0.5, (k.size, 3, 3)).astype(np.float32)
    tris[:, 0, 0], tris[:, 1, 0], tris[:, 2, 0] = k - 0.25, k + 0.25, k
    return _mesh(tris[rng.permutation(k.size)])


def cost_tie():
    """a flat mesh (z = 0: an area is 2 x y, the same product either way round) that is its own image under x <-> y, each
    triangle followed by its mirror: bins, counts and costs on axis 1 are those on axis 0 bit for bit, and the strict
    compare keeps axis 0"""
    rng = np.random.default_rng(52)
    n = 40
    tris = np.zeros((n, 3, 3), np.float32)
    tris[:, :, :2] = rng.uniform(0.0, 8.0, (n, 1, 2)).astype(np.float32) + rng.uniform(0.0, 0.5, (n, 3, 2)).astype(np.float32)
    both = np.empty((2 * n, 3, 3), np.float32)
    both[0::2] = tris
    both[1::2] = tris[:, :, [1, 0, 2]]
    return _mesh(both)


def depth_chain(n=180):
    """Triangle k sits at x = 2^90 * 2^-k with an extent of x / 8 in y and z, the last one at the origin: the binned split
    peels a few triangles off the right at every level, the left chain reaches level 40 and stays a fat leaf there"""
    x = (np.float32(2.0) ** (90 - np.arange(n, dtype=np.float32))).astype(np.float32)
    x[-1] = 0.0
    tris = np.zeros((n, 3, 3), np.float32)
    tris[:, :, 0] = x[:, None]
    tris[:, 1, 1] = x / 8
    tris[:, 2, 2] = x / 8
    return _mesh(tris)


def box_extent_overflow(n=6):
    """triangles that each span -3e38 .. 3e38 in x, with distinct finite centroids: the node box's x extent is inf in
    binary32, so every area and cost is inf or NaN and no split is found. Up to 8 triangles that is a leaf on the host;
    more would be sorted there and are refused on the device (bvh_sah.h, kSahNoFiniteCost)."""
    t = np.arange(n, dtype=np.float32)
    tris = np.zeros((n, 3, 3), np.float32)
    tris[:, 0] = np.stack([np.full(n, -3e38, np.float32), t, np.zeros(n, np.float32)], 1)
    tris[:, 1] = np.stack([np.full(n, 3e38, np.float32), t, np.ones(n, np.float32)], 1)
    tris[:, 2] = np.stack([np.zeros(n, np.float32), t + 0.5, np.full(n, 0.5, np.float32)], 1)
    return _mesh(tris)


CASES = {
    "tri1": lambda: base.soup(1, 1),
    "tri2": lambda: base.soup(2, 2),
    "tri3": lambda: base.soup(3, 3),
    "tri7": lambda: base.soup(7, 4),
    **{f"coincident_{n}": functools.partial(coincident, n) for n in (5, 8, 9, 20, 33)},
    "nearly_equal_6": lambda: nearly_equal(6),
    "nearly_equal_9": lambda: nearly_equal(9),
    "signed_zero_a": lambda: base.signed_zero(21),
    "signed_zero_b": lambda: base.signed_zero(22),
    **{f"two_clusters_{a}_{b}": functools.partial(base.two_clusters, a, b, 30 + i) for i, (a, b) in enumerate(SEGMENT_SIZES)},
    "on_bin_edges": on_bin_edges,
    "cost_tie": cost_tie,
    "depth_chain": depth_chain,
    "box_extent_overflow": box_extent_overflow,
    "soup_20000": lambda: base.soup(20000, 5, spread=20.0),
    **{os.path.splitext(os.path.basename(p))[0]: functools.partial(wscene.obj_load, p) for p in base.MODELS},
    "cornell": base.cornell_mesh,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, the host SAH builder's result): computed once, shared, never modified by a test."""
    mesh = CASES[name]()
    return mesh, wscene.bvh_build(mesh, "sah")


def leaf_counts(bvh):
    """the leaves' triangle counts, in index order"""
    leaves = sorted((int(n["leftNodeOrTriangleIndex"]), int(n["triangleCount"]) // 3) for n in bvh.nodes if n["triangleCount"])
    return [c for _, c in leaves]


def _centroids(mesh, indices):
    """the host builder's centroids 0.5f * (lo + hi) of the triangles of `indices`, (n, 3)"""
    tri = np.asarray(mesh.positions, np.float32)[np.asarray(indices).reshape(-1, 3)]
    return np.float32(0.5) * (tri.min(axis=1) + tri.max(axis=1))


def _first_zero_bits(values):
    v = np.asarray(values, np.float32).ravel()
    return int(v[v == 0][0:1].view(np.uint32)[0])


# status bits of a refused level build (bvh_midpoint.h, bvh_sah.h)
BAD_INDEX, NOT_FINITE, CENTROID_NOT_FINITE, BAD_SCALE, NO_FINITE_COST = 1, 2, 4, 8, 16


def refusal_meshes():
    """name -> (mesh, status): the inputs the level build refuses. `infinite_extent` places two triangles 6e38 apart;
    its centroids 0.5f * (lo + hi) overflow before any extent is formed -- a finite centroid is at most FLOAT32_MAX / 2
    in magnitude, so an extent of finite centroids is finite -- and it is refused as a centroid overflow."""
    mesh, _ = case("tri7")
    pos, idx = mesh.positions.copy(), mesh.indices.copy()
    tri = idx.reshape(-1, 3)
    out = {}
    wrong = idx.copy()
    wrong[10] = pos.shape[0]
    out["index"] = (wscene.HostMesh(pos, wrong), BAD_INDEX)
    for what, value in (("nan", np.nan), ("inf", -np.inf)):
        p = pos.copy()
        p[int(idx[10]), 1] = value
        out[what] = (wscene.HostMesh(p, idx), NOT_FINITE)
    p = pos.copy()
    p[tri[2], 1] = (3.3e38, 3.2e38, 3.3e38)   # lo + hi overflows
    out["centroid_overflow"] = (wscene.HostMesh(p, idx), CENTROID_NOT_FINITE)
    p = pos.copy()
    p[:, 2] = 0.0
    p[tri[4], 2] = 1e-40                      # a centroid extent of 1e-40 in z: 16.f / ext is inf
    out["scale_not_finite"] = (wscene.HostMesh(p, idx), BAD_SCALE)
    p = pos.copy()
    p[tri[1], 0], p[tri[5], 0] = -3e38, 3e38
    out["infinite_extent"] = (wscene.HostMesh(p, idx), CENTROID_NOT_FINITE)
    out["no_finite_cost"] = (box_extent_overflow(12), NO_FINITE_COST)
    return out


def check_cases():
    """The crafted inputs reach the paths they are named for, in the host builder's own tree."""
    # no axis of positive centroid extent: a leaf up to 8 triangles, else the identity median split, recursively
    for n, leaves in ((5, [5]), (8, [8]), (9, [4, 5]), (20, [5, 5, 5, 5]), (33, [4, 5, 8, 8, 8])):
        mesh, ref = case(f"coincident_{n}")
        assert sorted(leaf_counts(ref)) == leaves
        assert np.array_equal(ref.indices, mesh.indices)
    _, ref = case("nearly_equal_6")
    assert len(ref.nodes) == 1 and ref.nodes[0]["triangleCount"] == 18
    _, ref = case("nearly_equal_9")
    assert leaf_counts(ref) == [4, 5] and len(ref.nodes) == 3
    # the root folds the triangles in their original order: its zero bounds carry the sign of the FIRST zero, and in at
    # least one of the two meshes that is not the sign of the last one
    differs = 0
    for name in ("signed_zero_a", "signed_zero_b"):
        mesh, ref = case(name)
        x, y = mesh.positions[:, 0], mesh.positions[:, 1]
        assert (x[x == 0].view(np.uint32) == 0).any() and (x[x == 0].view(np.uint32) != 0).any()
        assert ref.nodes[0]["min"][0] == 0 and ref.nodes[0]["max"][1] == 0
        assert int(ref.nodes[0]["min"][0:1].view(np.uint32)[0]) == _first_zero_bits(x)
        assert int(ref.nodes[0]["max"][1:2].view(np.uint32)[0]) == _first_zero_bits(y)
        differs += _first_zero_bits(x) != _first_zero_bits(x[::-1]) or _first_zero_bits(y) != _first_zero_bits(y[::-1])
    assert differs
    for a, b in SEGMENT_SIZES:
        _, ref = case(f"two_clusters_{a}_{b}")
        assert base.level_segments(ref, 1) == sorted((a, b))
    mesh, ref = case("on_bin_edges")
    cx = _centroids(mesh, mesh.indices)[:, 0]
    assert sorted(cx.tolist()) == np.repeat(np.arange(17.0), 3).tolist()
    mesh, ref = case("cost_tie")
    tris = mesh.positions.reshape(-1, 3, 3)
    assert np.array_equal(tris[1::2], tris[0::2][:, :, [1, 0, 2]]) and not tris[:, :, 2].any()
    left = int(ref.nodes[0]["leftNodeOrTriangleIndex"])
    n_left = base._count(ref, left)
    cen = _centroids(mesh, ref.indices)
    assert cen[:n_left, 0].max() < cen[n_left:, 0].min()          # the root was split on axis 0 ...
    assert not cen[:n_left, 1].max() < cen[n_left:, 1].min()      # ... and not on axis 1
    _, ref = case("depth_chain")
    assert ref.depth() == 41                                       # levels 0..40
    at_40 = base.level_segments(ref, 40)
    assert at_40 and max(at_40) > 8 and not base.level_segments(ref, 41)
    _, ref = case("box_extent_overflow")
    with np.errstate(over="ignore"):
        assert len(ref.nodes) == 1 and not np.isfinite(ref.nodes[0]["max"][0] - ref.nodes[0]["min"][0])
