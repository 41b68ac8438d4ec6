"""Meshes for the midpoint builders (test input, no product code): each aims at one place where a level-synchronous
build can part from wcpt_bvh_build. Shared by tests/test_bvh_levels.py (host) and tests/test_gpu_bvh_build.py (device)."""
import ctypes as C
import functools
import glob
import os

import numpy as np

from wcpt import scene as wscene
from wcpt._lib import SceneC, check, lib

import deep_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "models", "*.obj")))


def soup(n, seed, spread=4.0, size=0.3):
    """n random triangles, each on three vertices of its own."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-spread, spread, (n, 1, 3))
    pos = (centres + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return wscene.HostMesh(np.ascontiguousarray(pos), np.arange(3 * n, dtype=np.uint32))


def _from_x(xs, seed):
    """One triangle per row of xs (its three x coordinates) on distinct vertices; y and z random in [0, 1)."""
    xs = np.asarray(xs, dtype=np.float32)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (xs.shape[0], 3, 3)).astype(np.float32)
    pos[:, :, 0] = xs
    return wscene.HostMesh(np.ascontiguousarray(pos.reshape(-1, 3)), np.arange(3 * xs.shape[0], dtype=np.uint32))


def coincident(xs, n=5):
    """n triangles with the x coordinates xs: one centroid, an x extent of 3 against 1 in y and z. (0, 3, 3) puts every
    centroid right of the split (the reference's loop rotates the segment by one), (0, 0, 3) left (nothing moves)."""
    return _from_x([xs] * n, seed=11)


def on_split():
    """Bounds [0, 4] in x, so splitPos = 2: centroids below, exactly on (they go right) and above it, interleaved."""
    rows = [(2, 2, 2), (0, 0, 1), (1, 2, 3), (4, 4, 4), (0, 2, 4), (1, 1, 1), (2, 2, 2), (3, 3, 4), (0, 1, 2), (2, 2, 2)]
    return _from_x(rows, seed=12)


def signed_zero(seed):
    """x >= 0 and y <= 0 everywhere, with +0.0 and -0.0 both present in either: the node minimum in x and maximum in y is
    a zero whose sign is the last one's in leaf order, at every level that keeps a zero."""
    rng = np.random.default_rng(seed)
    n = 24
    pos = rng.uniform(0.0, 4.0, (n, 3, 3)).astype(np.float32)
    pos[:, :, 1] = -pos[:, :, 1]
    zero = rng.random((n, 3)) < 0.4
    sign = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    pos[:, :, 0] = np.where(zero, sign, pos[:, :, 0])
    zero_y = rng.random((n, 3)) < 0.4
    pos[:, :, 1] = np.where(zero_y, -sign, pos[:, :, 1])
    return wscene.HostMesh(np.ascontiguousarray(pos.reshape(-1, 3)), np.arange(3 * n, dtype=np.uint32))


def deep_chain_mesh():
    """The mesh of tests/deep_tree.py's 40-level chain (its hand-made nodes are not used here)."""
    s = deep_tree.deep_chain_scene(wscene.HostScene("chain", None, None, None), levels=40)
    m = s.meshes[0]
    return wscene.HostMesh(m.positions, m.indices)


def budget_chain(n=46):
    """Triangle k sits at x = 4^-k with an extent of x / 8 in y and z, the last one at the origin: a node's x range is
    [0, 4^-j], so every split peels one triangle off to the right, exactly, and the left chain reaches level 32 with
    n - 32 triangles and stays a fat leaf there (depth budget 0)."""
    x = (4.0 ** -np.arange(n)).astype(np.float32)
    x[-1] = 0.0
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, :, 0] = x[:, None]
    pos[:, 1, 1] = x / 8
    pos[:, 2, 2] = x / 8
    return wscene.HostMesh(np.ascontiguousarray(pos.reshape(-1, 3)), np.arange(3 * n, dtype=np.uint32))


def two_clusters(a, b, seed):
    """a triangles in x < 1.5 and b in x > 8.5, shuffled: the root's split leaves level-1 segments of a and b triangles."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (a + b, 3, 3)).astype(np.float32)
    pos[a:, :, 0] += np.float32(9.0)
    pos[0, :, 0], pos[a, :, 0] = (0.0, 0.5, 0.5), (10.0, 9.5, 9.5)  # fixed bounds: splitPos = 5
    pos = pos[rng.permutation(a + b)]
    return wscene.HostMesh(np.ascontiguousarray(pos.reshape(-1, 3)), np.arange(3 * (a + b), dtype=np.uint32))


def cornell_mesh():
    s = SceneC()
    check(lib.wcpt_scene_generate(b"cornell", 0, C.byref(s)))
    try:
        mesh = wscene._mesh_from_c(s.mesh)
    finally:
        lib.wcpt_scene_free(C.byref(s))
    return wscene.obj_parse(wscene.mesh_to_obj(mesh))


SEGMENT_SIZES = ((63, 64), (65, 255), (256, 257), (1023, 1024), (1025, 63))

CASES = {
    "tri1": lambda: soup(1, 1),
    "tri2": lambda: soup(2, 2),
    "tri3": lambda: soup(3, 3),
    "tri7": lambda: soup(7, 4),
    "all_right_rotation": lambda: coincident((0, 3, 3)),
    "all_left_no_move": lambda: coincident((0, 0, 3)),
    "centroid_on_split": on_split,
    "signed_zero_a": lambda: signed_zero(21),
    "signed_zero_b": lambda: signed_zero(22),
    "deep_chain_mesh": deep_chain_mesh,
    "budget_chain": budget_chain,
    **{f"segments_{a}_{b}": functools.partial(two_clusters, a, b, 30 + i) for i, (a, b) in enumerate(SEGMENT_SIZES)},
    "soup_20000": lambda: soup(20000, 5, spread=20.0),
    **{os.path.splitext(os.path.basename(p))[0]: functools.partial(wscene.obj_load, p) for p in MODELS},
    "cornell": cornell_mesh,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, the host builder's result): computed once, shared, never modified by a test."""
    mesh = CASES[name]()
    return mesh, wscene.bvh_build(mesh)


def level_segments(bvh, level):
    """Triangle counts of the nodes on `level` of a built tree."""
    out, stack = [], [(0, 0, bvh.indices.size // 3)]
    while stack:
        i, d, _ = stack.pop()
        n = bvh.nodes[i]
        if d == level:
            out.append(_count(bvh, i))
        elif n["triangleCount"] == 0:
            left = int(n["leftNodeOrTriangleIndex"])
            stack += [(left, d + 1, 0), (left + 1, d + 1, 0)]
    return sorted(out)


def _count(bvh, i):
    n = bvh.nodes[i]
    if n["triangleCount"]:
        return int(n["triangleCount"]) // 3
    left = int(n["leftNodeOrTriangleIndex"])
    return _count(bvh, left) + _count(bvh, left + 1)
