"""Meshes and trees of the tiny-tree tests (tests/test_mk_tiny_rule.py on the CPU, tests/test_gpu_tiny_tree.py on the GPU).

The reference's midpoint builder stops at 6 index positions (2 triangles) or where a split leaves one side empty, so a
leaf of more triangles exists only where every centroid falls on one side of the box's midpoint -- the Cornell room's
two 17-triangle leaves are such. The helpers here build meshes whose trees are known, and say what the tree must be."""
import numpy as np

from wcpt import scene as wscene
from wcpt._lib import NODE_DTYPE


def shape(bvh):
    """[(leftNodeOrTriangleIndex, triangleCount)] of every node"""
    return [(int(n["leftNodeOrTriangleIndex"]), int(n["triangleCount"])) for n in bvh.nodes]


def stack(n):
    """n triangles stacked along +x in front of a camera at the origin (yaw = pitch = 0 looks along +x), shrinking with
    distance so that each shows around the one before it. Every centroid has z = 0 while the box spans z in [-1, 2]
    (the longest axis, midpoint 0.5): the split leaves its right side empty, and the tree is a root leaf for any n."""
    pos, idx = [], []
    for k in range(n):
        x, h = 3.0 + 0.3 * k, 1.0 - 0.15 * k
        pos += [(x, -h, -1.0), (x, h, -1.0), (x, 0.0, 2.0)]
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    return wscene.HostMesh(np.array(pos, np.float32), np.array(idx, np.uint32))


def strip(n):
    """n triangles side by side along z at x = 3, each a unit apart: the midpoint builder halves them until 2 are left,
    so n = 1, 2 is a root leaf, n = 3, 4 a root over two leaves, and n = 5 the first tree of five nodes."""
    pos, idx = [], []
    for k in range(n):
        z = k - 0.5 * n
        pos += [(3.0, -0.5, z), (3.0, 0.5, z), (3.0 + 0.05 * k, 0.0, z + 0.9)]
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    return wscene.HostMesh(np.array(pos, np.float32), np.array(idx, np.uint32))


def box_mesh(cx, cy, cz, h):
    """the 12 triangles of an axis-aligned cube of half-width h"""
    c = np.array([[cx + sx * h, cy + sy * h, cz + sz * h] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)],
                 np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([v for a, b, cc, d in quads for v in (a, b, cc, a, cc, d)], np.uint32)
    return c, idx


def two_boxes_mesh(h=0.3):
    """two cubes centred at x = -0.6 and x = +0.6"""
    p0, i0 = box_mesh(-0.6, 0.0, 0.0, h)
    p1, i1 = box_mesh(0.6, 0.0, 0.0, h)
    return wscene.HostMesh(np.concatenate([p0, p1]), np.concatenate([i0, i1 + 8]))


def two_leaf_bvh(mesh, left_triangles):
    """A root over two leaves: the mesh's first `left_triangles` triangles and the rest, with their exact boxes. The
    midpoint builder splits each cube of two_boxes_mesh once more (6 / 6: its faces' centroids lie on either side of
    its middle), so the 12 / 12 tree of the two cubes is written out here; any BVH over the draw's indices is a valid
    input of the renderer and of the oracle."""
    pos, idx = mesh.positions, mesh.indices
    cut = 3 * left_triangles
    nodes = np.zeros(3, NODE_DTYPE)

    def bounds(node, a, b):
        v = pos[idx[a:b]]
        node["min"], node["max"] = v.min(axis=0), v.max(axis=0)

    bounds(nodes[0], 0, idx.size)
    nodes[0]["leftNodeOrTriangleIndex"], nodes[0]["triangleCount"] = 1, 0
    bounds(nodes[1], 0, cut)
    nodes[1]["leftNodeOrTriangleIndex"], nodes[1]["triangleCount"] = 0, cut
    bounds(nodes[2], cut, idx.size)
    nodes[2]["leftNodeOrTriangleIndex"], nodes[2]["triangleCount"] = cut, idx.size - cut
    return wscene.HostBVH(pos.copy(), idx.copy(), nodes)
