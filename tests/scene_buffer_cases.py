"""Test input (plain numpy, no product code) for tests/test_gpu_scene_buffers.py: hand-made trees of a root over two
leaves whose nodes and index ranges sit anywhere in their buffers -- children at the last two of 2^24 - 1, 2^24 or
2^24 + 1 nodes, leaves that end at index position 2^24 - 1, cross 2^24 or start past it -- the byte layout of an arena
that holds a whole scene at offsets, and two meshes stored one after the other in shared buffers.

For each tree there is the *equivalent compact scene* the oracle renders (TwoLeafTree.compact): the same tree renumbered
0, 1, 2 over the leaves' indices back to back. The oracle's image and counters depend on the tree's shape and the
triangles a leaf names, not on node numbers, index positions or the bytes in between, so it never needs the
half-gigabyte arrays; tests/test_scene_buffer_cases.py proves that on small spread versions of the same constructions
(TwoLeafTree.spread), along with everything else the GPU tests lean on.

Geometry: a few dozen random triangles per leaf in front of the `default` scene's camera (at the origin, looking along
-z), about the spheres' fronts, so most primary rays and many bounce rays enter the tree; the leaves' boxes overlap and
are placed so that both child orders occur among the primary rays, also within one wave (leaf_geometry). Frames of 48x40 at 2 bounces:
the smallest shapes that still cross the thresholds."""
import numpy as np

NODE_DTYPE = np.dtype([("min", "<f4", (3,)), ("max", "<f4", (3,)), ("leftNodeOrTriangleIndex", "<u4"),
                       ("triangleCount", "<u4")])
DRAW_DTYPE = np.dtype([("vertexBuffer", "<u8"), ("indexBuffer", "<u8"), ("bvhBuffer", "<u8"), ("indexCount", "<u4"),
                       ("_pad", "<u4")])
FILL = 0xA5                     # the bytes between sub-allocations and of the nodes no tree uses
W, H, BOUNCES = 48, 40, 2
N24 = 1 << 24
PACKED, INDEX24 = 1, 2          # frame_prep.h table word 3


def leaf_geometry(rng, ntri, vbase, shelf=False):
    """ntri random triangles over 3 * ntri vertices of their own: (positions [3 ntri, 3], indices [3 ntri] from vbase).
    A slab across the whole view at z = -0.6 .. -0.4, or (shelf) a deeper box above the camera's axis, y = 0.2 .. 0.5, z =
    -0.9 .. -0.3: a ray that passes both enters the shelf through its front when it climbs steeply and through its
    underside, behind the slab's front, when it does not."""
    pos = (rng.random((ntri * 3, 3), dtype=np.float32) * 2.0 - 1.0).astype(np.float32)
    pos[:, 0] = pos[:, 0] * np.float32(0.5)
    if shelf:
        pos[:, 1] = pos[:, 1] * np.float32(0.15) + np.float32(0.35)
        pos[:, 2] = pos[:, 2] * np.float32(0.3) - np.float32(0.6)
    else:
        pos[:, 1] = pos[:, 1] * np.float32(0.5)
        pos[:, 2] = pos[:, 2] * np.float32(0.1) - np.float32(0.5)
    idx = (rng.permutation(ntri * 3) + vbase).astype(np.uint32)
    return pos, idx


def _box(positions, idx):
    p = positions[idx]
    return p.min(axis=0), p.max(axis=0)


class TwoLeafTree:
    """A root (node 0 of the draw) over two leaves at nodes `left` and `left + 1`; leaf i names the index positions
    [firsts[i], firsts[i] + len(leaf_indices[i])). node_count: the nodes of the draw's BVH from its address to the end
    of the buffer; index_count: the draw's indexCount; index_total: the index positions of the buffer."""

    def __init__(self, name, positions, leaf_indices, firsts, left, node_count, index_count, index_total):
        assert left >= 1 and left + 1 < node_count
        for f, ix in zip(firsts, leaf_indices):
            assert ix.size % 3 == 0 and f + ix.size <= index_total
        self.name, self.positions, self.leaf_indices, self.firsts = name, positions, list(leaf_indices), list(firsts)
        self.left, self.node_count, self.index_count, self.index_total = left, node_count, index_count, index_total

    # ---- the draw as it lies in its buffers -----------------------------------------------------------------------
    def sparse_nodes(self, left=None, firsts=None):
        """the three nodes the tree uses: root, left child, right child (at nodes 0, left, left + 1)"""
        left = self.left if left is None else left
        firsts = self.firsts if firsts is None else firsts
        nodes = np.zeros(3, NODE_DTYPE)
        boxes = [_box(self.positions, ix) for ix in self.leaf_indices]
        nodes[0] = (np.minimum(boxes[0][0], boxes[1][0]), np.maximum(boxes[0][1], boxes[1][1]), left, 0)
        for i in (0, 1):
            nodes[1 + i] = (boxes[i][0], boxes[i][1], firsts[i], self.leaf_indices[i].size)
        return nodes

    def node_buffer(self):
        """every node of the draw: FILL bytes but for the tree's three (small trees only)"""
        buf = np.full(self.node_count * NODE_DTYPE.itemsize, FILL, np.uint8).view(NODE_DTYPE)
        s = self.sparse_nodes()
        buf[0], buf[self.left], buf[self.left + 1] = s[0], s[1], s[2]
        return buf

    def index_buffer(self, filler=0):
        """every index position of the buffer: `filler` (a degenerate triangle, which no ray accepts and no leaf names)
        but for the leaves' ranges. Leaves that overlap must agree where they do."""
        buf = np.full(self.index_total, filler, np.uint32)
        for f, ix in zip(self.firsts, self.leaf_indices):
            buf[f:f + ix.size] = ix
        for f, ix in zip(self.firsts, self.leaf_indices):
            assert np.array_equal(buf[f:f + ix.size], ix), "overlapping leaves disagree"
        return buf

    def spread(self, filler=0):
        """(positions, indices, nodes) as the device holds them -- for the oracle only where the tree is small"""
        return self.positions, self.index_buffer(filler), self.node_buffer()

    # ---- the compact twin -----------------------------------------------------------------------------------------
    def compact(self, drop=None):
        """(positions, indices, nodes) of the same tree renumbered: nodes 0, 1, 2, the leaves' indices back to back.
        drop = i: leaf i's triangles removed (every index 0: degenerate), the tree's shape and boxes kept."""
        ix = [a.copy() for a in self.leaf_indices]
        if drop is not None:
            ix[drop][:] = 0
        nodes = self.sparse_nodes(left=1, firsts=[0, ix[0].size])
        return self.positions, np.concatenate(ix), nodes


def _tree(name, seed, tris, firsts, left, node_count, index_count, index_total, share=0):
    """Two leaves of tris[0] and tris[1] triangles. share = k: leaf 1 begins with leaf 0's last k triangles (their ranges
    overlap by 3 k positions)."""
    rng = np.random.default_rng(seed)
    p0, i0 = leaf_geometry(rng, tris[0], 0)
    p1, i1 = leaf_geometry(rng, tris[1], 3 * tris[0], shelf=True)
    if share:
        assert firsts[1] == firsts[0] + 3 * (tris[0] - share)
        i1[:3 * share] = i0[-3 * share:]
    return TwoLeafTree(name, np.concatenate([p0, p1]), [i0, i1], firsts, left, node_count, index_count, index_total)


# ---- section 4: the 2^24 edges --------------------------------------------------------------------------------------
# One node buffer of 2^24 + 1 nodes and one index buffer for every large case. A draw whose bvhBuffer is 0, 1 or 2 nodes
# into the node buffer has 2^24 + 1, 2^24 or 2^24 - 1 nodes; its root is its node 0 and its children are its last two
# nodes, which are the buffer's last two nodes in every case.
BIG_NODES = N24 + 1
T_END, T_FAT, T_CROSS, T_PAST, SHARE = 31, 90, 31, 30, 10
IC_BELOW = N24 - 1                                   # 3 x 5,592,405 triangles: the last one is positions 2^24 - 4 .. 2^24 - 2
FIRST_END = IC_BELOW - 3 * T_END                     # the leaf that ends at the draw's last triangle
FIRST_FAT = 3 * 1001                                 # the fat leaf (>= 255 index units), at an odd triangle index
FIRST_CROSS = IC_BELOW - 3 * SHARE                   # starts below 2^24, ends above it
FIRST_PAST = FIRST_CROSS + 3 * T_CROSS               # starts past 2^24
# An index buffer of 2^24 + 2 positions, the smallest with an indexCount that is a multiple of 3 and >= 2^24, cannot hold a
# whole triangle that starts at or past 2^24 (positions 2^24 .. 2^24 + 2 end one past it), so the buffer is the 600 bytes
# longer that the leaves across and past 2^24 need.
BIG_INDICES = FIRST_PAST + 3 * T_PAST
IC_AT = N24 + 2                                      # the first such count: neither flag; both leaves lie off its records


def _end_fat(node_count, index_count):
    """leaf 0 ends at the last triangle of a draw of 2^24 - 1 index positions; leaf 1, the right child, is fat"""
    return _tree(f"end_fat-{node_count}-{index_count}", 41, (T_END, T_FAT), [FIRST_END, FIRST_FAT], node_count - 2,
                 node_count, index_count, BIG_INDICES)


def _cross_past(node_count, index_count):
    """leaf 0 crosses 2^24, leaf 1 starts past it. Leaf 0 begins SHARE triangles before the end leaf's end, in the one
    index buffer: there it holds the end leaf's index values (valid in this tree's vertices too)."""
    t = _tree(f"cross_past-{node_count}-{index_count}", 43, (T_CROSS, T_PAST), [FIRST_CROSS, FIRST_PAST],
              node_count - 2, node_count, index_count, BIG_INDICES)
    t.leaf_indices[0][:3 * SHARE] = _end_fat(N24 - 1, IC_BELOW).leaf_indices[0][-3 * SHARE:]
    return t


# name -> (tree, the table flags of PACKED | INDEX24 the rule must give)
def big_cases():
    c = {}
    c["below"] = (_end_fat(N24 - 1, IC_BELOW), PACKED | INDEX24)
    c["nodes_at"] = (_end_fat(N24, IC_BELOW), INDEX24)
    c["nodes_above"] = (_end_fat(N24 + 1, IC_BELOW), INDEX24)
    c["index_at"] = (_cross_past(N24 - 1, IC_AT), 0)
    c["index_above"] = (_cross_past(N24 - 1, BIG_INDICES), 0)
    c["both_above"] = (_cross_past(N24 + 1, BIG_INDICES), 0)
    return c


def big_index_buffer(cases):
    """the one index buffer of every large case: filler 0, every tree's leaves at their positions"""
    buf = np.zeros(BIG_INDICES, np.uint32)
    for tree, _ in cases.values():
        for f, ix in zip(tree.firsts, tree.leaf_indices):
            buf[f:f + ix.size] = ix
    for tree, _ in cases.values():
        for f, ix in zip(tree.firsts, tree.leaf_indices):
            assert np.array_equal(buf[f:f + ix.size], ix), "overlapping leaves disagree"
    return buf


def big_positions(cases):
    """one vertex buffer for every large case: the two trees' vertices one after the other; returns (positions,
    {case name: first vertex})"""
    parts, base, at, seen = [], {}, 0, {}
    for name, (tree, _) in cases.items():
        key = tree.positions.tobytes()
        if key not in seen:
            seen[key] = at
            parts.append(tree.positions)
            at += len(tree.positions)
        base[name] = seen[key]
    return np.concatenate(parts), base


def small_twins():
    """The same constructions at a size the oracle can hold: children at nodes 5 and 6 of an 8-node buffer, leaves a
    few hundred index positions apart with filler between them; a fat second leaf; overlapping leaves; a leaf off the
    draw's records."""
    return [
        _tree("small-end-fat", 41, (T_END, T_FAT), [900, 3 * 7], 5, 8, 993, 1200),
        _tree("small-cross-past", 43, (T_CROSS, T_PAST), [300, 600], 5, 8, 690, 700),
        _tree("small-shared", 42, (T_END, T_CROSS), [300, 300 + 3 * (T_END - SHARE)], 5, 8, 500, 500, share=SHARE),
        _tree("small-off-records", 43, (T_CROSS, T_PAST), [300, 600], 5, 8, 302, 700),
    ]


# ---- section 2: one arena for a whole scene ---------------------------------------------------------------------------
def arena_layout(parts, order, align=64, gap=64, tail=0):
    """Offsets of the sub-allocations `parts` (name -> bytes) laid out in `order`, each at a multiple of `align`, at
    least `gap` bytes after the one before; `tail` bytes after the last. Returns ({name: offset}, total bytes)."""
    at, off = gap, {}
    for n in order:
        at = (at + align - 1) // align * align
        off[n] = at
        at += parts[n] + gap
    return off, at - gap + tail


def arena_bytes(arrays, order, draws=1, **kw):
    """The arena of a scene's arrays (name -> ndarray) and `draws` draw commands: (FILL bytes with every array at its
    offset, offsets, total). The draw commands' bytes are left FILL: they hold addresses, which only the device knows."""
    sizes = {n: a.nbytes for n, a in arrays.items()}
    sizes["draws"] = draws * DRAW_DTYPE.itemsize
    off, total = arena_layout(sizes, order, **kw)
    buf = np.full(total, FILL, np.uint8)
    for n, a in arrays.items():
        buf[off[n]:off[n] + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, off, total


ORDER_NODES_LAST = ["materials", "spheres", "draws", "vertices", "indices", "nodes"]
ORDER_NODES_FIRST = ["nodes", "vertices", "indices", "materials", "spheres", "draws"]


def tiny_arena_tree(on_records=True):
    """A root at node 0 over leaves at nodes 4 and 5 of an 8-node sub-allocation (the other nodes FILL). on_records =
    False: the draw's indexCount ends inside the second leaf, so that leaf is off the derived records and the tree is
    not tiny by the rule; the oracle's frame is the same."""
    n = 3 * (17 + 17)
    return _tree("tiny-arena", 44, (17, 17), [0, 51], 4, 8, n if on_records else n - 3, n)


def one_leaf_mesh():
    """A root leaf of 24 triangles and the triangle of it (visible: tests/test_scene_buffer_cases.py) whose second vertex
    index the vertex-bound test puts out of range: (positions, indices, nodes, triangle)"""
    pos, idx = leaf_geometry(np.random.default_rng(11), 24, 0)
    nodes = np.zeros(1, NODE_DTYPE)
    nodes[0] = (pos.min(axis=0), pos.max(axis=0), 0, idx.size)
    return pos, idx, nodes, 16


def with_nan_vertex(pos, idx, triangle):
    """the mesh in which `triangle`'s second vertex is NaN: what a vertex index past the vertex bound must render as"""
    out = idx.copy()
    out[3 * triangle + 1] = len(pos)
    return np.concatenate([pos, np.full((1, 3), np.nan, np.float32)]), out


def two_shared_meshes():
    """Mesh A and mesh B for one vertex, one index and one node buffer: B's indices are relative to B's first vertex.
    Returns (A, B), each a compact (positions, indices, nodes)."""
    a = _tree("shared-a", 45, (20, 23), [0, 60], 1, 3, 129, 129)
    b = _tree("shared-b", 46, (25, 18), [0, 75], 1, 3, 129, 129)
    b.positions = b.positions + np.array([0.25, 0.0, -0.02], np.float32)
    return a.compact(), b.compact()
