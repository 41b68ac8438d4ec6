"""Scene buffers as an application hands them over, on the GPU: addresses inside a context buffer (one arena for a whole
scene, two meshes in shared buffers), addresses the context does not know (another context's allocations), and draws at
the 2^24 thresholds of the stack-entry and record-offset layouts (csrc/frame_prep.h draw_packed_refs, kTriFlagIndex24).

Every frame is compared bit for bit with the CPU oracle, and wcpt_render_counters with the oracle's counters, for both
kernels and single and pair records. The inputs, and the compact twins the oracle renders in place of the half-gigabyte
buffers, come from tests/scene_buffer_cases.py; tests/test_scene_buffer_cases.py proves on the CPU what is assumed of
them here (renumbering invariance, the flags of each case, the visibility of every leaf).

Offsets keep to what include/wcpt.h asks at wcpt_draw_command: node addresses at multiples of 16 bytes, vertex and index
addresses at multiples of 4."""
import copy
import ctypes

import numpy as np
import pytest

import wcpt
import oracle
from wcpt import scene as wscene

import scene_buffer_cases as sbc
from test_gpu_parity import assert_close, get_scene
from test_scene_buffer_cases import fp, mkt  # noqa: F401  (fixtures: the product's rules through their CPU shims)

pytestmark = pytest.mark.gpu

T = wcpt._lib
MK, WF = wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT
W, H, BOUNCES = sbc.W, sbc.H, sbc.BOUNCES
CONFIGS = [(MK, 0), (MK, 1), (WF, 0), (WF, 1)]        # kernel, WCPT_OPTION_PAIR_RECORDS
ARENA_CONFIGS = [(MK, 0), (MK, 1), (WF, -1)]


def _scene(base, meshes):
    s = copy.copy(get_scene(base))
    s.meshes = [wscene.HostBVH(*m) for m in meshes]
    return s


_refs = {}


def _oracle(key, s, frames=1):
    """the oracle's accumulated image after each of `frames` still-camera frames and its counters of frame 0, computed
    once per key and shared (never written)"""
    if key not in _refs:
        acc, out, cnt0 = None, [], None
        for f in range(frames):
            acc, cnt = oracle.render_scene(s, W, H, max_bounce=BOUNCES, frame=f, image=acc, threads=8)
            out.append(acc.copy())
            cnt0 = cnt0 or cnt
        _refs[key] = (out, cnt0)
    if len(_refs[key][0]) < frames:
        del _refs[key]
        return _oracle(key, s, frames)
    return _refs[key]


def _sd(s, frame=0):
    return s.scene_data(W, H, max_bounce=BOUNCES, frame=frame)


def _plan_kernel(fp, ntri, leaves):
    """what WCPT_KERNEL_AUTO resolves to for one draw of ntri triangles and a leaf estimate, by frame_prep.h frame_plan"""
    out = (ctypes.c_uint64 * 6)()
    fp.fp_frame_plan(1, ntri, sbc.INDEX24, ntri, leaves, ntri, -1, wcpt.KERNEL_AUTO, out)
    return int(out[4])


def _check_configs(ctx, s, key, addrs, configs, auto=None):
    """frame 0 and the counters of every (kernel, pair records) against the oracle; auto: the kernel WCPT_KERNEL_AUTO
    must resolve to, with the same frame"""
    refs, ref_cnt = _oracle(key, s)
    if auto is not None:
        ctx.set_kernel(wcpt.KERNEL_AUTO)
        ctx.set_option(T.OPTION_PAIR_RECORDS, -1)
        ctx.render(_sd(s), *addrs)
        ctx.sync()
        assert ctx.last_kernel() == auto
        assert_close(ctx.readback(H), refs[0], exact=True)
    for kernel, pairs in configs:
        ctx.set_kernel(kernel)
        ctx.set_option(T.OPTION_PAIR_RECORDS, pairs)
        ctx.render(_sd(s), *addrs)
        ctx.sync()
        assert ctx.last_kernel() == kernel
        assert_close(ctx.readback(H), refs[0], exact=True)
        assert ctx.render_counters(_sd(s), *addrs) == ref_cnt, (kernel, pairs)


def _check_sequence(ctx, s, key, addrs, pairs=1):
    """frames 0, 1, 2 of a still camera on the megakernel: frame 1 writes the primary cache, frame 2 reads it"""
    refs, _ = _oracle(key, s, frames=3)
    ctx.set_kernel(MK)
    ctx.set_option(T.OPTION_PAIR_RECORDS, pairs)
    w0, r0 = ctx.primary_cache_stats()
    for f in range(3):
        ctx.render(_sd(s, f), *addrs)
        ctx.sync()
        assert_close(ctx.readback(H), refs[f], exact=True)
    w1, r1 = ctx.primary_cache_stats()
    assert w1 > w0 and r1 > r0, "the primary cache must have been written and read"


def _draw(vertices, indices, nodes, index_count):
    d = np.zeros(1, T.DRAW_COMMAND_DTYPE)
    d[0] = (vertices, indices, nodes, index_count, 0)
    return d


# ---- 2. sub-allocated buffers ----------------------------------------------------------------------------------------
class Arena:
    """One context buffer holding a whole one-mesh scene at offsets, the bytes between the sub-allocations 0xA5."""

    def __init__(self, ctx, s, order, index_count=None, **kw):
        m = s.meshes[0]
        self.arrays = dict(materials=s.materials, spheres=s.spheres, vertices=np.ascontiguousarray(m.positions, np.float32),
                           indices=m.indices, nodes=m.nodes)
        fill, self.off, self.total = sbc.arena_bytes(self.arrays, order, **kw)
        self.ctx = ctx
        self.h = ctx.buffer_alloc(self.total)
        ctx.buffer_upload(self.h, np.full(self.total, sbc.FILL, np.uint8))
        for name, a in self.arrays.items():
            ctx.buffer_upload(self.h, a, offset=self.off[name])
        self.base = ctx.buffer_address(self.h)
        assert ctx.buffer_download(self.h, self.total) == fill.tobytes()
        self.set_draw(m.indices.size if index_count is None else index_count)

    def at(self, name):
        return self.base + self.off[name]

    def set_draw(self, index_count):
        self.ctx.buffer_upload(self.h, _draw(self.at("vertices"), self.at("indices"), self.at("nodes"), index_count),
                               offset=self.off["draws"])

    def addresses(self):
        return self.at("materials"), self.at("spheres"), self.at("draws")

    def free(self):
        self.ctx.buffer_free(self.h)


@pytest.mark.parametrize("order", [sbc.ORDER_NODES_LAST, sbc.ORDER_NODES_FIRST], ids=["nodes_last", "nodes_first"])
@pytest.mark.parametrize("name", ["cornell", "reference_init"])
def test_a_scene_in_one_arena(fp, name, order):
    """Cornell, and the reference's Init mesh with its spheres, each in one arena. Nodes last: the leaf scan sees exactly
    the tree. Nodes first: it reads the vertex, index and filler bytes behind the tree as nodes. Either way the frame and
    the counters are the oracle's; then a still-camera sequence through the primary cache."""
    s = get_scene(name)
    with wcpt.Context(0) as ctx:
        ctx.create_screen(W, H)
        arena = Arena(ctx, s, order)
        assert arena.off["nodes"] % 16 == 0
        if order is sbc.ORDER_NODES_LAST:
            assert arena.off["nodes"] + s.meshes[0].nodes.nbytes == arena.total
        # the leaf estimate takes the whole arena for nodes: thin leaves, the wavefront kernel
        ntri = s.meshes[0].indices.size // 3
        auto = _plan_kernel(fp, ntri, fp.fp_leaf_estimate(1, arena.total, ntri))
        assert auto == WF
        _check_configs(ctx, s, name, arena.addresses(), ARENA_CONFIGS, auto=auto)
        _check_sequence(ctx, s, name, arena.addresses(), pairs=1)
        arena.free()


def test_two_draws_out_of_shared_buffers():
    """Mesh B stored after mesh A in one vertex, one index and one node buffer: B's addresses are 12 * nvertA, 12 * ntriA
    and 32 * nodesA bytes in (4-byte-aligned interior addresses; the nodes' 32), its indices relative to its own first
    vertex. An indexCount one triangle past what is left of the index buffer from B's offset is refused, with the offset
    in the message, and the same context then renders the valid command again."""
    a, b = sbc.two_shared_meshes()
    s = _scene("default", [a, b])
    nva, nta, nna = len(a[0]), a[1].size // 3, len(a[2])
    with wcpt.Context(0) as ctx:
        ctx.create_screen(W, H)
        vb = ctx.buffer_from(np.concatenate([a[0], b[0]]))
        ib = ctx.buffer_from(np.concatenate([a[1], b[1]]))
        nb = ctx.buffer_from(np.concatenate([a[2], b[2]]))
        mats, sph = ctx.buffer_from(s.materials), ctx.buffer_from(s.spheres)
        va, ia, na = (ctx.buffer_address(h) for h in (vb, ib, nb))
        draws = np.concatenate([_draw(va, ia, na, a[1].size),
                                _draw(va + 12 * nva, ia + 12 * nta, na + 32 * nna, b[1].size)])
        db = ctx.buffer_from(draws)
        addrs = (ctx.buffer_address(mats), ctx.buffer_address(sph), ctx.buffer_address(db))
        _check_configs(ctx, s, "shared", addrs, ARENA_CONFIGS)
        bad = draws.copy()
        bad[1]["indexCount"] = b[1].size + 3
        ctx.buffer_upload(db, bad)
        with pytest.raises(wcpt.WcptError) as e:
            ctx.render(_sd(s), *addrs)
        assert e.value.code == -1000 and "indexCount" in str(e.value)
        assert f"{b[1].size * 4} bytes from offset {12 * nta}" in str(e.value)
        ctx.buffer_upload(db, draws)
        _check_configs(ctx, s, "shared", addrs, ARENA_CONFIGS)
        _check_sequence(ctx, s, "shared", addrs)


@pytest.mark.parametrize("kernel", [MK, WF])
@pytest.mark.parametrize("path", ["singles", "pairs", "index"])
def test_vertex_index_past_the_vertex_bound_from_the_offset(kernel, path):
    """The vertex bound of a draw whose vertices lie inside an arena is what is left of the arena from their offset. An
    index inside the arena's 12-byte count but beyond that bound gives a triangle no ray accepts: the oracle's frame with
    that vertex NaN. Through single records, pair records and the index path (indexCount covers one triangle only, so
    the leaf is gathered from the index and vertex buffers)."""
    pairs = {"singles": 0, "pairs": 1, "index": -1}[path]
    pos, idx, nodes, bad = sbc.one_leaf_mesh()
    s_dev = _scene("default", [(pos, idx.copy(), nodes)])
    with wcpt.Context(0) as ctx:
        ctx.create_screen(W, H)
        arena = Arena(ctx, s_dev, sbc.ORDER_NODES_LAST, index_count=3 if path == "index" else None)
        bound = (arena.total - arena.off["vertices"]) // 12
        past = bound + 1
        assert len(pos) < bound < past < arena.total // 12          # inside the arena, beyond bytes - offset
        idx_dev = idx.copy()
        idx_dev[3 * bad + 1] = past
        ctx.buffer_upload(arena.h, idx_dev, offset=arena.off["indices"])
        ctx.set_kernel(kernel)
        ctx.set_option(T.OPTION_PAIR_RECORDS, pairs)
        ctx.render(_sd(s_dev), *arena.addresses())
        ctx.sync()
        img = ctx.readback(H)
        arena.free()
    pos_ref, idx_ref = sbc.with_nan_vertex(pos, idx, bad)
    refs, _ = _oracle("past-bound", _scene("default", [(pos_ref, idx_ref, nodes)]))
    assert_close(img, refs[0], exact=True)


@pytest.mark.parametrize("order", [sbc.ORDER_NODES_LAST, sbc.ORDER_NODES_FIRST], ids=["nodes_last", "nodes_first"])
@pytest.mark.parametrize("on_records", [True, False])
def test_a_tiny_tree_whose_children_are_not_nodes_1_and_2(mkt, on_records, order):
    """Root at node 0, leaves at nodes 4 and 5 of an 8-node sub-allocation, a forced cut, pair records, one sample: the
    oracle's frame, and wcpt_mk_tiny_tree_stats advances exactly when the rule (csrc/mk_tiny_rule.h, on the arena's bytes
    from the nodes' offset) says the tree is tiny -- not when the draw's indexCount ends inside the second leaf."""
    tree = sbc.tiny_arena_tree(on_records)
    s = _scene("default", [tree.spread()])
    with wcpt.Context(0) as ctx:
        ctx.create_screen(W, H)
        ctx.set_option(T.OPTION_MK_SPLIT, 2)
        ctx.set_option(T.OPTION_PAIR_RECORDS, 1)
        arena = Arena(ctx, s, order, index_count=tree.index_count)
        view = np.frombuffer(ctx.buffer_download(arena.h, arena.total - arena.off["nodes"], arena.off["nodes"]), np.uint8)
        leaves = mkt.mkt_leaves(view.ctypes.data, view.size // 32, 3 * (tree.index_count // 3))
        assert leaves == (2 if on_records else 0)
        n0 = ctx.mk_tiny_tree_stats()
        ctx.render(_sd(s), *arena.addresses())
        ctx.sync()
        img = ctx.readback(H)
        assert ctx.mk_split_stats() == 1
        assert ctx.mk_tiny_tree_stats() - n0 == (1 if leaves else 0)
        refs, cnt = _oracle("tiny-arena", _scene("default", [sbc.tiny_arena_tree(True).compact()]))
        assert_close(img, refs[0], exact=True)
        assert ctx.render_counters(_sd(s), *arena.addresses()) == cnt
        arena.free()


# ---- 3. buffers the context does not know ----------------------------------------------------------------------------
@pytest.mark.parametrize("foreign", ["all_six", "geometry"])
@pytest.mark.parametrize("name", ["cornell", "reference_init"])
def test_buffers_of_another_context(fp, name, foreign):
    """The scene allocated and uploaded on a second context of the same device: to the rendering context its addresses
    are plain device pointers. No vertex bound, no node count (node-index stack entries, no scan), a leaf estimate of one
    triangle per leaf. all_six: the draw commands are foreign too and are read from the device; geometry: materials,
    spheres and draw commands are the rendering context's own."""
    s = get_scene(name)
    ntri = s.meshes[0].indices.size // 3
    with wcpt.Context(0) as owner, wcpt.Context(0) as ctx:
        dev = wcpt.DeviceScene(owner, s)
        owner.sync()
        ctx.create_screen(W, H)
        if foreign == "all_six":
            addrs = dev.addresses()
        else:
            draws = np.frombuffer(owner.buffer_download(dev.buffers[-1], 32), T.DRAW_COMMAND_DTYPE)
            own = [ctx.buffer_from(a) for a in (s.materials, s.spheres, draws)]
            addrs = tuple(ctx.buffer_address(h) for h in own)
        _check_configs(ctx, s, name, addrs, CONFIGS)
        ctx.set_kernel(wcpt.KERNEL_AUTO)
        ctx.set_option(T.OPTION_PAIR_RECORDS, -1)
        ctx.render(_sd(s), *addrs)
        ctx.sync()
        assert fp.fp_leaf_estimate(0, 32 * len(s.meshes[0].nodes), ntri) == ntri
        assert ctx.last_kernel() == _plan_kernel(fp, ntri, ntri) == WF
        assert_close(ctx.readback(H), _oracle(name, s)[0][0], exact=True)
        _check_sequence(ctx, s, name, addrs)
        dev.free()


def _moved(s, dx):
    """Cornell's positions moved by dx (the BVH left as it was, which the oracle traverses identically): (positions, scene)"""
    m = s.meshes[0]
    pos = np.ascontiguousarray(m.positions + np.float32(dx), np.float32)
    return pos, _scene("cornell", [(pos, m.indices, m.nodes)])


@pytest.mark.parametrize("kernel", [MK, WF])
@pytest.mark.parametrize("foreign", ["all_six", "geometry"])
def test_foreign_vertices_rewritten_with_the_triangle_cache_off(kernel, foreign):
    """WCPT_OPTION_TRIANGLE_CACHE = 0 on the rendering context: vertex bytes rewritten by their owner between two frames
    (its wcpt_buffer_upload, then its wcpt_sync) are what the next frame renders."""
    s = get_scene("cornell")
    with wcpt.Context(0) as owner, wcpt.Context(0) as ctx:
        dev = wcpt.DeviceScene(owner, s)
        owner.sync()
        ctx.create_screen(W, H)
        ctx.set_kernel(kernel)
        ctx.set_option(T.OPTION_TRIANGLE_CACHE, 0)
        if foreign == "all_six":
            addrs = dev.addresses()
        else:
            draws = np.frombuffer(owner.buffer_download(dev.buffers[-1], 32), T.DRAW_COMMAND_DTYPE)
            addrs = tuple(ctx.buffer_address(ctx.buffer_from(a)) for a in (s.materials, s.spheres, draws))
        for step, dx in enumerate((0.0, 0.06, -0.04)):
            pos, moved = _moved(s, dx)
            owner.buffer_upload(dev.buffers[2], pos)         # materials, spheres, vertices, indices, BVH, draws
            owner.sync()
            ctx.render(_sd(s), *addrs)
            ctx.sync()
            assert_close(ctx.readback(H), _oracle(f"cornell{dx:+.2f}", moved)[0][0], exact=True)
        dev.free()


def test_foreign_vertices_rewritten_with_the_triangle_cache_on():
    """include/wcpt.h, WCPT_OPTION_TRIANGLE_CACHE, of buffers the context does not know: their records are never kept
    from one frame preparation to the next, but a frame whose preparation is reused -- the draw commands uploaded on
    this context, and nothing allocated, uploaded, freed or set on it since -- renders the records of the frame before.
    So a rewrite by the owner is not seen by the next render, and is seen by the first render after any wcpt_buffer_upload
    on the rendering context; with draw commands the context reads from the device every render prepares anew, and a
    render with renderedFramesCount == 0 sees the rewrite."""
    s = get_scene("cornell")
    pos, moved = _moved(s, 0.06)
    old, new = _oracle("cornell+0.00", _moved(s, 0.0)[1])[0][0], _oracle("cornell+0.06", moved)[0][0]
    assert (old != new).any()
    for kernel in (MK, WF):
        with wcpt.Context(0) as owner, wcpt.Context(0) as ctx:
            dev = wcpt.DeviceScene(owner, s)
            owner.sync()
            ctx.create_screen(W, H)
            ctx.set_kernel(kernel)
            draws = np.frombuffer(owner.buffer_download(dev.buffers[-1], 32), T.DRAW_COMMAND_DTYPE)
            own = [ctx.buffer_from(a) for a in (s.materials, s.spheres, draws)]
            mine = tuple(ctx.buffer_address(h) for h in own)

            def frame(addrs):
                ctx.render(_sd(s), *addrs)
                ctx.sync()
                return ctx.readback(H)

            assert_close(frame(mine), old, exact=True)
            owner.buffer_upload(dev.buffers[2], pos)
            owner.sync()
            assert_close(frame(mine), old, exact=True)       # the preparation is reused: not seen
            ctx.buffer_upload(own[2], draws)                  # any upload on the rendering context: prepared anew
            assert_close(frame(mine), new, exact=True)
            # draw commands read from the device: every render prepares anew
            owner.buffer_upload(dev.buffers[2], _moved(s, 0.0)[0])
            owner.sync()
            assert_close(frame(dev.addresses()), old, exact=True)
            owner.buffer_upload(dev.buffers[2], pos)
            owner.sync()
            assert_close(frame(dev.addresses()), new, exact=True)
            dev.free()


# ---- 4. the 2^24 edges ----------------------------------------------------------------------------------------------
class BigBuffers:
    """One node buffer of 2^24 + 1 nodes (512 MiB; only the nodes the trees use are ever written), one index buffer of a
    little over 2^24 positions (64 MiB, filler 0) and one vertex buffer for every large case, allocated and uploaded once
    per module."""

    def __init__(self):
        self.cases = sbc.big_cases()
        self.ctx = wcpt.Context(0)
        ctx = self.ctx
        ctx.create_screen(W, H)
        s = get_scene("default")
        self.mats, self.sph = ctx.buffer_from(s.materials), ctx.buffer_from(s.spheres)
        pos, self.vbase = sbc.big_positions(self.cases)
        self.vb = ctx.buffer_from(pos)
        self.ib = ctx.buffer_from(sbc.big_index_buffer(self.cases))
        self.nb = ctx.buffer_alloc(32 * sbc.BIG_NODES)
        self.db = ctx.buffer_alloc(32)
        assert ctx.buffer_size(self.nb) == 32 * (sbc.N24 + 1) and ctx.buffer_size(self.ib) == 4 * sbc.BIG_INDICES

    def select(self, name):
        """the nodes of case `name` into the node buffer (its root at the draw's node 0, its leaves at the buffer's last
        two nodes) and its draw command; returns (scene of the compact twin, addresses)"""
        tree, _ = self.cases[name]
        ctx, nodes = self.ctx, tree.sparse_nodes()
        skip = sbc.BIG_NODES - tree.node_count            # the draw's BVH address, in nodes from the buffer's start
        assert skip + tree.left == sbc.BIG_NODES - 2
        ctx.buffer_upload(self.nb, nodes[:1], offset=32 * skip)
        ctx.buffer_upload(self.nb, nodes[1:], offset=32 * (sbc.BIG_NODES - 2))
        ctx.buffer_upload(self.db, _draw(ctx.buffer_address(self.vb) + 12 * self.vbase[name], ctx.buffer_address(self.ib),
                                         ctx.buffer_address(self.nb) + 32 * skip, tree.index_count))
        addrs = tuple(ctx.buffer_address(h) for h in (self.mats, self.sph, self.db))
        return _scene("default", [tree.compact()]), addrs

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def big():
    b = BigBuffers()
    yield b
    b.close()


BIG_NAMES = ["below", "nodes_at", "nodes_above", "index_at", "index_above", "both_above"]


@pytest.mark.parametrize("name", BIG_NAMES)
def test_draws_at_the_2_24_thresholds(big, fp, name):
    """below: 2^24 - 1 nodes and 2^24 - 1 index positions, packed stack entries and 24-bit record offsets -- the far child
    a fat leaf at node 2^24 - 2, pushed as (node_index << 8) | 255, the other a leaf that ends at the draw's last triangle,
    pushed as (left << 8) | count. nodes_at / nodes_above: 2^24 and 2^24 + 1 nodes, node-index entries, still 24-bit
    offsets. index_at / index_above / both_above: 2^24 + 2 index positions (both leaves off the records: the index path)
    and a few more (both on them: leaf_record_off), a leaf across 2^24 and one that starts past it. Every kernel and record
    kind, the counters, and a still-camera sequence, against the oracle on the compact twin."""
    s, addrs = big.select(name)
    ctx = big.ctx
    try:
        key = "big-" + big.cases[name][0].name.split("-")[0]  # the cases of one tree share its compact twin
        ntri = big.cases[name][0].index_count // 3
        auto = _plan_kernel(fp, ntri, fp.fp_leaf_estimate(1, 32 * sbc.BIG_NODES, ntri))
        assert auto == (MK if ntri >= 4 * ((sbc.BIG_NODES + 1) // 2) else WF) == WF
        _check_configs(ctx, s, key, addrs, CONFIGS, auto=auto)
        _check_sequence(ctx, s, key, addrs)
    finally:
        ctx.set_kernel(MK)
        ctx.set_option(T.OPTION_PAIR_RECORDS, -1)


def test_the_tiny_walk_reads_children_at_the_last_nodes(big, mkt):
    """below, with a forced cut: a root over two leaves on the records is tiny by the rule wherever its children are, and
    the walk reads them at nodes 2^24 - 3 and 2^24 - 2 through the scalar cache."""
    s, addrs = big.select("below")
    tree, ctx = big.cases["below"][0], big.ctx
    host = np.zeros(tree.node_count, T.NODE_DTYPE)          # untouched pages are never committed
    host[[0, tree.left, tree.left + 1]] = tree.sparse_nodes()
    assert mkt.mkt_leaves(host.ctypes.data, tree.node_count, tree.index_count) == 2
    try:
        ctx.set_kernel(MK)
        ctx.set_option(T.OPTION_PAIR_RECORDS, 1)
        ctx.set_option(T.OPTION_MK_SPLIT, 2)
        n0, s0 = ctx.mk_tiny_tree_stats(), ctx.mk_split_stats()
        ctx.render(_sd(s), *addrs)
        ctx.sync()
        assert ctx.mk_split_stats() - s0 == 1 and ctx.mk_tiny_tree_stats() - n0 == 1
        assert_close(ctx.readback(H), _oracle("big-end_fat", s)[0][0], exact=True)
    finally:
        ctx.set_option(T.OPTION_MK_SPLIT, -1)
        ctx.set_option(T.OPTION_PAIR_RECORDS, -1)
