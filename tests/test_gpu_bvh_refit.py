"""wcpt_bvh_refit_device on the GPU: the boxes the kernels of pt_bvh_refit.hip store equal wcpt_bvh_refit's byte for byte on
the trees of bvh_refit_cases.py (the host refit's results are computed once there and shared), nothing but nodes[0 ..
nodes_used) is written, every refusal leaves the node buffer as it was, the renders that follow a refit equal the CPU
oracle's of the same positions with the host-refit nodes, and the call is a write of the node and the vertex buffer to the
runtime's caches."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import wcpt
from wcpt import scene as wscene
from wcpt._lib import NODE_DTYPE

import oracle
import bvh_refit_cases as cases
from test_gpu_parity import KERNELS, assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
NODE = NODE_DTYPE.itemsize
SENTINEL_NODES = 5


@pytest.fixture(scope="module")
def ctx():
    c = wcpt.Context(0)
    yield c
    c.close()


# ---- bytes -----------------------------------------------------------------------------------------------------------------
MIDPOINT = ["tri1", "tri2", "tri3", "tri7", "cornell", "signed_zero_a", "budget_chain", "segments_1023_1024",
            "segments_1025_63", "mushroom", "soup_20000"]
SAH = ["tri1", "tri2", "tri3", "tri7", "cornell", "signed_zero_a", "depth_chain", "two_clusters_1023_1024",
       "two_clusters_1025_63", "mushroom", "soup_20000"]
TREES = [("midpoint", n) for n in MIDPOINT] + [("sah", n) for n in SAH] + [("handmade", "handmade")]


def _device_refit(ctx, positions, indices, nodes, nodes_used=None):
    """(the whole node buffer, the index buffer, the vertex buffer) after a device refit; the node buffer is
    SENTINEL_NODES nodes larger than the tree and those hold 0xA5 bytes"""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32)
    raw = np.concatenate([np.frombuffer(nodes.tobytes(), np.uint8), np.full(SENTINEL_NODES * NODE, 0xA5, np.uint8)])
    vb, ib, nb = ctx.buffer_from(pos), ctx.buffer_from(idx), ctx.buffer_from(raw)
    try:
        ctx.bvh_refit_device(vb, pos.shape[0], ib, idx.size, nb, len(nodes) if nodes_used is None else nodes_used)
        return (ctx.buffer_download(nb, raw.nbytes), ctx.buffer_download(ib, idx.nbytes), ctx.buffer_download(vb, pos.nbytes))
    finally:
        for b in (vb, ib, nb):
            ctx.buffer_free(b)


@pytest.mark.parametrize("move", [None, 5])
@pytest.mark.parametrize("kind,name", TREES)
def test_device_refit_equals_the_host_refit(ctx, kind, name, move):
    bvh = cases.tree(kind, name)
    pos, want = cases.host_refit(kind, name, move)
    got, idx, vertices = _device_refit(ctx, pos, bvh.indices, bvh.nodes)
    used = len(bvh.nodes) * NODE
    assert np.array_equal(np.frombuffer(got[:used], np.uint8), np.frombuffer(want.tobytes(), np.uint8))
    assert got[used:] == bytes([0xA5]) * (SENTINEL_NODES * NODE)
    assert idx == np.ascontiguousarray(bvh.indices, np.uint32).tobytes() and vertices == pos.tobytes()


def test_nodes_past_nodes_used_keep_their_bytes(ctx):
    """a root leaf refitted alone out of a larger tree's buffer: nodes_used 1, the other nodes as they were"""
    bvh = cases.tree("midpoint", "tri1")
    pos = cases.moved(bvh.positions, 8)
    two = np.concatenate([bvh.nodes[:1], bvh.nodes[:1]])
    got, _, _ = _device_refit(ctx, pos, bvh.indices, two, nodes_used=1)
    assert got[:NODE] == wscene.bvh_refit(bvh, pos).nodes.tobytes()
    assert got[NODE:2 * NODE] == bvh.nodes[:1].tobytes()


def test_scratch_shrinks_and_grows_between_calls(ctx):
    for kind, name in (("midpoint", "soup_20000"), ("midpoint", "tri3"), ("sah", "mushroom"), ("midpoint", "soup_20000")):
        bvh = cases.tree(kind, name)
        pos, want = cases.host_refit(kind, name, 5)
        got, _, _ = _device_refit(ctx, pos, bvh.indices, bvh.nodes)
        assert got[:len(want) * NODE] == want.tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _refused(ctx, pos, idx, nodes, nodes_used=None, vertex_count=None, index_count=None, handles=None):
    """the error of a refused device refit, after checking that the node buffer is byte-identical to before"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32)
    vb, ib, nb = ctx.buffer_from(pos), ctx.buffer_from(idx), ctx.buffer_from(nodes)
    try:
        h = handles(vb, ib, nb) if handles else (vb, ib, nb)
        with pytest.raises(wcpt.WcptError) as e:
            ctx.bvh_refit_device(h[0], pos.shape[0] if vertex_count is None else vertex_count, h[1],
                                 idx.size if index_count is None else index_count, h[2],
                                 len(nodes) if nodes_used is None else nodes_used)
        assert ctx.buffer_download(nb, nodes.nbytes) == nodes.tobytes()
        assert ctx.buffer_download(ib, idx.nbytes) == idx.tobytes() and ctx.buffer_download(vb, pos.nbytes) == pos.tobytes()
        return e.value
    finally:
        for b in (vb, ib, nb):
            ctx.buffer_free(b)


@pytest.mark.parametrize("what", list(cases.refusals()))
def test_what_is_not_a_tree_is_refused_with_the_nodes_unchanged(ctx, what):
    """argument errors found by read-only passes: none of these inputs lets a read depend on the wrong value"""
    pos, idx, nodes, _, word = cases.refusals()[what]
    e = _refused(ctx, pos, idx, nodes)
    assert e.code == T.WCPT_ERROR_INVALID_ARGUMENT and "bvh refit" in str(e) and word in str(e)


def test_handle_and_count_errors(ctx):
    bvh = cases.handmade()
    pos, idx, nodes = bvh.positions, bvh.indices, bvh.nodes
    bad = T.WCPT_ERROR_INVALID_ARGUMENT
    assert _refused(ctx, pos, idx, nodes, handles=lambda vb, ib, nb: (vb, ib, 0xDEAD)).code == bad
    assert _refused(ctx, pos, idx, nodes, handles=lambda vb, ib, nb: (0xDEAD, ib, nb)).code == bad
    assert _refused(ctx, pos, idx, nodes, handles=lambda vb, ib, nb: (vb, 0xDEAD, nb)).code == bad
    assert _refused(ctx, pos, idx, nodes, handles=lambda vb, ib, nb: (vb, vb, nb)).code == bad
    assert _refused(ctx, pos, idx, nodes, handles=lambda vb, ib, nb: (vb, ib, ib)).code == bad
    assert _refused(ctx, pos, idx, nodes, vertex_count=pos.shape[0] + 1).code == bad
    assert _refused(ctx, pos, idx, nodes, index_count=idx.size + 1).code == bad
    assert _refused(ctx, pos, idx, nodes, nodes_used=len(nodes) + 1).code == bad
    e = _refused(ctx, pos, idx, nodes, nodes_used=0)
    assert e.code == bad and "nodes_used" in str(e)
    # the context is still good for a refit, and a coordinate no index refers to may be anything
    extra = np.vstack([pos, np.full((1, 3), np.nan, np.float32)])
    got, _, _ = _device_refit(ctx, extra, idx, nodes)
    assert got[:len(nodes) * NODE] == cases.host_refit("handmade", "handmade", None)[1].tobytes()


# ---- render parity ---------------------------------------------------------------------------------------------------------
W = H = 64
FRAMES = range(3)


def _deformed(name):
    """the scene's mesh with every vertex moved by up to 0.1"""
    m = get_scene(name).meshes[0]
    return cases.moved(m.positions, 9, amount=0.1)


def _with_mesh(s, mesh):
    d = copy.copy(s)
    d.meshes = [mesh]
    return d


def _oracle_frames(s):
    acc = None
    for f in FRAMES:
        acc, _ = oracle.render_scene(s, W, H, sd=s.scene_data(W, H, max_bounce=3, frame=f), image=acc, threads=8)
    return acc


@functools.lru_cache(maxsize=None)
def _want(name, bvh="midpoint"):
    """the oracle's accumulation of FRAMES over the deformed positions with the host-refit nodes (computed once)"""
    s = get_scene(name)
    m = s.meshes[0]
    if bvh == "sah":
        m = wscene.bvh_build(wscene.HostMesh(m.positions, m.indices), "sah")
    return _oracle_frames(_with_mesh(s, wscene.bvh_refit(m, _deformed(name))))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["cornell", "reference_init"])
def test_render_after_a_device_refit_equals_the_oracle(name, kernel):
    """the scene rendered still until every cache is warm; then the mesh's positions move, are uploaded and the tree is
    refitted on the device: frames 0..2 are the oracle's of those positions with the host-refit nodes, bit for bit"""
    s = get_scene(name)
    m = s.meshes[0]
    with wcpt.Context(0) as c:
        c.set_kernel(kernel)
        dev = wcpt.DeviceScene(c, s)
        try:
            c.create_screen(W, H)
            for f in FRAMES:
                c.render(s.scene_data(W, H, max_bounce=3, frame=f), *dev.addresses())
            vb, ib, nb = dev.buffers[2:5]
            wscene.device_bvh_refit(c, vb, ib, nb, _deformed(name), m.indices.size, len(m.nodes))
            for f in FRAMES:
                c.render(s.scene_data(W, H, max_bounce=3, frame=f), *dev.addresses())
            c.sync()
            got = c.readback(H)
        finally:
            dev.free()
    assert_close(got, _want(name))


def _renderer_frames(name, refit, build="host", bvh="midpoint"):
    s = get_scene(name)
    cam = wscene.update_camera(s.camera, W / H)
    r = wcpt.PathTracingRenderer(0)
    try:
        r.Init(scene=s, build=build, bvh=bvh)
        r.CreateScreen((W, H))
        for _ in range(2):
            r.Render(cam)
        with pytest.raises(ValueError):
            r.UpdateMesh(0, _deformed(name)[:-1])
        assert r.renderedFramesCount == 2
        r.UpdateMesh(0, _deformed(name), refit=refit)
        assert r.renderedFramesCount == 0
        for _ in FRAMES:
            r.Render(cam)
        return r.Readback()
    finally:
        r.Deinit()


@pytest.mark.parametrize("refit", ["device", "host"])
@pytest.mark.parametrize("name", ["cornell", "reference_init"])
def test_renderer_update_mesh(name, refit):
    assert_close(_renderer_frames(name, refit), _want(name))


@pytest.mark.parametrize("refit", ["device", "host"])
def test_renderer_update_mesh_after_a_device_sah_build(refit):
    """Init(build="device", bvh="sah"): the host knows neither the index order nor the nodes; UpdateMesh needs neither"""
    assert_close(_renderer_frames("cornell", refit, build="device", bvh="sah"), _want("cornell", "sah"))


# ---- the runtime's caches --------------------------------------------------------------------------------------------------
def test_a_refit_drops_the_primary_cache():
    """still camera, frames 0, 1, 2: plain, write, read. The refit alone -- nothing uploaded, the same boxes -- is a write
    of the node and vertex buffers: the frame after it must not read the cache, as after an upload"""
    s = get_scene("cornell")
    m = s.meshes[0]
    with wcpt.Context(0) as c:
        dev = wcpt.DeviceScene(c, s)
        try:
            c.create_screen(W, H)
            for f in range(3):
                c.render(s.scene_data(W, H, max_bounce=3, frame=f), *dev.addresses())
            c.sync()
            writes, reads = c.primary_cache_stats()
            assert writes >= 1 and reads >= 1
            vb, ib, nb = dev.buffers[2:5]
            c.bvh_refit_device(vb, m.positions.shape[0], ib, m.indices.size, nb, len(m.nodes))
            c.render(s.scene_data(W, H, max_bounce=3, frame=3), *dev.addresses())
            c.sync()
            assert c.primary_cache_stats()[1] == reads
        finally:
            dev.free()


@pytest.mark.parametrize("kernel", KERNELS)
def test_vertices_written_behind_the_runtime_are_seen_after_a_refit(kernel):
    """the vertex buffer overwritten by a plain hipMemcpy to its device address, which the runtime does not see; the
    refit counts as a write of the vertices, so with WCPT_OPTION_TRIANGLE_CACHE left at 1 the triangle records are
    derived anew and the image is the oracle's for the new positions"""
    hip = ctypes.CDLL(wcpt.LIB_PATH)  # the HIP runtime the library is linked against
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    s = get_scene("cornell")
    m = s.meshes[0]
    pos = np.ascontiguousarray(_deformed("cornell"), np.float32)
    with wcpt.Context(0) as c:
        c.set_kernel(kernel)
        c.set_option(T.OPTION_TRIANGLE_CACHE, 1)
        dev = wcpt.DeviceScene(c, s)
        try:
            c.create_screen(W, H)
            for f in FRAMES:
                c.render(s.scene_data(W, H, max_bounce=3, frame=f), *dev.addresses())
            c.sync()
            vb, ib, nb = dev.buffers[2:5]
            assert hip.hipMemcpy(c.buffer_address(vb), pos.ctypes.data, pos.nbytes, 1) == 0  # hipMemcpyHostToDevice
            c.bvh_refit_device(vb, pos.shape[0], ib, m.indices.size, nb, len(m.nodes))
            for f in FRAMES:
                c.render(s.scene_data(W, H, max_bounce=3, frame=f), *dev.addresses())
            c.sync()
            got = c.readback(H)
        finally:
            dev.free()
    assert_close(got, _want("cornell"))
