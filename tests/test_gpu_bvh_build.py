"""wcpt_bvh_build_device on the GPU: the midpoint BVH built by the kernels of pt_bvh_build.hip equals wcpt_bvh_build byte
for byte -- nodes [0, used), the node count and the whole index buffer -- on the cases of bvh_build_cases.py (the host
builder's results are computed once there and shared); every refusal leaves both buffers as they were; and the call is a
write of the index and node buffers to the runtime's caches and an ordinary citizen of the context's stream.

The renders that follow a device build are compared bit for bit with a fresh context's renders of host-built buffers."""
import copy

import numpy as np
import pytest

import wcpt
from wcpt import scene as wscene
from wcpt._lib import DRAW_COMMAND_DTYPE, NODE_DTYPE

import bvh_build_cases as cases
from test_gpu_parity import get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
NODE = NODE_DTYPE.itemsize


@pytest.fixture(scope="module")
def ctx():
    c = wcpt.Context(0)
    yield c
    c.close()


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def _download(ctx, ib, index_count, nb, used):
    idx = np.frombuffer(ctx.buffer_download(ib, 4 * index_count), np.uint32)
    nodes = ctx.buffer_download(nb, NODE * used)
    return idx, nodes


def _device_build(ctx, mesh):
    vb, ib, nb, used = wscene.device_bvh_build(ctx, mesh)
    try:
        return (used,) + _download(ctx, ib, mesh.indices.size, nb, used)
    finally:
        for b in (vb, ib, nb):
            ctx.buffer_free(b)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_build_equals_the_host_builder(ctx, name):
    mesh, ref = cases.case(name)
    used, idx, nodes = _device_build(ctx, mesh)
    assert used == len(ref.nodes)
    assert np.array_equal(idx, ref.indices)
    assert nodes == ref.nodes.tobytes()


def test_scratch_shrinks_and_grows_between_calls(ctx):
    """a small build after a large one (the scratch is kept) and a larger one after that (it grows)"""
    for name in ("soup_20000", "tri3", "segments_1023_1024", "soup_20000"):
        mesh, ref = cases.case(name)
        used, idx, nodes = _device_build(ctx, mesh)
        assert used == len(ref.nodes) and np.array_equal(idx, ref.indices) and nodes == ref.nodes.tobytes()


def test_idempotence(ctx):
    """twice from the same starting indices: the same bytes; from the permuted indices: the tree wcpt_bvh_build gives
    from those indices"""
    mesh, ref = cases.case("suzanita")
    a = _device_build(ctx, mesh)
    b = _device_build(ctx, mesh)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    permuted = wscene.HostMesh(mesh.positions, ref.indices)
    again = wscene.bvh_build(permuted)
    used, idx, nodes = _device_build(ctx, permuted)
    assert used == len(again.nodes) and np.array_equal(idx, again.indices) and nodes == again.nodes.tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(ctx, pos, idx, node_count=None, vertex_count=None, index_count=None, handles=None):
    """the call's error code, after checking that the index and node buffers are byte-identical to before"""
    pos = np.ascontiguousarray(pos, np.float32)
    idx = np.ascontiguousarray(idx, np.uint32)
    n_nodes = max(1, 2 * (idx.size // 3)) if node_count is None else node_count
    fill = np.full(max(n_nodes, 1) * NODE, 0xA5, np.uint8)
    vb, ib, nb = ctx.buffer_from(pos), ctx.buffer_from(idx), ctx.buffer_from(fill[: n_nodes * NODE])
    try:
        h = handles(vb, ib, nb) if handles else (vb, ib, nb)
        with pytest.raises(wcpt.WcptError) as e:
            ctx.bvh_build_device(h[0], pos.shape[0] if vertex_count is None else vertex_count, h[1],
                                 idx.size if index_count is None else index_count, h[2])
        assert ctx.buffer_download(ib, idx.nbytes) == idx.tobytes()
        assert ctx.buffer_download(nb, n_nodes * NODE) == fill[: n_nodes * NODE].tobytes()
        return e.value.code
    finally:
        for b in (vb, ib, nb):
            ctx.buffer_free(b)


def test_refusals_leave_both_buffers_alone(ctx):
    mesh, _ = cases.case("tri7")
    pos, idx = mesh.positions, mesh.indices
    bad = T.WCPT_ERROR_INVALID_ARGUMENT
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (vb, ib, 0xDEAD)) == bad
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (0xDEAD, ib, nb)) == bad
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (vb, 0xDEAD, nb)) == bad
    assert _refused(ctx, pos, idx, index_count=0) == bad
    assert _refused(ctx, pos, idx, index_count=20) == bad
    assert _refused(ctx, pos, idx, vertex_count=pos.shape[0] + 1) == bad
    assert _refused(ctx, pos, idx, index_count=idx.size + 3) == bad
    assert _refused(ctx, pos, idx, node_count=2 * 7 - 1) == bad
    for at in (0, 10, idx.size - 1):
        for value in (pos.shape[0], 0xFFFFFFFF):
            wrong = idx.copy()
            wrong[at] = value
            assert _refused(ctx, pos, wrong) == bad
    for value in (np.nan, np.inf, -np.inf):
        for c in range(3):
            wrong = pos.copy()
            wrong[int(idx[11]), c] = value
            assert _refused(ctx, wrong, idx) == bad
    # the context is still good for a build, and a coordinate no index refers to may be anything
    extra = np.vstack([pos, np.full((1, 3), np.nan, np.float32)])
    used, out_idx, nodes = _device_build(ctx, wscene.HostMesh(extra, idx))
    _, ref = cases.case("tri7")
    assert used == len(ref.nodes) and np.array_equal(out_idx, ref.indices) and nodes == ref.nodes.tobytes()


# ---- the runtime's caches ------------------------------------------------------------------------------------------------
W, H, BOUNCES = 76, 40, 3


def _scene_with(base, bvh):
    s = copy.copy(get_scene(base))
    s.meshes = [bvh]
    return s


def _fresh_render(s, w, h, frames, kernel, bounces=BOUNCES, pairs=-1):
    """a fresh context's accumulation of `frames` of the host-built scene s"""
    with wcpt.Context(0) as c:
        c.set_kernel(kernel)
        c.set_option(T.OPTION_PAIR_RECORDS, pairs)
        dev = wcpt.DeviceScene(c, s)
        try:
            c.create_screen(w, h)
            for f in frames:
                c.render(s.scene_data(w, h, max_bounce=bounces, frame=f), *dev.addresses())
            c.sync()
            return c.readback(h), c.mk_tiny_tree_stats()
        finally:
            dev.free()


class _SharedBuffers:
    """one vertex, index and node buffer large enough for every mesh of a test, and the draw command over them"""

    def __init__(self, ctx, base, meshes):
        self.ctx, self.base = ctx, get_scene(base)
        self.vb = ctx.buffer_alloc(max(m.positions.nbytes for m in meshes))
        self.ib = ctx.buffer_alloc(max(m.indices.nbytes for m in meshes))
        self.nb = ctx.buffer_alloc(max(2 * (m.indices.size // 3) for m in meshes) * NODE)
        self.mat, self.sph = ctx.buffer_from(self.base.materials), ctx.buffer_from(self.base.spheres)
        self.draws = ctx.buffer_alloc(DRAW_COMMAND_DTYPE.itemsize)

    def set_draw(self, index_count):
        a = self.ctx.buffer_address
        self.ctx.buffer_upload(self.draws, np.array([(a(self.vb), a(self.ib), a(self.nb), index_count, 0)], DRAW_COMMAND_DTYPE))

    def upload_host_built(self, bvh):
        self.ctx.buffer_upload(self.vb, bvh.positions)
        self.ctx.buffer_upload(self.ib, bvh.indices)
        self.ctx.buffer_upload(self.nb, bvh.nodes)
        self.set_draw(bvh.indices.size)

    def build_on_device(self, mesh):
        self.ctx.buffer_upload(self.vb, np.ascontiguousarray(mesh.positions, np.float32))
        self.ctx.buffer_upload(self.ib, np.ascontiguousarray(mesh.indices, np.uint32))
        self.set_draw(mesh.indices.size)
        return self.ctx.bvh_build_device(self.vb, mesh.positions.shape[0], self.ib, mesh.indices.size, self.nb)

    def render(self, w, h, frame, bounces=BOUNCES):
        s = _scene_with(self.base.name, None)
        a = self.ctx.buffer_address
        self.ctx.render(s.scene_data(w, h, max_bounce=bounces, frame=frame), a(self.mat), a(self.sph), a(self.draws))

    def free(self):
        for b in (self.vb, self.ib, self.nb, self.mat, self.sph, self.draws):
            self.ctx.buffer_free(b)


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_render_after_a_device_build_over_warm_caches(kernel):
    """mushroom, host-built, rendered still until the triangle records and the primary cache are warm; then suzanita
    built on the device into the same index and node buffers: the next frames are a fresh context's of host-built
    suzanita"""
    mushroom = wscene.bvh_build(wscene.obj_load(wscene.MUSHROOM_OBJ))
    mesh, ref = cases.case("suzanita")
    want, _ = _fresh_render(_scene_with("default", ref), W, H, range(3), kernel)
    with wcpt.Context(0) as c:
        c.set_kernel(kernel)
        sb = _SharedBuffers(c, "default", [mushroom, ref])
        try:
            c.create_screen(W, H)
            sb.upload_host_built(mushroom)
            for f in range(3):
                sb.render(W, H, f)
            c.sync()
            used = sb.build_on_device(mesh)
            assert used == len(ref.nodes)
            for f in range(3):
                sb.render(W, H, f)
            c.sync()
            got = c.readback(H)
        finally:
            sb.free()
    assert np.array_equal(_bits(got), _bits(want))


def test_tiny_tree_is_relearned_after_a_device_build():
    """at 1280x720 and 4 bounces the automatic split and the tiny-tree walk engage for the Cornell box (a root over two
    leaves); the buffers held the mushroom before, which is neither split nor tiny. Pair records, which the walk needs,
    are set from the start on both contexts: the automatic choice estimates the leaves from the node buffer's size, and
    the shared buffer has the mushroom's."""
    w, h, bounces = 1280, 720, 4
    mushroom = wscene.bvh_build(wscene.obj_load(wscene.MUSHROOM_OBJ))
    mesh, ref = cases.case("cornell")
    want, tiny_want = _fresh_render(_scene_with("cornell", ref), w, h, range(2), wcpt.KERNEL_MEGAKERNEL, bounces, pairs=1)
    assert tiny_want == 2
    with wcpt.Context(0) as c:
        c.set_option(T.OPTION_PAIR_RECORDS, 1)
        sb = _SharedBuffers(c, "cornell", [mushroom, ref])
        try:
            c.create_screen(w, h)
            sb.upload_host_built(mushroom)
            for f in range(2):
                sb.render(w, h, f, bounces)
            c.sync()
            assert c.mk_tiny_tree_stats() == 0
            sb.build_on_device(mesh)
            for f in range(2):
                sb.render(w, h, f, bounces)
            c.sync()
            assert c.mk_tiny_tree_stats() == 2
            got = c.readback(h)
        finally:
            sb.free()
    assert np.array_equal(_bits(got), _bits(want))


def test_build_between_overlapped_renders_without_a_sync():
    """frames 0-5 with the frame overlap forced on, then -- no wcpt_sync -- a device build in place, from the permuted
    indices the frames in flight are reading, then frames 6-9 on the new tree: the accumulated image is that of a plain
    stream which uploads the host builder's tree of the same indices between the two runs"""
    first = wscene.bvh_build(wscene.obj_load(wscene.MUSHROOM_OBJ))
    second = wscene.bvh_build(wscene.HostMesh(first.positions, first.indices))

    def run(overlap, device):
        with wcpt.Context(0) as c:
            c.set_option(T.OPTION_FRAME_OVERLAP, overlap)
            sb = _SharedBuffers(c, "default", [first])
            try:
                c.create_screen(W, H)
                sb.upload_host_built(first)
                for f in range(6):
                    sb.render(W, H, f)
                if device:
                    used = c.bvh_build_device(sb.vb, first.positions.shape[0], sb.ib, first.indices.size, sb.nb)
                    assert used == len(second.nodes)
                else:
                    c.buffer_upload(sb.ib, second.indices)
                    c.buffer_upload(sb.nb, second.nodes)
                for f in range(6, 10):
                    sb.render(W, H, f)
                img = c.readback(H)
                idx, nodes = _download(c, sb.ib, first.indices.size, sb.nb, len(second.nodes))
                return img, idx, nodes
            finally:
                sb.free()

    got, idx, nodes = run(2, True)
    want, _, _ = run(0, False)
    assert np.array_equal(idx, second.indices) and nodes == second.nodes.tobytes()
    assert np.array_equal(_bits(got), _bits(want))


def test_renderer_init_with_a_device_build():
    """PathTracingRenderer.Init(build="device") renders the reference scene as build="host" does"""
    s = wscene.reference_init()
    cam = wscene.update_camera(s.camera, 1.0)
    images = []
    for build in ("host", "device"):
        r = wcpt.PathTracingRenderer(0)
        try:
            r.Init(model_path=wscene.MUSHROOM_OBJ, build=build)
            r.CreateScreen((64, 64))
            for _ in range(2):
                r.Render(cam)
            images.append(r.Readback())
        finally:
            r.Deinit()
    assert np.array_equal(_bits(images[0]), _bits(images[1]))
    r = wcpt.PathTracingRenderer(0)
    try:
        with pytest.raises(ValueError):
            r.Init(build="gpu")
    finally:
        r.Deinit()
