"""wcpt_bvh_build_sah_device on the GPU: the binned-SAH BVH built by the kernels of pt_bvh_sah.hip equals
wcpt_bvh_build_sah byte for byte -- nodes [0, used), the node count and the whole index buffer -- on the cases of
bvh_sah_cases.py (the host builder's results are computed once there and shared); every refusal leaves both buffers as
they were; the scratch is shared with wcpt_bvh_build_device without either build disturbing the other; and the call is a
write of the index and node buffers to the runtime's caches.

The renders that follow a device build are compared bit for bit with a fresh context's renders of host-built buffers."""
import numpy as np
import pytest

import wcpt
from wcpt import scene as wscene
from wcpt._lib import NODE_DTYPE

import bvh_build_cases as midpoint_cases
import bvh_sah_cases as cases
from test_gpu_bvh_build import BOUNCES, H, W, _SharedBuffers, _bits, _download, _fresh_render, _scene_with

pytestmark = pytest.mark.gpu

T = wcpt._lib
NODE = NODE_DTYPE.itemsize


@pytest.fixture(scope="module")
def ctx():
    c = wcpt.Context(0)
    yield c
    c.close()


def _device_build(ctx, mesh, builder="sah"):
    vb, ib, nb, used = wscene.device_bvh_build(ctx, mesh, builder)
    try:
        return (used,) + _download(ctx, ib, mesh.indices.size, nb, used)
    finally:
        for b in (vb, ib, nb):
            ctx.buffer_free(b)


def _equals(got, ref):
    used, idx, nodes = got
    return used == len(ref.nodes) and np.array_equal(idx, ref.indices) and nodes == ref.nodes.tobytes()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_build_equals_the_host_builder(ctx, name):
    mesh, ref = cases.case(name)
    used, idx, nodes = _device_build(ctx, mesh)
    assert used == len(ref.nodes)
    assert np.array_equal(idx, ref.indices)
    assert nodes == ref.nodes.tobytes()


def test_scratch_shrinks_and_grows_between_the_two_builders(ctx):
    """a small build after a large one (the scratch and the bins are kept) and a larger one after that (they grow),
    alternating with the midpoint build, which carves the same allocation differently"""
    for name in ("soup_20000", "tri3", "two_clusters_1023_1024", "soup_20000"):
        mesh, ref = cases.case(name)
        assert _equals(_device_build(ctx, mesh), ref)
        mid_name = name.replace("two_clusters", "segments")
        mid_mesh, mid_ref = midpoint_cases.case(mid_name)
        assert _equals(_device_build(ctx, mid_mesh, "midpoint"), mid_ref)
    with wcpt.Context(0) as fresh:  # the midpoint build first, on a context whose scratch it sizes
        mesh, ref = cases.case("suzanita")
        mid_mesh, mid_ref = midpoint_cases.case("suzanita")
        assert _equals(_device_build(fresh, mid_mesh, "midpoint"), mid_ref)
        assert _equals(_device_build(fresh, mesh), ref)
        assert _equals(_device_build(fresh, mid_mesh, "midpoint"), mid_ref)


def test_idempotence(ctx):
    """twice from the same starting indices: the same bytes; from the permuted indices: the tree wcpt_bvh_build_sah gives
    from those indices"""
    mesh, ref = cases.case("suzanita")
    a = _device_build(ctx, mesh)
    b = _device_build(ctx, mesh)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    permuted = wscene.HostMesh(mesh.positions, ref.indices)
    again = wscene.bvh_build(permuted, "sah")
    assert _equals(_device_build(ctx, permuted), again)


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
                                 idx.size if index_count is None else index_count, h[2], builder="sah")
        assert ctx.buffer_download(ib, idx.nbytes) == idx.tobytes()
        assert ctx.buffer_download(nb, n_nodes * NODE) == fill[: n_nodes * NODE].tobytes()
        return e.value.code
    finally:
        for b in (vb, ib, nb):
            ctx.buffer_free(b)


def test_refusals_leave_both_buffers_alone(ctx):
    mesh, ref = cases.case("tri7")
    pos, idx = mesh.positions, mesh.indices
    bad = T.WCPT_ERROR_INVALID_ARGUMENT
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (vb, ib, 0xDEAD)) == bad
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (0xDEAD, ib, nb)) == bad
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (vb, 0xDEAD, nb)) == bad
    assert _refused(ctx, pos, idx, handles=lambda vb, ib, nb: (vb, ib, ib)) == bad
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
    # the SAH builder's own: a centroid overflow, a scale that is not finite, triangles an infinite extent apart, and a
    # node without a finite cost
    meshes = cases.refusal_meshes()
    for what in ("centroid_overflow", "scale_not_finite", "infinite_extent", "no_finite_cost"):
        m, _ = meshes[what]
        assert _refused(ctx, m.positions, m.indices) == bad, what
    # the context is still good for a build, and a coordinate no index refers to may be anything
    extra = np.vstack([pos, np.full((1, 3), np.nan, np.float32)])
    assert _equals(_device_build(ctx, wscene.HostMesh(extra, idx)), ref)


# ---- the runtime's caches ------------------------------------------------------------------------------------------------
class _SahBuffers(_SharedBuffers):
    def build_on_device(self, mesh):
        self.ctx.buffer_upload(self.vb, np.ascontiguousarray(mesh.positions, np.float32))
        self.ctx.buffer_upload(self.ib, np.ascontiguousarray(mesh.indices, np.uint32))
        self.set_draw(mesh.indices.size)
        return self.ctx.bvh_build_device(self.vb, mesh.positions.shape[0], self.ib, mesh.indices.size, self.nb, builder="sah")


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_render_after_a_device_build_over_warm_caches(kernel):
    """mushroom, midpoint tree, host-built, rendered still until the triangle records and the primary cache are warm; then
    suzanita's SAH tree built on the device into the same index and node buffers: the next frames are a fresh context's
    of the host-built SAH tree of suzanita"""
    mushroom = wscene.bvh_build(wscene.obj_load(wscene.MUSHROOM_OBJ))
    mesh, ref = cases.case("suzanita")
    want, _ = _fresh_render(_scene_with("default", ref), W, H, range(3), kernel)
    with wcpt.Context(0) as c:
        c.set_kernel(kernel)
        sb = _SahBuffers(c, "default", [mushroom, ref])
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
    assert BOUNCES == 3 and (W, H) == (76, 40)
    assert np.array_equal(_bits(got), _bits(want))


def test_renderer_init_with_a_device_sah_build():
    """PathTracingRenderer.Init(build="device", bvh="sah") renders the reference scene as build="host", bvh="sah" does"""
    s = wscene.reference_init()
    cam = wscene.update_camera(s.camera, 1.0)
    images = []
    for build in ("host", "device"):
        r = wcpt.PathTracingRenderer(0)
        try:
            r.Init(model_path=wscene.MUSHROOM_OBJ, build=build, bvh="sah")
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
            r.Init(bvh="lbvh")
    finally:
        r.Deinit()
