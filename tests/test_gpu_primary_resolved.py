"""The resolved primary segment in the primary cache (csrc/primary_record.h) on the GPU: a write frame stores, per pixel,
the primary ray's direction and resolve_hit's result for it, and a read frame shades segment 0 from that entry without
computing the direction, its reciprocal or the hit resolution. Same bits, so every frame of every sequence here equals,
bit for bit, the same frame on a context with WCPT_OPTION_PRIMARY_CACHE = 0 and -- in exact arithmetic -- the CPU
oracle's accumulation; fast arithmetic is compared fast against fast only.

The sequence is frame 0 (plain), frame 1 (write), frames 2-4 (read), asserted through wcpt_primary_cache_stats so that no
case passes with the cache never valid. 70x44 leaves partial 8x8 tiles at both edges. The cases whose point is a kind of
primary hit (a back-facing sphere hit, a back-facing triangle hit, one wave with every kind) assert on the host, from the
scene's geometry in binary64, that such pixels exist. (A camera inside a sphere does not see it: the reference takes a
sphere's near root only. `front` false on a sphere needs a negative radius, and that is the case that carries it.) The oracle's accumulations are computed once per module and shared.
"""
import copy

import numpy as np
import pytest

import wcpt
import oracle
from wcpt import scene as wscene

from test_gpu_parity import _variant, assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 70, 44
FRAMES = range(5)
MISS, SPHERE, TRIANGLE = 0, 1, 2


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


# ---- scenes ---------------------------------------------------------------------------------------------------------
def _rays(s, w, h):
    """Host side, binary64: the primary rays of a w x h frame (pt_path.h primary_direction's expressions)."""
    sd = s.scene_data(w, h)
    P = np.asarray(sd["inverseProjection"], np.float64).reshape(4, 4).T   # column-major
    V = np.asarray(sd["inverseView"], np.float64).reshape(4, 4).T
    o = np.asarray(sd["position"], np.float64)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    cx = ((x + 0.5) / w) * 2.0 - 1.0
    cy = (1.0 - (y + 0.5) / h) * 2.0 - 1.0
    t = np.einsum("rc,chw->rhw", P, np.stack([cx, cy, np.ones_like(cx), np.ones_like(cx)]))
    d = t[:3] / t[3]
    d /= np.linalg.norm(d, axis=0)
    wd = np.einsum("rc,chw->rhw", V[:3, :3], d)
    wd /= np.linalg.norm(wd, axis=0)
    return o, np.moveaxis(wd, 0, -1)                                       # [3], [h, w, 3]


def _classify(s, w, h):
    """Host side, binary64: per pixel the kind of the primary hit (MISS / SPHERE / TRIANGLE), whether it is front-facing
    (dot(direction, normal) < 0) and the sphere's material. Not bit-exact with the kernel, and not needed to be: the
    tests ask only that pixels of a kind exist."""
    o, d = _rays(s, w, h)
    best = np.full((h, w), np.inf)
    kind = np.full((h, w), MISS)
    front = np.zeros((h, w), bool)
    material = np.zeros((h, w), np.int64)
    for sp in s.spheres:
        # the reference's sphere test (pathTracer.comp:110-119, :141-145): the near root only, so a sphere is invisible
        # from inside, and the normal is (p - c) / radius with the radius' sign
        c, r = np.asarray(sp["position"], np.float64), float(sp["radius"])
        oc = o - c
        b = (d * oc).sum(-1)
        disc = b * b - ((oc * oc).sum() - r * r)
        with np.errstate(invalid="ignore"):
            t = -b - np.sqrt(disc)
        take = (disc >= 0.0) & (t > 1e-9) & (t < best)
        n = (o + d * t[..., None] - c) / r
        best = np.where(take, t, best)
        kind = np.where(take, SPHERE, kind)
        front = np.where(take, (d * n).sum(-1) < 0.0, front)
        material = np.where(take, int(sp["material"]), material)
    for m in s.meshes:
        tri = m.positions[m.indices].astype(np.float64).reshape(-1, 3, 3)
        for a, bb, cc in tri:
            e1, e2 = bb - a, cc - a
            p = np.cross(d, e2)
            det = (p * e1).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                tv = o - a
                u = (p * tv).sum(-1) * inv
                q = np.cross(tv, e1)
                v = (d * q).sum(-1) * inv
                t = (q * e2).sum(-1) * inv
            take = (np.abs(det) > 1e-12) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 1e-9) & (t < best)
            n = np.cross(e1, e2)
            best = np.where(take, t, best)
            kind = np.where(take, TRIANGLE, kind)
            front = np.where(take, (d * n).sum(-1) < 0.0, front)
            material = np.where(take, 0, material)
    return kind, front, material


def _sphere(pos, radius, material):
    sp = np.zeros(1, T.SPHERE_DTYPE)
    sp["position"], sp["radius"], sp["material"] = pos, radius, material
    return sp


def _glass(radius, camera):
    """default_dielectric's glass (material 0, a dielectric) with absorption, as one sphere of the given radius at
    (0, 0, -1), and a metal sphere beside it."""
    s = copy.copy(get_scene("default_dielectric"))
    m = s.materials.copy()
    assert m["type"][0] == T.MATERIAL_DIELECTRIC
    m["absorptionStrength"][0] = 0.7
    s.materials = m
    s.spheres = np.concatenate([_sphere((0.0, 0.0, -1.0), radius, 0), _sphere((0.9, 0.0, -1.6), 0.5, 3)])
    s.meshes = []
    s.camera = camera
    return s


def _inside_glass():
    """The camera inside the dielectric sphere. The reference's sphere test takes the near root only, which lies behind a
    camera inside the sphere: the sphere is invisible from there, and the entries are the metal sphere's and misses."""
    return _glass(0.5, wscene.make_camera(position=(0.1, 0.05, -0.9), yaw=-90.0, pitch=0.0, fov=90.0))


def _hollow_glass():
    """`front` false on a sphere: the same sphere with a negative radius, seen from outside. Its normal (p - c) / radius
    points inwards, so every hit on it is a back-facing one -- the inside of a glass shell -- and the refracted paths'
    absorption term reads the entry's t."""
    return _glass(-0.5, wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=-90.0, pitch=0.0, fov=90.0))


def _quad_mesh(x, half):
    """a square at distance x in front of a camera at the origin that looks along +x; its normal points along +x, away
    from that camera"""
    pos = np.array([(x, -half, -half), (x, half, -half), (x, half, half), (x, -half, half)], np.float32)
    return wscene.HostMesh(pos, np.array([0, 1, 2, 0, 2, 3], np.uint32))


def _behind_quad():
    """A camera behind a single quad: its triangle hits are back-facing, so resolve_hit flipped the stored normal."""
    s = copy.copy(get_scene("cornell"))
    s.spheres = s.spheres[:0]
    s.meshes = [wscene.bvh_build(_quad_mesh(3.0, 2.0))]
    s.camera = wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)
    return s


def _every_kind():
    """One wave with every kind of entry. Small spheres on the primary rays of every 4th pixel of the rows around the
    middle of the frame, their materials cycling through the Cornell box's four sphere materials (an emissive metal, a
    mirror, the dielectric, a rough metal) with period 2 x 2, so any 8 x 8 tile there holds all four; behind them a quad
    that ends at the frame's middle row: triangle hits between the spheres below it, misses above."""
    s = copy.copy(get_scene("cornell"))
    s.meshes = []
    s.spheres = s.spheres[:0]
    s.camera = wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)
    o, d = _rays(s, W, H)
    dist = 4.0
    pixel = float(np.linalg.norm(d[H // 2, W // 2 + 1] - d[H // 2, W // 2])) * dist
    sph = []
    for j, y in enumerate(range(H // 2 - 10, H // 2 + 10, 4)):
        for k, x in enumerate(range(1, W, 4)):
            sph.append(_sphere(tuple(o + dist * d[y, x]), 1.0 * pixel, 1 + 2 * (j % 2) + (k % 2)))
    s.spheres = np.concatenate(sph)
    # the quad's upper edge on the middle of the frame (y = 0 for this camera), everything below it covered
    pos = np.array([(8.0, -20.0, -20.0), (8.0, 0.0, -20.0), (8.0, 0.0, 20.0), (8.0, -20.0, 20.0)], np.float32)
    s.meshes = [wscene.bvh_build(wscene.HostMesh(pos, np.array([0, 1, 2, 0, 2, 3], np.uint32)))]
    return s


_built = {}


def _scene(name):
    if name not in _built:
        if name == "two_draws":
            _built[name] = _variant("cornell", "two_draws")
        elif name == "inside_glass":
            _built[name] = _inside_glass()
        elif name == "hollow_glass":
            _built[name] = _hollow_glass()
        elif name == "behind_quad":
            _built[name] = _behind_quad()
        elif name == "every_kind":
            _built[name] = _every_kind()
        else:
            _built[name] = get_scene(name)
    return _built[name]


# ---- runs -----------------------------------------------------------------------------------------------------------
class _Run:
    """One context with the cache on or off, a resident scene and a screen."""

    def __init__(self, s, cache, w=W, h=H, arith=0, split=None, overlap=None):
        self.s, self.w, self.h = s, w, h
        self.ctx = wcpt.Context(0)
        self.ctx.set_option(T.OPTION_PRIMARY_CACHE, 1 if cache else 0)
        self.ctx.set_option(T.OPTION_ARITH, arith)
        if split is not None:
            self.ctx.set_option(T.OPTION_MK_SPLIT, split)
        if overlap is not None:
            self.ctx.set_option(T.OPTION_FRAME_OVERLAP, overlap)
        self.dev = wcpt.DeviceScene(self.ctx, s)
        self.ctx.create_screen(w, h)

    def render(self, frame, bounces, spp=1):
        self.ctx.render(self.s.scene_data(self.w, self.h, max_bounce=bounces, samples=spp, frame=frame),
                        *self.dev.addresses())

    def image(self, rows=None):
        self.ctx.sync()
        return self.ctx.readback(self.h if rows is None else rows)

    def close(self):
        self.dev.free()
        self.ctx.close()


def _sequence(s, cache, bounces, spp=1, layout=None, frames=FRAMES, **kw):
    """The image after each frame, (writes, reads) and the split renders the context counted. layout: wcpt_set_row_stripes'
    (y_first, rows, stripe, period), stripe 0 for a row block."""
    r = _Run(s, cache, **kw)
    try:
        rows = None
        if layout is not None:
            rows = layout[1]
            if layout[2]:
                r.ctx.set_row_stripes(*layout)
            else:
                r.ctx.set_row_range(layout[0], layout[1])
        imgs = []
        for f in frames:
            r.render(f, bounces, spp)
            imgs.append(r.image(rows))
        return imgs, r.ctx.primary_cache_stats(), r.ctx.mk_split_stats()
    finally:
        r.close()


_oracles = {}


def _oracle_acc(name, bounces, spp=1, frames=FRAMES):
    """The oracle's accumulation after each of the frames, full frame; computed once per module and left unchanged."""
    key = (name, bounces, spp, len(frames))
    if key not in _oracles:
        s, acc, out = _scene(name), None, []
        for f in frames:
            acc, _ = oracle.render_scene(s, W, H, sd=s.scene_data(W, H, max_bounce=bounces, samples=spp, frame=f),
                                         image=acc, threads=8)
            out.append(acc.copy())
        _oracles[key] = out
    return _oracles[key]


def _frame_rows(layout):
    y_first, rows, stripe, period = layout
    ly = np.arange(rows)
    return y_first + ly + ((ly // stripe) * (period - stripe) if stripe else 0)


def _check(name, bounces, spp=1, layout=None, arith=0, **kw):
    """Cache on against cache off, every frame bit for bit; frame 1 wrote and frames 2-4 read; in exact arithmetic every
    frame against the oracle's accumulation. Returns the cache-on images and the split renders counted."""
    s = _scene(name)
    on, stats, splits = _sequence(s, True, bounces, spp, layout, arith=arith, **kw)
    off, stats_off, _ = _sequence(s, False, bounces, spp, layout, arith=arith, **kw)
    assert stats == (1, len(FRAMES) - 2) and stats_off == (0, 0)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"frame {i} differs from the cache-off context"
    if arith == 0:
        ref = _oracle_acc(name, bounces, spp)
        rows = slice(None) if layout is None else _frame_rows(layout)
        for i, a in enumerate(on):
            assert np.array_equal(_bits(a), _bits(ref[i][rows])), f"frame {i} differs from the oracle's accumulation"
            assert_close(a, ref[i][rows])
    return on, splits


# ---- 1. the Cornell box; the primary segment as the last segment ----------------------------------------------------
@pytest.mark.parametrize("bounces", [4, 0])
def test_cornell(bounces):
    """bounces 0: segment 0 is the path's last, so a read frame is the entry, path_shade's emission term and the store."""
    _check("cornell", bounces)


# ---- 2. a camera inside a dielectric sphere; front false on a sphere -------------------------------------------------
def test_camera_inside_a_dielectric_sphere():
    """The sphere around the camera is never hit (near root only): what the frame holds is the sphere beside it and the
    sky, and the camera really is inside."""
    s = _scene("inside_glass")
    cam = np.array([float(v) for v in s.camera.position])
    assert np.linalg.norm(cam - np.asarray(s.spheres["position"][0], np.float64)) < float(s.spheres["radius"][0])
    kind, front, material = _classify(s, W, H)
    assert not ((kind == SPHERE) & (material == 0)).any()
    assert ((kind == SPHERE) & (material == 3)).sum() > 100 and (kind == MISS).sum() > 100
    _check("inside_glass", 4)


def test_back_facing_sphere_hit_and_its_absorption():
    s = _scene("hollow_glass")
    kind, front, material = _classify(s, W, H)
    assert ((kind == SPHERE) & ~front & (material == 0)).sum() > 100, "no back-facing hit on the dielectric sphere"
    assert s.materials["type"][0] == T.MATERIAL_DIELECTRIC and s.materials["absorptionStrength"][0] > 0.0
    assert np.any(np.asarray(s.materials["absorption"][0]) > 0.0)       # the absorption term reads h.t
    on, _ = _check("hollow_glass", 4)
    # ... and the term is in the image: without absorption the first frame differs
    s2 = copy.copy(s)
    s2.materials = s.materials.copy()
    s2.materials["absorptionStrength"][0] = 0.0
    plain, _, _ = _sequence(s2, False, 4, frames=range(1))
    assert not np.array_equal(_bits(plain[0]), _bits(on[0]))


# ---- 3. back-facing triangles: the stored normal is the flipped one ---------------------------------------------------
def test_camera_behind_a_quad():
    s = _scene("behind_quad")
    kind, front, _ = _classify(s, W, H)
    assert ((kind == TRIANGLE) & ~front).sum() > 100
    assert not ((kind == TRIANGLE) & front).any()
    assert (kind == MISS).any()
    _check("behind_quad", 4)


# ---- 4. one wave with every kind of entry ---------------------------------------------------------------------------
def test_every_kind_in_one_wave():
    s = _scene("every_kind")
    kind, front, material = _classify(s, W, H)
    mixed = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            k, m = kind[ty:ty + 8, tx:tx + 8], material[ty:ty + 8, tx:tx + 8]
            if (k == TRIANGLE).any() and (k == MISS).any() and all(((k == SPHERE) & (m == i)).any() for i in (1, 2, 3, 4)):
                mixed += 1
    assert mixed >= 1, "no 8x8 tile holds a triangle hit, a hit on each sphere material and a miss"
    types = {int(s.materials["type"][i]) for i in (1, 2, 3, 4)}
    assert types == {T.MATERIAL_METAL, T.MATERIAL_DIELECTRIC}
    _check("every_kind", 4)


# ---- 5. two draw commands: the same entry format -------------------------------------------------------------------
def test_two_draws():
    assert len(_scene("two_draws").meshes) == 2
    _check("two_draws", 4)


# ---- 6. the sample-reuse builds write and read ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "two_draws", "every_kind"])
def test_two_samples(name):
    _check(name, 4, spp=2)


def test_entry_written_by_two_samples_read_by_one_and_back():
    """the sample-reuse write build's entry (stored after its sample loop) serves the one-sample read build, and the
    one-sample write build's entry the sample-reuse read build"""
    s = _scene("cornell")
    for spps in ([1, 2, 1, 2, 1], [1, 1, 2, 1, 2]):
        res = {}
        for cache in (True, False):
            r = _Run(s, cache)
            try:
                imgs = []
                for f, spp in zip(FRAMES, spps):
                    r.render(f, 4, spp)
                    imgs.append(r.image())
                res[cache] = imgs
                assert r.ctx.primary_cache_stats() == ((1, 3) if cache else (0, 0))
            finally:
                r.close()
        for i, (a, b) in enumerate(zip(res[True], res[False])):
            assert np.array_equal(_bits(a), _bits(b)), f"samples {spps}: frame {i}"


# ---- 7. a forced cut: the head stage reads ---------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [1, 3])
@pytest.mark.parametrize("name", ["cornell", "every_kind"])
def test_forced_cut(name, cut):
    """WCPT_OPTION_MK_SPLIT = 1: the head is the entry's path_shade alone and appends right after it; 3: two traced
    segments follow it in the head"""
    _, splits = _check(name, 4, split=cut)
    assert splits == len(FRAMES)


# ---- 8. rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [(8, 24, 0, 0), (4, 24, 8, 16), (12, 16, 8, 16)])
def test_row_range_and_stripes(layout):
    """a row block and 8-row stripes of every other 8 rows: the entries are those of the context's rows"""
    _check("cornell", 4, layout=layout)


@pytest.mark.parametrize("stripe", [0, 8])
def test_two_rank_group_equals_one_context(stripe):
    """A one-process group of 2 ranks on one device (COPY), row blocks and 8-row stripes: each rank keeps the entries of
    its own rows, and the presented frame equals one context with the cache off."""
    s = _scene("cornell")
    fmt = T.PAYLOAD_RGBA32F
    with wcpt.Group([0, 0], root=0, transport=T.GROUP_TRANSPORT_COPY) as g:
        if stripe:
            g.set_option(T.GROUP_OPTION_ROW_STRIPE, stripe)
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(2)]
        g.create_screen(W, H)
        rc = g.context(0)
        nbytes = W * H * T.PAYLOAD_PIXEL_BYTES[fmt]
        out = rc.buffer_from(np.full(nbytes // 4, -5.0, np.float32))
        g.set_output(fmt, rc.buffer_address(out), nbytes)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        for f in FRAMES:
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.sync()
        raw = rc.buffer_download(out, nbytes)
        stats = [g.context(r).primary_cache_stats() for r in range(2)]
        rc.buffer_free(out)
        for d in devs:
            d.free()
    assert stats == [(1, 3), (1, 3)]
    off, _, _ = _sequence(s, False, 4)
    assert np.array_equal(np.frombuffer(raw, np.uint32).reshape(H, W, 4), _bits(off[-1]))
    assert np.array_equal(_bits(off[-1]), _bits(_oracle_acc("cornell", 4)[-1]))


# ---- 9. fast arithmetic: the entry holds the fast kernel's values -----------------------------------------------------
@pytest.mark.parametrize("name,spp,split", [("cornell", 1, None), ("every_kind", 1, None), ("hollow_glass", 1, None),
                                            ("cornell", 2, None), ("cornell", 1, 2), ("two_draws", 1, None)])
def test_fast_arithmetic(name, spp, split):
    _check(name, 4, spp=spp, arith=1, split=split)


def test_arithmetic_change_rewrites_the_entries():
    """an option change bumps the generation: the frame after it writes again, in the new arithmetic"""
    s = _scene("cornell")
    res = {}
    for cache in (True, False):
        r = _Run(s, cache)
        try:
            imgs = []
            for f in FRAMES:
                if f == 3:
                    r.ctx.set_option(T.OPTION_ARITH, 1)
                r.render(f, 4)
                imgs.append(r.image())
            res[cache] = imgs
            assert r.ctx.primary_cache_stats() == ((2, 2) if cache else (0, 0))
        finally:
            r.close()
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert np.array_equal(_bits(a), _bits(b)), f"frame {i}"


# ---- 10. forced overlap across a re-sort ------------------------------------------------------------------------------
def test_forced_overlap_across_a_resort():
    """18 consecutive frames as two pipes (the tile order is re-sorted after renders 1, 4 and 16: the pipes join and fork
    again), read back only after the whole sequence: equal to the sequence with the cache off and the overlap off, and to
    the oracle's accumulation."""
    s = _scene("cornell")
    frames = range(18)
    res = {}
    for cache, ov in ((True, 2), (False, 0)):
        r = _Run(s, cache, overlap=ov)
        try:
            for f in frames:
                r.render(f, 4)
            res[cache] = r.image()
            if cache:
                assert r.ctx.primary_cache_stats() == (1, 16)
        finally:
            r.close()
    assert np.array_equal(_bits(res[True]), _bits(res[False]))
    assert np.array_equal(_bits(res[True]), _bits(_oracle_acc("cornell", 4, frames=frames)[-1]))


# ---- 11. a sphere upload between read frames --------------------------------------------------------------------------
def test_sphere_upload_between_read_frames():
    """frames 0-2 (plain, write, read), then the spheres move: frame 3 writes again instead of shading the stale entries,
    frame 4 reads the new ones; every image equals the cache-off context's, and the move does change the image"""
    s = _scene("cornell")
    moved = s.spheres.copy()
    moved["position"][:, 1] += np.float32(0.125)
    res = {}
    for cache in (True, False):
        r = _Run(s, cache)
        try:
            imgs = []
            for f in FRAMES:
                if f == 3:
                    r.ctx.buffer_upload(r.dev.buffers[1], moved)   # DeviceScene: materials, then spheres
                r.render(f, 4)
                imgs.append(r.image())
            res[cache] = imgs
            assert r.ctx.primary_cache_stats() == ((2, 2) if cache else (0, 0))
        finally:
            r.close()
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert np.array_equal(_bits(a), _bits(b)), f"frame {i} differs from the cache-off context"
    still = _oracle_acc("cornell", 4)
    assert np.array_equal(_bits(res[True][2]), _bits(still[2]))
    assert not np.array_equal(_bits(res[True][3]), _bits(still[3]))
    s2 = copy.copy(s)
    s2.spheres = moved
    acc = still[2].copy()
    for f in (3, 4):
        acc, _ = oracle.render_scene(s2, W, H, sd=s2.scene_data(W, H, max_bounce=4, frame=f), image=acc, threads=8)
        assert np.array_equal(_bits(res[True][f]), _bits(acc))
