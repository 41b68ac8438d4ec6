"""The scenes of the primary-hit tests (tests/test_primary_ref.py pins tests/primary_ref.py to the C oracle on each of
them; tests/test_gpu_primary_hits.py compares the GPU's records with it). Test input, no product code, and no import of a
test module: the builders of every_kind, behind_quad, hollow_glass and inside_glass restate those of
tests/test_gpu_primary_resolved.py (the same geometry, cameras and materials), so the CPU suite depends on no GPU test
module."""
import copy

import numpy as np

import wcpt
from wcpt import scene as wscene

T = wcpt._lib
W, H = 70, 44   # partial 8x8 tiles on both edges
# the scenes whose whole frame is compared; assert_kinds says what each is there for
SCENES = ("cornell", "reference_init", "two_draws", "mixed_draws", "every_kind", "behind_quad", "hollow_glass",
          "inside_glass", "tie_quads", "tie_spheres")

_generated = {}
_built = {}


def get_scene(name):
    """wcpt.scene.generate(name), once."""
    if name not in _generated:
        _generated[name] = wscene.generate(name)
    return _generated[name]


def rays(s, w, h):
    """Host side, binary64: the primary rays of a w x h frame (origin [3], directions [h, w, 3]); for placing geometry on
    chosen pixels only."""
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
    return o, np.moveaxis(wd, 0, -1)


def sphere(pos, radius, material):
    sp = np.zeros(1, T.SPHERE_DTYPE)
    sp["position"], sp["radius"], sp["material"] = pos, radius, material
    return sp


def _glass(radius, camera):
    """default_dielectric's glass (material 0) with absorption as one sphere of the given radius at (0, 0, -1), and a
    metal sphere beside it."""
    s = copy.copy(get_scene("default_dielectric"))
    m = s.materials.copy()
    m["absorptionStrength"][0] = 0.7
    s.materials = m
    s.spheres = np.concatenate([sphere((0.0, 0.0, -1.0), radius, 0), sphere((0.9, 0.0, -1.6), 0.5, 3)])
    s.meshes = []
    s.camera = camera
    return s


def _inside_glass():
    """The camera inside the sphere: the reference takes a sphere's near root only, so the sphere is invisible from there."""
    return _glass(0.5, wscene.make_camera(position=(0.1, 0.05, -0.9), yaw=-90.0, pitch=0.0, fov=90.0))


def _hollow_glass():
    """`front` false on a sphere: a negative radius, seen from outside; its normal (p - c) / radius points inwards."""
    return _glass(-0.5, wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=-90.0, pitch=0.0, fov=90.0))


def _behind_quad():
    """A camera behind a single quad whose normal points away from it: back-facing triangle hits."""
    s = copy.copy(get_scene("cornell"))
    s.spheres = s.spheres[:0]
    x, half = 3.0, 2.0
    pos = np.array([(x, -half, -half), (x, half, -half), (x, half, half), (x, -half, half)], np.float32)
    s.meshes = [wscene.bvh_build(wscene.HostMesh(pos, np.array([0, 1, 2, 0, 2, 3], np.uint32)))]
    s.camera = wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)
    return s


def _every_kind():
    """One wave with every kind: small spheres on the primary rays of every 4th pixel of the rows around the middle, their
    materials cycling through four with period 2 x 2, and behind them a quad that ends at the frame's middle row."""
    s = copy.copy(get_scene("cornell"))
    s.meshes = []
    s.spheres = s.spheres[:0]
    s.camera = wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)
    o, d = rays(s, W, H)
    dist = 4.0
    pixel = float(np.linalg.norm(d[H // 2, W // 2 + 1] - d[H // 2, W // 2])) * dist
    sph = []
    for j, y in enumerate(range(H // 2 - 10, H // 2 + 10, 4)):
        for k, x in enumerate(range(1, W, 4)):
            sph.append(sphere(tuple(o + dist * d[y, x]), 1.0 * pixel, 1 + 2 * (j % 2) + (k % 2)))
    s.spheres = np.concatenate(sph)
    pos = np.array([(8.0, -20.0, -20.0), (8.0, 0.0, -20.0), (8.0, 0.0, 20.0), (8.0, -20.0, 20.0)], np.float32)
    s.meshes = [wscene.bvh_build(wscene.HostMesh(pos, np.array([0, 1, 2, 0, 2, 3], np.uint32)))]
    return s


def _two_draws():
    """The Cornell mesh drawn twice: every triangle hit ties with its twin, and draw 0 keeps it."""
    s = copy.copy(get_scene("cornell"))
    s.meshes = [s.meshes[0], s.meshes[0]]
    return s


def _mixed_draws():
    """Two different meshes, both visible: the Cornell mesh as draw 0 and, as draw 1, two quads hung on the primary rays of
    chosen pixels at distance 3.6 -- in front of the box's back wall (4.5), behind its blocks and spheres (2.8-3.4) and, on
    the left, over the sky beside the box. The quads have opposite windings: one faces the camera, one faces away. So
    the frame holds triangle hits of draw 0 and of draw 1, front- and back-facing in each, and draw 1 both wins and loses
    against draw 0."""
    s = copy.copy(get_scene("cornell"))
    o, d = rays(s, W, H)
    dist = 3.6

    def at(x, y):
        return tuple(o + dist * d[y, x])

    pos = np.array([at(2, 4), at(34, 4), at(34, 32), at(2, 32),           # quad A
                    at(37, 8), at(60, 8), at(60, 40), at(37, 40)], np.float32)  # quad B
    idx = np.array([0, 1, 2, 0, 2, 3, 4, 6, 5, 4, 7, 6], np.uint32)       # B wound the other way
    s.meshes = [s.meshes[0], wscene.bvh_build(wscene.HostMesh(pos, idx))]
    return s


def _tie_quads():
    """Two coincident quads in two draw commands: every hit has the same t in both, and the first draw keeps it."""
    s = copy.copy(scene("behind_quad"))
    s.meshes = [s.meshes[0], copy.deepcopy(s.meshes[0])]
    return s


def _tie_spheres():
    """One sphere at two indices (the second with another material), behind another: index 1 keeps the hit."""
    s = copy.copy(scene("hollow_glass"))
    b = sphere((0.0, 0.0, -1.0), 0.5, 0)
    dup = b.copy()
    dup["material"] = 2
    s.spheres = np.concatenate([sphere((0.9, 0.0, -1.6), 0.5, 3), b, dup])
    return s


_BUILDERS = {"two_draws": _two_draws, "mixed_draws": _mixed_draws, "every_kind": _every_kind, "behind_quad": _behind_quad,
             "hollow_glass": _hollow_glass, "inside_glass": _inside_glass, "tie_quads": _tie_quads,
             "tie_spheres": _tie_spheres}


def scene(name):
    if name not in _built:
        _built[name] = _BUILDERS[name]() if name in _BUILDERS else get_scene(name)
    return _built[name]


def with_distinct_emissions(s):
    """`s` with every material emitting its own colour, so that an image rendered with maxBounceCount 0 names the
    material of every hit."""
    out = copy.copy(s)
    m = s.materials.copy()
    for i in range(len(m)):
        m["emission"][i] = (0.125 + i, 0.25 + 2 * i, 0.5 + 3 * i)
        m["emissionStrength"][i] = 1.0 + 0.5 * i
    out.materials = m
    return out


def assert_kinds(name, r):
    """What scene `name` is there for, asserted from its records `r` [H, W]: back-facing triangle hits, back-facing
    sphere hits, misses, one 8x8 tile with every kind, triangle hits of two different draws, and ties that the earlier
    primitive keeps."""
    k = r["kind"] & T.HIT_KIND_MASK
    front = (r["kind"] & T.HIT_FRONT) != 0
    miss, sph, tri = k == T.HIT_MISS, k == T.HIT_SPHERE, k == T.HIT_TRIANGLE
    if name in ("behind_quad", "tie_quads"):
        assert (tri & ~front).sum() > 100 and miss.any() and not (tri & front).any()
        assert not r["draw"].any()                                   # tie_quads: the first of the coincident draws
    elif name == "hollow_glass":
        assert (sph & ~front).sum() > 100 and (sph & front).any() and miss.any()
    elif name == "inside_glass":
        assert sph.any() and miss.any() and not (r["index"][sph] == 0).any()   # invisible from inside
    elif name == "every_kind":
        full = 0
        for ty in range(r.shape[0] // 8):
            for tx in range(r.shape[1] // 8):
                tile = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
                full += bool(miss[tile].any() and sph[tile].any() and tri[tile].any() and
                             len(set(r["material"][tile][sph[tile]])) == 4)
        assert full > 0
    elif name in ("cornell", "two_draws"):
        assert tri.sum() > 1000 and sph.any() and miss.any() and (tri & ~front).any()
        assert len(set(r["index"][tri])) > 10 and len(set(r["index"][sph])) == 3
        assert not r["draw"].any()                                   # two_draws: the same mesh twice, the first keeps it
    elif name == "mixed_draws":
        d0, d1 = tri & (r["draw"] == 0), tri & (r["draw"] == 1)
        assert d0.sum() > 300 and d1.sum() > 300 and sph.any() and miss.any()
        assert (d1 & front).sum() > 100 and (d1 & ~front).sum() > 100      # both windings of draw 1
        assert (d0 & front).any() and (d0 & ~front).any()
        assert set(r["index"][d1]) == {0, 1, 2, 3} and len(set(r["index"][d0])) > 5
        assert not r["draw"][~tri].any()
    elif name == "reference_init":
        assert tri.sum() > 1000 and sph.sum() > 1000 and miss.any()
    elif name == "tie_spheres":
        assert (r["index"][sph] == 1).sum() > 100 and not (r["index"][sph] == 2).any()
        assert set(r["material"][sph & (r["index"] == 1)]) == {0}
    else:
        raise AssertionError(name)
