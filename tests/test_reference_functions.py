"""The shader's own functions, executed (oracle/refshader.py), against their two restatements:

  * the C oracle's exported helpers (oracle_ray_box, oracle_ray_sphere, oracle_ray_triangle, oracle_random_direction,
    pcg_hash, rand), and
  * arith_ref.model(fn, F32(), x), the exact-mode binary32 restatement that tests/test_gpu_arith_functions.py holds the
    kernels to bit for bit -- which ties those function-level GPU tests to reference text.

On every input set of tests/arith_ref.py for the functions the shader has: the triangle sets (grazing, edges, steep, far
and near, ...), the never-accepted ones (zero determinant: parallel and degenerate), the slivers, the origin-in-plane
items, the sphere sets (tangent, inside, behind), the optics sets (critical angle, small denominators, every ior pair) and
the child-pair items of the traversal (NaN and infinite slab bounds). Bit patterns, every item, no tolerance; a NaN must
meet a NaN.

fn 1 and 2 (the kernels' paired triangle test), fn 4 (the sphere's hit record), fn 6 (normalize, a built-in) and fn 7 (one
shading step) are code inside Intersect and TraceRay, or of the prelude, not functions the shader has: the image
comparisons of tests/test_reference_shader.py hold them to the reference.
"""
import functools

import numpy as np
import pytest

import arith_ref as R
import oracle
import ref_cases

F32 = np.float32


@pytest.fixture(scope="module")
def ref():
    return ref_cases.reference_library()


@functools.lru_cache(maxsize=None)
def _sets():
    sets = dict(R.all_sets())
    for name, x in R.never_accepted_sets().items():
        sets[0, f"never_{name}"] = x
    sets[0, "sliver"] = R.sliver_set()
    sets[0, "origin_in_plane"] = R.origin_in_plane_set()
    return sets


def _keys(fn):
    return sorted(name for f, name in _sets() if f == fn)


def _same(got, want, what):
    """float32 arrays (or uint32 views of them), bit for bit, NaN against NaN"""
    got = np.ascontiguousarray(got).view(np.uint32)
    want = np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, what
    both_nan = np.isnan(got.view(F32)) & np.isnan(want.view(F32))
    differ = (got != want) & ~both_nan
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} words differ, first item {int(np.argwhere(differ)[0][0])}"


def test_rng_is_the_shaders(ref):
    """pcg_hash, rand and RandomDirection: the shader's against the oracle's, on the seeds of the first pixels of a frame,
    of later frames (renderedFramesCount * 719393) and on the extremes; rand's state after each draw included."""
    seeds = list(range(64)) + [719393 * k + j for k in (1, 7, 49) for j in range(8)] + [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    for s in seeds:
        h = ref.pcg_hash(s)
        assert h == oracle.pcg_hash(s)
        got_v, got_s = ref.rand_stream(h, 16)
        want_v, want_s = oracle.rand_stream(h, 16)
        assert got_s == want_s
        _same(got_v, want_v, f"rand from {h}")
        (gd, gs), (wd, ws) = ref.random_direction(h), oracle.random_direction(h)
        assert gs == ws
        _same(gd, wd, f"RandomDirection from {h}")
    _same(ref.rand_stream(0, 1)[0], np.zeros(1, F32) + oracle.rand_stream(0, 1)[0], "rand from 0")


@pytest.mark.parametrize("name", _keys(0))
def test_ray_triangle(ref, name):
    x = _sets()[0, name]
    got = ref.ray_triangle(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12:15])
    _same(got[:, :1], R.model(0, R.F32(), x).view(F32), f"{name}: arith_ref.model")
    want = np.array([oracle.ray_triangle(*(r[k:k + 3] for k in (0, 3, 6, 9, 12))) for r in x], F32)
    _same(got[:, 0], want, f"{name}: oracle_ray_triangle")
    if name.startswith("never_"):
        assert (got[:, 0] == -1.0).all()


@pytest.mark.parametrize("name", _keys(3))
def test_ray_sphere(ref, name):
    x = _sets()[3, name]
    got = ref.ray_sphere(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9])
    _same(got[:, :1], R.model(3, R.F32(), x).view(F32), f"{name}: arith_ref.model")
    want = np.array([oracle.ray_sphere(r[0:3], r[3:6], r[6:9], r[9]) for r in x], F32)
    _same(got[:, 0], want, f"{name}: oracle_ray_sphere")
    miss = got[:, 0] == -1.0
    assert (got[miss, 1] == -1.0).all() and (got[~miss, 1] >= got[~miss, 0]).all()      # vec2(-1.0), and the far root


@pytest.mark.parametrize("name", _keys(5))
def test_reflectance_reflect_refract(ref, name):
    """CalculateReflectance, with reflect and refract as TraceRay calls them (eta = etaI / etaT), against fn 5's model."""
    x = _sets()[5, name]
    want = R.model(5, R.F32(), x).view(F32)
    eta = x[:, 6] / x[:, 7]
    assert eta.dtype == F32
    _same(ref.reflect_refract(x[:, 0:3], x[:, 3:6], eta), want[:, :6], f"{name}: reflect, refract")
    _same(ref.reflectance(x[:, 0:3], x[:, 3:6], x[:, 6], x[:, 7]), want[:, 6], f"{name}: CalculateReflectance")


def test_ray_box_and_child_pair(ref):
    """rayBoxIntersect on the child-pair items (NaN and infinite slab bounds among them): t0 and t1 against the oracle's
    helper where the item has a direction that gives its invDirection, and the traversal's decisions formed from the
    shader's (t0, t1) as pathTracer.comp:162 and :189-192 write them against arith_ref.child_pair_model and the oracle."""
    x = R.child_pair_set()
    o, inv = x[:, 0:3], x[:, 3:6]
    zero = np.zeros_like(o)
    lt = ref.ray_box(o, zero, inv, x[:, 6:9], x[:, 9:12])
    rt = ref.ray_box(o, zero, inv, x[:, 12:15], x[:, 15:18])
    with np.errstate(all="ignore"):
        dist = lambda t: np.where(t[:, 0] > 0, t[:, 0], t[:, 1])                         # noqa: E731  (:189-190)
        culled = lambda t, rec: (t[:, 0] > t[:, 1]) | (t[:, 1] < 0) | (t[:, 0] > rec)    # noqa: E731  (:162)
        inf = np.full(len(x), np.inf, F32)
        words = np.stack([(dist(lt) < dist(rt)).astype(np.uint32), (~culled(lt, inf)).astype(np.uint32),
                          (~culled(rt, inf)).astype(np.uint32), lt[:, 0].copy().view(np.uint32),
                          rt[:, 0].copy().view(np.uint32), (~culled(lt, x[:, 18])).astype(np.uint32)], axis=1)
    for want, what in ((R.child_pair_model(x), "arith_ref.child_pair_model"), (oracle.child_pair(x), "oracle_child_pair")):
        _same(words[:, 3:5], want[:, 3:5], f"{what}: t0")
        assert np.array_equal(words[:, (0, 1, 2, 5)], want[:, (0, 1, 2, 5)]), what
    # the oracle's own helper takes a direction: items whose invDirection is 1 / d of a finite d
    with np.errstate(all="ignore"):
        d = F32(1.0) / inv
        usable = np.isfinite(d).all(axis=1) & ((F32(1.0) / d).view(np.uint32) == inv.view(np.uint32)).all(axis=1)
    assert usable.sum() >= 100
    want = np.array([oracle.ray_box(r[0:3], dd, r[6:9], r[9:12]) for r, dd in zip(x[usable], d[usable])], F32)
    _same(lt[usable], want, "oracle_ray_box")
