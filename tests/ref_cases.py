"""The cases on which the oracle and the kernels are held to the compiled reference shaders (oracle/refshader.py), shared by
tests/test_reference_shader.py and tests/test_gpu_reference_shader.py (test infrastructure; not a test module).

The reference's `uint nodeStack[32]` is a real array in the compiled shader, so a case is rendered there only after the
oracle's counters say that no segment of it goes deeper (refshader.fits_reference_stack). DROPPED lists what that guard
keeps out; test_reference_shader.py asserts both lists."""
import collections
import copy
import functools
import os

import numpy as np
import pytest

import wcpt
from wcpt import scene as wscene
import oracle
import refshader
from deep_tree import deep_chain_scene
from random_scenes import random_scene

Case = collections.namedtuple("Case", "id scene W H bounces spp frame init y0 rows")


@functools.lru_cache(maxsize=None)
def get_scene(name):
    return wscene.generate(name)


def variant(s, kind):
    """The edge inputs of test_edge_inputs_match_oracle on a copy of scene s."""
    s = copy.copy(s)
    if kind == "no_spheres":
        s.spheres = s.spheres[:0]
    elif kind == "no_meshes":
        s.meshes = []
    elif kind == "empty":
        s.spheres = s.spheres[:0]
        s.meshes = []
    elif kind == "two_draws":          # the same mesh drawn twice: exercises the per-draw loop (:152-201)
        s.meshes = [s.meshes[0], s.meshes[0]]
    elif kind == "all_dielectric":     # type 1 everywhere, with absorption (:263-280)
        m = s.materials.copy()
        m["type"] = 1
        m["ior"] = 1.5
        m["absorptionStrength"] = 0.7
        m["absorption"] = [0.2, 0.5, 0.9]
        s.materials = m
    elif kind != "base":
        raise ValueError(kind)
    return s


def nan_slab_scene():
    """A camera exactly on the plane of a box face, looking along an axis: with a one-row frame every ray has
    direction.y == 0 and origin.y == the root box's min.y, so that slab's tbot is 0 * inf = NaN (pathTracer.comp:98).
    The hand-made root leaf's box is loose around a quad that the rays do meet: min / max as minNum / maxNum drop the
    NaN, the other slab bound (+inf) culls the node and the pixels show the sky; min / max that hand the NaN on leave
    every comparison of :162 false and the quad is hit."""
    s = copy.copy(get_scene("default"))
    s.spheres = s.spheres[:0]
    pos = np.array([[3, -1, -2], [3, 1, -2], [3, 1, 2], [3, -1, 2]], np.float32)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    nodes = np.zeros(1, dtype=wcpt._lib.NODE_DTYPE)
    nodes[0] = ((2, 0, -3), (4, 2, 3), 0, 6)
    s.meshes = [wscene.HostBVH(pos, idx, nodes)]
    s.camera = wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)
    return s


def _named(name, kind="base"):
    return lambda: variant(get_scene(name), kind)


@functools.lru_cache(maxsize=None)
def _random_scene(seed):
    return random_scene(seed)


def _random(seed):
    return lambda: _random_scene(seed)[0]


def _cases():
    out = []
    # the golden scenes
    for name, bounces, spp in (("cornell", 4, 1), ("default", 3, 1), ("default_dielectric", 3, 2), ("default_emissive", 3, 2),
                               ("reference_init", 3, 1), ("reference_init_glass", 3, 2), ("atrium", 4, 1)):
        out.append(Case(name, _named(name), 48, 32, bounces, spp, 0, None, 0, None))
    # the 12 random scenes of test_random_scenes_match_oracle, with its initial image and frame number
    for seed in range(12):
        _, bounces, spp, frame = _random_scene(seed)
        out.append(Case(f"random{seed}", _random(seed), 40, 28, bounces, spp, frame, seed + 100, 0, None))
    # every kind of test_edge_inputs_match_oracle
    for kind, bounces, spp in (("no_spheres", 3, 1), ("no_meshes", 3, 1), ("empty", 3, 1), ("two_draws", 3, 1),
                               ("all_dielectric", 6, 2), ("base", 0, 1), ("base", 12, 1), ("base", 3, 0)):
        out.append(Case(f"edge_{kind}_b{bounces}_s{spp}", _named("cornell", kind), 40, 24, bounces, spp, 0, None, 0, None))
    # progressive accumulation: renderedFramesCount > 0 over a random image (:314-318)
    out.append(Case("accumulate_f5", _named("default_dielectric"), 40, 28, 3, 1, 5, 7, 0, None))
    out.append(Case("accumulate_init_f2", _named("reference_init_glass"), 40, 28, 3, 1, 2, 8, 0, None))
    # a row sub-range of a frame, and the smallest frames
    out.append(Case("rows_7_9", _named("cornell"), 48, 32, 3, 1, 1, 9, 7, 9))
    out.append(Case("frame_1x1", _named("cornell"), 1, 1, 3, 2, 0, None, 0, None))
    out.append(Case("frame_9x3", _named("reference_init"), 9, 3, 3, 1, 0, None, 0, None))
    # a NaN slab bound (the min / max choice), on a one-row frame
    out.append(Case("nan_slab", nan_slab_scene, 9, 1, 2, 1, 0, None, 0, None))
    # deeper than the reference's stack: kept out by the guard (DROPPED)
    for levels in (40, 33):
        out.append(Case(f"deep_chain_{levels}", lambda levels=levels: deep_chain_scene(get_scene("default"), levels=levels),
                        40, 24, 2, 1, 0, None, 0, None))
    return out


ALL = {c.id: c for c in _cases()}
# what the stack guard drops (asserted in test_reference_shader.py): the hand-made chains deeper than 32 entries. The
# atrium (27 levels, deepest stack 23 at this size) stays.
DROPPED = ["deep_chain_40", "deep_chain_33"]
KEPT = [k for k in ALL if k not in DROPPED]


@functools.lru_cache(maxsize=None)
def scene_of(case_id):
    return ALL[case_id].scene()


def init_image(case):
    if case.init is None:
        return None
    rows = case.H - case.y0 if case.rows is None else case.rows
    return np.random.default_rng(case.init).random((rows, case.W, 4)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_result(case_id):
    """(image, counters) of the C oracle for a case; the arrays are shared: do not write to them."""
    c = ALL[case_id]
    img, cnt = oracle.render_scene(scene_of(case_id), c.W, c.H, max_bounce=c.bounces, samples=c.spp, frame=c.frame, y0=c.y0,
                                   rows=c.rows, image=init_image(c), threads=4)
    img.setflags(write=False)
    return img, cnt


def reference_library():
    """The compiled reference shaders, or the test's outcome where they are missing: a failure that says "run build()"
    where the reference checkout is present, a skip where it is not."""
    if not os.path.exists(refshader.LIB_PATH):
        if refshader.reference_present():
            pytest.fail(f"{refshader.LIB_PATH} is missing although the reference checkout is present: run build()")
        pytest.skip("no compiled reference shaders (oracle/_ref/) and no reference checkout to build them from")
    return refshader.RefShader()


_ref_images = {}


def reference_result(ref, case_id):
    """The compiled shader's image for a kept case (guarded by the oracle's counters), computed once."""
    if case_id not in _ref_images:
        c = ALL[case_id]
        _, cnt = oracle_result(case_id)
        assert refshader.fits_reference_stack(cnt), f"{case_id} leaves the reference's nodeStack[32]: {cnt}"
        img = ref.render_scene(scene_of(case_id), c.W, c.H, max_bounce=c.bounces, samples=c.spp, frame=c.frame, y0=c.y0,
                               rows=c.rows, image=init_image(c))
        img.setflags(write=False)
        _ref_images[case_id] = img
    return _ref_images[case_id]


def assert_same_bits(got, want, what=""):
    """Every channel of every pixel bit for bit; a NaN must meet a NaN (payloads are not compared)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not differ.any(), f"{what}: {int(differ.any(axis=-1).sum())} of {differ[..., 0].size} pixels differ"


# ---- the display step ------------------------------------------------------------------------------------------------
def hdr_image(width=72, height=40):
    """The synthetic HDR set of test_composite_matches_oracle: noise over every branch of the tonemap, and a row with 0, 1,
    NaN, inf, a negative value and one below the toe."""
    rng = np.random.default_rng(11)
    hdr = np.ones((height, width, 4), np.float32)
    hdr[..., :3] = (rng.random((height, width, 3)) ** 4 * 16.0).astype(np.float32)
    hdr[0, :6, :3] = [[0, 0, 0], [1, 1, 1], [np.nan, 0.5, 0.5], [np.inf, 0, 0], [-1, 0.2, 0.2], [0.05, 0.07, 0.9]]
    return hdr


def bloom_params(threshold=1.0, knee=0.1):
    """bloom.comp's Params as the host forms them once, in binary32."""
    threshold, knee = np.float32(threshold), np.float32(knee)
    return np.array([threshold, threshold - knee, knee * np.float32(2.0), np.float32(0.25) / knee], np.float32)


def reference_bloom_chain(ref, img, sizes, threshold=1.0, knee=0.1):
    """The protocol of DESIGN.md §8 dispatched through the compiled bloom.comp and composite.comp, one dispatch per step:
    (the down levels D, the up levels U, the display image). `sizes` are the levels' (w, h)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    params, n = bloom_params(threshold, knee), len(sizes)
    down = [ref.bloom_dispatch(refshader.MODE_PREFILTER, params, 0, [img], None, *sizes[0])]
    for l in range(1, n):
        down.append(ref.bloom_dispatch(refshader.MODE_DOWNSAMPLE, params, l - 1, down + [None] * (n - l), None, *sizes[l]))
    up = [None] * n
    up[n - 2] = ref.bloom_dispatch(refshader.MODE_UPSAMPLE_FIRST, params, n - 2, down, None, *sizes[n - 2])
    for l in range(n - 3, -1, -1):
        up[l] = ref.bloom_dispatch(refshader.MODE_UPSAMPLE, params, l, down, up, *sizes[l])
    return down, up, ref.composite(img, bloom=up[0])
