"""The fast arithmetic mode (WCPT_OPTION_ARITH = WCPT_ARITH_FAST) on the GPU.

The mode is a permission for the megakernel's render launches (pt_device.h kArithFast): fused multiply-adds written out in
the triangle tests and the shading arithmetic, the bare hardware reciprocal and square root, v_log_f32 / v_cos_f32 in
RandomValueNormalDistribution. Everything else -- the wavefront kernels, the counters, the display step -- stays exact.

What is checked:
  1. plumbing: the option's values, wcpt_last_arith, the paths that stay exact;
  2. the exact mode is untouched by a detour through the fast one, and the primary cache is dropped at each change;
  3. the fast image really comes from other code (not every pixel bit-equal to the exact one);
  4. determinism, fast against fast, bit for bit, across everything that changes which pixels share a wave or which
     instantiation runs (no oracle needed);
  5. statistics against the exact CPU oracle. The bounds are not taken from the kernel: the oracle itself rebuilt with
     contraction allowed diverges on up to 0.13 % of a frame's pixels, so (a) at most 0.5 % of the
     pixels diverge, (b) the median of |d| / max(1, |ref|) over the colour channels is <= 1e-6 (a systematic error moves
     every pixel; a flipped path moves a few), (c) finiteness matches;
  6. the fast device functions against the exact ones, within the precision the Vulkan specification grants the
     reference's GLSL.

52x44 leaves partial 8x8 tiles at both edges.
"""
import functools

import numpy as np
import pytest

import wcpt
import oracle
from wcpt import dist

from wcpt import scene as wscene

from test_gpu_parity import _random_scene, _variant, _with_mesh, assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 52, 44
FAST, EXACT = T.ARITH_FAST, T.ARITH_EXACT


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def _scene(name):
    if name in ("two_draws", "all_dielectric", "no_meshes", "empty"):
        return _variant("cornell", name)
    return get_scene(name)


class _Run:
    """One context in an arithmetic mode with a resident scene and a screen."""

    def __init__(self, s, arith=FAST, w=W, h=H, options=()):
        self.s, self.w, self.h = s, w, h
        self.ctx = wcpt.Context(0)
        if arith is not None:
            self.ctx.set_option(T.OPTION_ARITH, arith)
        for opt, val in options:
            self.ctx.set_option(opt, val)
        self.dev = wcpt.DeviceScene(self.ctx, s)
        self.ctx.create_screen(w, h)

    def sd(self, frame, bounces=4, spp=1):
        return self.s.scene_data(self.w, self.h, max_bounce=bounces, samples=spp, frame=frame)

    def render(self, frame, bounces=4, spp=1):
        self.ctx.render(self.sd(frame, bounces, spp), *self.dev.addresses())

    def sequence(self, frames, bounces=4, spp=1):
        for f in frames:
            self.render(f, bounces, spp)
        return self.image()

    def image(self, rows=None):
        self.ctx.sync()
        return self.ctx.readback(self.h if rows is None else rows)

    def close(self):
        self.dev.free()
        self.ctx.close()


def _render(name, arith, frames, bounces, spp=1, w=W, h=H, options=(), check=None):
    r = _Run(_scene(name), arith, w, h, options)
    try:
        img = r.sequence(frames, bounces, spp)
        assert r.ctx.last_arith() == arith
        if check:
            check(r)
        return img
    finally:
        r.close()


@functools.lru_cache(maxsize=None)
def _fast(name, bounces, nframes, spp=1, w=W, h=H):
    """The fast image of frames 0..nframes-1 on a context with default options: computed once, never written to."""
    img = _render(name, FAST, range(nframes), bounces, spp, w, h)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _oracle(name, bounces, nframes, spp=1, w=W, h=H):
    s = _scene(name)
    acc = None
    for f in range(nframes):
        acc, _ = oracle.render_scene(s, w, h, sd=s.scene_data(w, h, max_bounce=bounces, samples=spp, frame=f),
                                     image=acc, threads=8)
    acc.setflags(write=False)
    return acc


def _assert_same(img, ref, what):
    assert img.shape == ref.shape
    differ = int((_bits(img) != _bits(ref)).any(axis=-1).sum())
    assert differ == 0, f"{what}: {differ} of {img.shape[0] * img.shape[1]} pixels differ"


# ---- 1. plumbing ----------------------------------------------------------------------------------------------------
def test_option_values_and_last_arith():
    r = _Run(_scene("cornell"), arith=None)
    try:
        assert r.ctx.last_arith() == EXACT                     # before any render
        r.render(0)
        r.ctx.sync()
        assert r.ctx.last_arith() == EXACT                     # the default
        r.ctx.set_option(T.OPTION_ARITH, FAST)
        for bad in (2, -1):
            with pytest.raises(wcpt.WcptError) as e:
                r.ctx.set_option(T.OPTION_ARITH, bad)
            assert e.value.code == T.WCPT_ERROR_INVALID_ARGUMENT
        img = r.sequence(range(6))
        assert r.ctx.last_arith() == FAST                      # a refused value left the option as it was
        _assert_same(img, _fast("cornell", 4, 6), "fast after refused values")
        r.ctx.set_option(T.OPTION_ARITH, EXACT)
        with pytest.raises(wcpt.WcptError) as e:
            r.ctx.set_option(T.OPTION_ARITH, 2)
        assert e.value.code == T.WCPT_ERROR_INVALID_ARGUMENT
        r.render(0)
        r.ctx.sync()
        assert r.ctx.last_arith() == EXACT
    finally:
        r.close()


def test_wavefront_stays_exact():
    r = _Run(_scene("cornell"), FAST)
    try:
        r.ctx.set_kernel(wcpt.KERNEL_WAVEFRONT)
        img = r.sequence(range(2))
        assert r.ctx.last_kernel() == wcpt.KERNEL_WAVEFRONT
        assert r.ctx.last_arith() == EXACT
    finally:
        r.close()
    assert_close(img, _oracle("cornell", 4, 2), exact=True)


def test_counters_stay_exact():
    s = _scene("cornell")
    got = {}
    for arith in (FAST, EXACT):
        r = _Run(s, arith)
        try:
            r.render(0)
            got[arith] = r.ctx.render_counters(r.sd(1), *r.dev.addresses())
            assert r.ctx.last_arith() == EXACT                 # the counting build has no fast twin
        finally:
            r.close()
    assert set(got[FAST]) == set(got[EXACT])
    for field in got[EXACT]:
        assert got[FAST][field] == got[EXACT][field], field
    assert got[EXACT]["pixels"] == W * H


# ---- 2. exact is untouched ------------------------------------------------------------------------------------------
def test_exact_after_fast_is_exact_and_cache_dropped():
    r = _Run(_scene("cornell"), FAST)
    try:
        fast = r.sequence(range(6))
        assert r.ctx.primary_cache_stats() == (1, 4)
        _assert_same(fast, _fast("cornell", 4, 6), "fast sequence")
        # a change inside a running accumulation: the next render must not read the other arithmetic's records
        r.ctx.set_option(T.OPTION_ARITH, EXACT)
        r.render(6)
        r.ctx.sync()
        assert r.ctx.last_arith() == EXACT
        assert r.ctx.primary_cache_stats() == (2, 4)
        r.ctx.set_option(T.OPTION_ARITH, FAST)
        r.render(7)
        r.ctx.sync()
        assert r.ctx.last_arith() == FAST
        assert r.ctx.primary_cache_stats() == (3, 4)
        # back to exact, accumulation restarted: the oracle's bits
        r.ctx.set_option(T.OPTION_ARITH, EXACT)
        exact = r.sequence(range(6))
        assert r.ctx.last_arith() == EXACT
        assert r.ctx.primary_cache_stats() == (4, 8)
    finally:
        r.close()
    assert_close(exact, _oracle("cornell", 4, 6), exact=True)


# ---- 3. fast is other code ------------------------------------------------------------------------------------------
def test_fast_differs_from_exact():
    fast = _fast("cornell", 4, 1)
    exact = _render("cornell", EXACT, range(1), 4)
    assert_close(exact, _oracle("cornell", 4, 1), exact=True)
    equal = (_bits(fast) == _bits(exact)).all(axis=-1).mean()
    print(f"bit-equal pixels fast / exact: {100 * equal:.2f} %")
    assert equal < 1.0, "the fast render is bit-identical to the exact one: the dispatch ran the exact kernel"


# ---- 4. determinism, fast against fast ------------------------------------------------------------------------------
def test_two_contexts_agree():
    _assert_same(_render("cornell", FAST, range(6), 4), _fast("cornell", 4, 6), "second context")


@pytest.mark.parametrize("order", [0, 1, 3])
def test_tile_orders(order):
    img = _render("cornell", FAST, range(6), 4, options=[(T.OPTION_MK_TILE_ORDER, order)])
    _assert_same(img, _fast("cornell", 4, 6), f"tile order {order} against 2")


def test_stack_kinds():
    img = _render("cornell", FAST, range(6), 4, options=[(T.OPTION_STACK, 0)])
    _assert_same(img, _fast("cornell", 4, 6), "scratch stack against LDS stack")


def test_frame_overlap():
    a = _render("cornell", FAST, range(6), 4, options=[(T.OPTION_FRAME_OVERLAP, 0)])
    b = _render("cornell", FAST, range(6), 4, options=[(T.OPTION_FRAME_OVERLAP, 2)])
    _assert_same(b, a, "overlap 2 against 0")
    _assert_same(a, _fast("cornell", 4, 6), "overlap 0 against the default")


@pytest.mark.parametrize("name,bounces", [("cornell", 4), ("two_draws", 3)])
def test_primary_cache_on_off(name, bounces):
    def on_stats(r):
        assert r.ctx.primary_cache_stats() == (1, 4)

    def off_stats(r):
        assert r.ctx.primary_cache_stats() == (0, 0)

    on = _render(name, FAST, range(6), bounces, options=[(T.OPTION_PRIMARY_CACHE, 1)], check=on_stats)
    off = _render(name, FAST, range(6), bounces, options=[(T.OPTION_PRIMARY_CACHE, 0)], check=off_stats)
    _assert_same(on, off, "primary cache on against off")


def test_sample_reuse_build():
    _assert_same(_render("cornell", FAST, range(1), 4, spp=4), _fast("cornell", 4, 1, 4), "samples=4, second run")


def test_row_range():
    """y0 = 13 is no multiple of 8: the waves hold other pixels than in the whole-frame render."""
    r = _Run(_scene("cornell"), FAST)
    try:
        r.ctx.set_row_range(13, 17)
        for f in range(6):
            r.render(f)
        img = r.image(17)
    finally:
        r.close()
    _assert_same(img, _fast("cornell", 4, 6)[13:30], "rows 13..29")


@pytest.mark.parametrize("rank", [0, 1])
def test_row_stripes(rank):
    stripe, period = 4, 8
    y_first, rows = dist.row_stripes(H, 2, rank, stripe)
    r = _Run(_scene("cornell"), FAST)
    try:
        r.ctx.set_row_stripes(y_first, rows, stripe, period)
        for f in range(6):
            r.render(f)
        img = r.image(rows)
    finally:
        r.close()
    ly = np.arange(rows)
    frame_rows = y_first + ly + (ly // stripe) * (period - stripe)
    assert frame_rows.max() < H and rows == 24 - 4 * rank
    _assert_same(img, _fast("cornell", 4, 6)[frame_rows], f"stripes of rank {rank}")


@pytest.mark.parametrize("fmt", [T.PAYLOAD_RGB32F, T.PAYLOAD_DISPLAY_RGBA8])
def test_gather_output(fmt):
    r = _Run(_scene("cornell"), FAST)
    nbytes = W * H * T.PAYLOAD_PIXEL_BYTES[fmt]
    buf = r.ctx.buffer_from(np.full(nbytes // 4, -7.0, np.float32))
    try:
        r.ctx.set_gather_output(r.ctx.buffer_address(buf), nbytes, fmt)
        img = r.sequence(range(6))
        raw = r.ctx.buffer_download(buf, nbytes)
    finally:
        r.ctx.set_gather_output(0, 0)
        r.ctx.buffer_free(buf)
        r.close()
    _assert_same(img, _fast("cornell", 4, 6), "image beside a gather output")
    if fmt == T.PAYLOAD_RGB32F:
        got = np.frombuffer(raw, np.uint32).reshape(H, W, 3)
        assert np.array_equal(got, _bits(img)[..., :3])
    else:  # the display step is the exact function of the accumulated (fast) value
        got = np.frombuffer(raw, np.uint8).reshape(H, W, 4)
        assert np.array_equal(got, oracle.composite(img)[1])


def test_group_equals_one_context():
    """2 ranks on one device (COPY), fast on both contexts: the presented frame is one fast context's frame."""
    s = _scene("cornell")
    fmt = T.PAYLOAD_RGBA32F
    with wcpt.Group([0, 0], root=0, transport=T.GROUP_TRANSPORT_COPY) as g:
        for rank in range(2):
            g.context(rank).set_option(T.OPTION_ARITH, FAST)
        devs = [wcpt.DeviceScene(g.context(rank), s) for rank in range(2)]
        g.create_screen(W, H)
        rc = g.context(0)
        nbytes = W * H * T.PAYLOAD_PIXEL_BYTES[fmt]
        out = rc.buffer_from(np.full(nbytes // 4, -5.0, np.float32))
        g.set_output(fmt, rc.buffer_address(out), nbytes)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        for f in range(6):
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.sync()
        raw = rc.buffer_download(out, nbytes)
        arith = [g.context(rank).last_arith() for rank in range(2)]
        rc.buffer_free(out)
        for d in devs:
            d.free()
    assert arith == [FAST, FAST]
    _assert_same(np.frombuffer(raw, np.float32).reshape(H, W, 4), _fast("cornell", 4, 6), "presented frame")


# ---- 5. statistics against the exact oracle -------------------------------------------------------------------------
STAT_CASES = [
    ("cornell", 256, 256, 1, 1, 1),
    ("cornell", 128, 96, 4, 1, 1),
    ("cornell", W, H, 4, 6, 1),
    ("default_dielectric", 128, 96, 3, 1, 1),
    ("reference_init", 128, 96, 3, 1, 1),
    ("reference_init", W, H, 3, 6, 1),
    ("two_draws", W, H, 3, 1, 1),
    ("cornell", W, H, 4, 1, 4),
]


@pytest.mark.parametrize("name,w,h,bounces,nframes,spp", STAT_CASES)
def test_statistics_against_the_oracle(name, w, h, bounces, nframes, spp):
    """Measured on the MI355X (diverged pixels / share, mean |d|, bit-equal share; the median is 0 in every case), in the
    order of STAT_CASES: 39 / 0.060 % / 3.5e-4 / 96.8 %; 9 / 0.073 % / 4.4e-4 / 88.3 %; 3 / 0.131 % / 2.0e-4 / 73.5 %;
    8 / 0.065 % / 6.7e-5 / 86.3 %; 8 / 0.065 % / 8.7e-5 / 88.0 %; 6 / 0.262 % / 7.1e-5 / 86.4 %; 3 / 0.131 % / 5.5e-4 /
    89.7 %; 3 / 0.131 % / 1.4e-4 / 72.4 %."""
    _assert_statistics(_fast(name, bounces, nframes, spp, w, h), _oracle(name, bounces, nframes, spp, w, h),
                       f"{name} {w}x{h} b{bounces} x{nframes} spp{spp}")


def _assert_statistics(img, ref, what):
    """(a) at most 0.5 % of the pixels diverge, (b) the median relative difference is <= 1e-6, (c) finiteness matches."""
    assert img.shape == ref.shape
    h, w = img.shape[:2]
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    both = np.isfinite(a) & np.isfinite(b)
    d = np.abs(np.where(both, a, 0.0) - np.where(both, b, 0.0))
    rel = d / np.maximum(1.0, np.where(both, np.abs(b), 1.0))
    close = both & (rel <= 1e-5)
    diverged = int((~close).any(axis=-1).sum())        # includes a finite / non-finite mismatch
    median = float(np.median(rel))
    equal = (_bits(img) == _bits(ref)).all(axis=-1).mean()
    print(f"{what}: diverged {diverged} / {w * h} "
          f"({100.0 * diverged / (w * h):.3f} %), median rel {median:.3g}, mean |d| {d.mean():.3g}, "
          f"bit-equal {100 * equal:.2f} %")
    assert diverged <= 0.005 * w * h, f"(a) {diverged} diverged pixels of {w * h}"
    assert median <= 1e-6, f"(b) median relative difference {median:.3g}"
    assert np.isfinite(ref).all() == np.isfinite(img).all(), "(c) finiteness"
    assert np.array_equal(_bits(img)[..., 3], _bits(ref)[..., 3])      # alpha is 1.0 in both


# ---- 6. device functions --------------------------------------------------------------------------------------------
def _rand_values():
    """Values rand() can produce, (float)k * 2^-32: 0, the smallest, the largest (k = 2^32 - 1 rounds to 1.0), powers of
    two and their neighbours, and a few thousand k spread over the range."""
    rng = np.random.default_rng(18)
    edges = [0, 1, 2, 3, 255, 256, 2**16, 2**24 - 1, 2**24, 2**24 + 1, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1]
    pows = [2**p + o for p in range(2, 32) for o in (-1, 0, 1)]
    k = np.concatenate([np.array(edges + pows, np.uint64), np.linspace(0, 2**32 - 1, 2048).astype(np.uint64),
                        rng.integers(0, 2**32, 2048, dtype=np.uint64),
                        (2.0 ** rng.uniform(0, 32, 1024)).astype(np.uint64)])
    return (k.astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float32)


def _random_normals(rng, n, positive):
    """Normal binary32 numbers whose reciprocal is normal too (biased exponent 2..252): the specification's precision
    holds for results in the normal range, and a denormal result may be flushed."""
    bits = (rng.integers(2, 253, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    if not positive:
        bits |= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    return bits.astype(np.uint32).view(np.float32)


def _f(words):
    return np.asarray(words, np.uint32).view(np.float32)


def _ulp_error(got, ref):
    """|got - ref| in units of ref's last place, over the finite ref; elsewhere the bits must agree."""
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin].view(np.uint32), ref[~fin].view(np.uint32)), "non-finite results differ"
    g, r = got[fin].astype(np.float64), ref[fin].astype(np.float64)
    assert np.isfinite(g).all()
    return np.abs(g - r) / np.spacing(np.abs(ref[fin])).astype(np.float64)


def test_fast_reciprocal(gpu_ctx):
    u = _rand_values()
    x = np.concatenate([u, _random_normals(np.random.default_rng(21), 4096, positive=False)])
    err = _ulp_error(_f(gpu_ctx.selftest(21, x.view(np.uint32))), _f(gpu_ctx.selftest(9, x.view(np.uint32))))
    print(f"fast rcp: max {err.max():.2f} ULP")
    assert err.max() <= 2.5


def test_fast_sqrt(gpu_ctx):
    u = _rand_values()
    x = np.concatenate([u, _random_normals(np.random.default_rng(20), 4096, positive=True)])
    err = _ulp_error(_f(gpu_ctx.selftest(20, x.view(np.uint32))), _f(gpu_ctx.selftest(5, x.view(np.uint32))))
    print(f"fast sqrt: max {err.max():.2f} ULP")
    assert err.max() <= 3.0


def test_fast_log(gpu_ctx):
    u = _rand_values()
    got, ref = _f(gpu_ctx.selftest(18, u.view(np.uint32))), _f(gpu_ctx.selftest(2, u.view(np.uint32)))
    inside = (u >= 0.5) & (u <= 2.0)
    err = _ulp_error(got[~inside], ref[~inside])
    abs_err = np.abs(got[inside].astype(np.float64) - ref[inside].astype(np.float64))
    print(f"fast log: max {err.max():.2f} ULP outside [0.5, 2], max abs {abs_err.max():.3g} inside")
    assert err.max() <= 3.0
    assert abs_err.max() <= 2.0 ** -21


def test_fast_cos(gpu_ctx):
    u = _rand_values()
    theta = (np.float32(2.0) * np.float32(np.pi)) * u          # the exact mode's argument (Random.glsl:34)
    got, ref = _f(gpu_ctx.selftest(19, u.view(np.uint32))), _f(gpu_ctx.selftest(3, theta.view(np.uint32)))
    abs_err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"fast cos: max abs {abs_err.max():.3g}")
    assert np.isfinite(got).all()
    assert abs_err.max() <= 2.0 ** -11


def test_fast_random_direction(gpu_ctx):
    rng = np.random.default_rng(22)
    seeds = np.concatenate([np.arange(64, dtype=np.uint32), rng.integers(0, 2**32, 4032, dtype=np.uint64).astype(np.uint32)])
    got = _f(gpu_ctx.selftest(22, seeds)).reshape(-1, 3).astype(np.float64)
    ref = _f(gpu_ctx.selftest(7, seeds)).reshape(-1, 3).astype(np.float64)
    assert np.array_equal(np.isfinite(got).all(axis=1), np.isfinite(ref).all(axis=1))
    fin = np.isfinite(ref).all(axis=1)
    assert fin.mean() > 0.99
    length = np.abs(np.linalg.norm(got[fin], axis=1) - 1.0)
    dist_ = np.linalg.norm(got[fin] - ref[fin], axis=1)
    print(f"fast RandomDirection: max | |d| - 1 | {length.max():.3g}, max distance to exact {dist_.max():.3g}")
    assert length.max() <= 1e-6
    assert dist_.max() <= 1e-3


# ---- 7. the instantiations the frames above never reach -------------------------------------------------------------
# About 40 fast instantiations exist (stack kind x pair records x single draw x sample reuse x primary-cache mode); the
# Cornell box keeps the traversal stack at three entries and its leaves on pair records. The atrium's 27-level tree spills
# the LDS stack and walks thin leaves on single records. AW x AH leaves partial tiles at the bottom edge.
AW, AH = 96, 54


# -- bit for bit, fast against fast (one helper per formula, so a pixel's bits do not depend on the
# -- instantiation, the stack or the pixels that share its wave)
@pytest.mark.parametrize("option,value", [(T.OPTION_STACK, 0), (T.OPTION_PACKED_REFS, 0), (T.OPTION_MK_TILE_ORDER, 0),
                                          (T.OPTION_MK_TILE_ORDER, 1), (T.OPTION_MK_TILE_ORDER, 3)])
def test_atrium_fast_against_fast(option, value):
    img = _render("atrium", FAST, range(3), 4, w=AW, h=AH, options=[(option, value)])
    _assert_same(img, _fast("atrium", 4, 3, 1, AW, AH), f"option {option} = {value} against the default")


def test_atrium_row_range():
    """y0 = 13 is no multiple of 8: other pixels share a wave, and other tiles a block's neighbourhood."""
    r = _Run(_scene("atrium"), FAST, AW, AH)
    try:
        r.ctx.set_row_range(13, 25)
        for f in range(3):
            r.render(f)
        img = r.image(25)
    finally:
        r.close()
    _assert_same(img, _fast("atrium", 4, 3, 1, AW, AH)[13:38], "rows 13..37")


# -- statistics against the oracle
def _frames(s, sds, w, h, options=(), init=None, prepare=None, arith=FAST):
    """The image after rendering the scene data `sds` in turn on one context (over `init`), and the oracle's."""
    r = _Run(s, arith, w, h, options)
    try:
        if prepare:
            prepare(r)
        if init is not None:
            r.ctx.image_upload(init)
        for sd in sds:
            r.ctx.render(sd, *r.dev.addresses())
        img = r.image()
        assert r.ctx.last_arith() == arith
    finally:
        r.close()
    return img


def _oracle_frames(s, sds, w, h, init=None):
    acc = init
    for sd in sds:
        acc, _ = oracle.render_scene(s, w, h, sd=sd, image=acc, threads=8)
    return acc


def test_statistics_atrium():
    _assert_statistics(_fast("atrium", 4, 3, 1, AW, AH), _oracle("atrium", 4, 3, 1, AW, AH), "atrium 96x54 b4 x3")


@pytest.mark.parametrize("name,option,w,h", [("cornell", T.OPTION_PAIR_RECORDS, W, H), ("atrium", T.OPTION_PAIR_RECORDS, AW, AH),
                                             ("cornell", T.OPTION_TRIANGLE_CACHE, W, H)])
def test_statistics_without_pair_records_or_triangle_cache(name, option, w, h):
    """Single records on both scenes (the fast rayTriangleE), and no derived records at all (the index path)."""
    img = _render(name, FAST, range(3), 4, w=w, h=h, options=[(option, 0)])
    _assert_statistics(img, _oracle(name, 4, 3, 1, w, h), f"{name} option {option} = 0")


def test_statistics_leaf_not_on_triangle_boundary():
    """test_gpu_parity.test_leaf_not_on_triangle_boundary's hand-made BVH: a leaf that starts at index position 1 and a draw
    whose indexCount covers fewer triangles than the leaves reference take the index path (tri_from_indices)."""
    rng = np.random.default_rng(7)
    ntri = 40
    pos = (rng.random((ntri * 3, 3), dtype=np.float32) * 2.0 - 1.0).astype(np.float32)
    pos[:, 2] -= 3.0
    idx = np.arange(ntri * 3 + 2, dtype=np.uint32) % (ntri * 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    nodes = np.zeros(3, dtype=T.NODE_DTYPE)
    nodes[0] = (lo, hi, 1, 0)
    nodes[1] = (lo, hi, 1, 60)
    nodes[2] = (lo, hi, 63, 3 * ntri - 63)
    s = _with_mesh(get_scene("default"), wscene.HostBVH(pos, idx, nodes))

    def short_draw(r):
        draws = np.zeros(1, dtype=T.DRAW_COMMAND_DTYPE)
        b = r.dev.buffers
        draws[0] = (r.ctx.buffer_address(b[2]), r.ctx.buffer_address(b[3]), r.ctx.buffer_address(b[4]), 30, 0)
        r.ctx.buffer_upload(b[5], draws)

    sds = [s.scene_data(AW, AH, max_bounce=2, frame=f) for f in range(2)]
    img = _frames(s, sds, AW, AH, prepare=short_draw)
    exact = _frames(s, sds, AW, AH, prepare=short_draw, arith=EXACT)
    ref = _oracle_frames(s, sds, AW, AH)
    assert_close(exact, ref, exact=True)                     # the same set-up in the exact mode is the oracle's frame
    assert (_bits(img) != _bits(ref)).any()
    _assert_statistics(img, ref, "leaf not on a triangle boundary")


def test_statistics_all_dielectric():
    """Refraction, Fresnel and absorption on every hit, 6 bounces, 2 samples (the sample-reuse build)."""
    _assert_statistics(_fast("all_dielectric", 6, 1, 2), _oracle("all_dielectric", 6, 1, 2), "all_dielectric b6 spp2")


def test_statistics_moved_camera():
    """test_gpu_parity.test_primary_records_follow_the_camera's sequence: the camera moves, moves back, and the mesh is
    uploaded again -- the primary records (whose origin terms the fast mode reads unfused) are rebuilt each time."""
    import ctypes
    s = get_scene("cornell")
    cams = []
    for dx in (0.0, 0.35, 0.0):
        cam = wcpt.Camera()
        ctypes.pointer(cam)[0] = s.camera
        cam.position[0] += dx
        cam.position[1] += dx * 0.5
        cams.append(cam)
    r = _Run(s, FAST, AW, AH, [(T.OPTION_PAIR_RECORDS, 1)])
    try:
        for f, cam in enumerate(cams + [cams[-1]]):
            if f == 3:
                r.ctx.buffer_upload(r.dev.buffers[2], np.ascontiguousarray(s.meshes[0].positions, dtype=np.float32))
            sd = s.scene_data(AW, AH, max_bounce=3, samples=2, frame=0, camera=cam)
            r.ctx.render(sd, *r.dev.addresses())
            img = r.image()
            assert r.ctx.last_arith() == FAST
            ref, _ = oracle.render_scene(s, AW, AH, sd=sd, threads=8)
            _assert_statistics(img, ref, f"camera {f}")
    finally:
        r.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_statistics_random_scenes(seed):
    s, bounces, spp, frame = _random_scene(seed)
    init = np.random.default_rng(seed + 100).random((AH, AW, 4)).astype(np.float32)
    sds = [s.scene_data(AW, AH, max_bounce=bounces, samples=spp, frame=frame)]
    _assert_statistics(_frames(s, sds, AW, AH, init=init), _oracle_frames(s, sds, AW, AH, init=init),
                       f"random scene {seed} b{bounces} spp{spp} frame {frame}")


@pytest.mark.parametrize("frame", [1, 7, 1000])
def test_statistics_progressive_accumulation(frame):
    """One fast frame mixed into a random image with weight 1 / (frame + 1): the accumulation itself is exact arithmetic."""
    s = _scene("cornell")
    init = np.random.default_rng(31).random((H, W, 4)).astype(np.float32)
    sds = [s.scene_data(W, H, max_bounce=4, frame=frame)]
    _assert_statistics(_frames(s, sds, W, H, init=init), _oracle_frames(s, sds, W, H, init=init), f"frame {frame}")


# -- edge inputs
def test_samples_zero():
    """The reference divides by zero samples (:312): NaN colour in both modes, the same alpha."""
    s = _scene("cornell")
    sds = [s.scene_data(W, H, max_bounce=3, samples=0)]
    img, ref = _frames(s, sds, W, H), _oracle_frames(s, sds, W, H)
    assert np.isnan(img[..., :3]).all() and np.isnan(ref[..., :3]).all()
    assert np.array_equal(_bits(img)[..., 3], _bits(ref)[..., 3])


@pytest.mark.parametrize("bounces", [0, 12])
def test_statistics_bounce_counts(bounces):
    _assert_statistics(_fast("cornell", bounces, 1), _oracle("cornell", bounces, 1), f"maxBounceCount {bounces}")


def test_empty_scene_is_exact():
    """Sky only. No relaxed operation reaches a sky pixel: the primary direction and ray_color are exact code in both modes,
    the fast reciprocal of path_begin's invDirection is read by the traversal only, and with no sphere and no draw there
    is none -- so the fast frame is the oracle's, bit for bit."""
    assert_close(_fast("empty", 3, 2), _oracle("empty", 3, 2), exact=True)


def test_statistics_no_meshes():
    """Spheres only. The pixels that see a sphere go through the sphere test's v_sqrt_f32 (raySphereNear stays unfused but
    takes the bare square root) and the fused shading arithmetic, so the frame gets the statistics; its sky pixels (those
    the oracle never lets hit anything) must be the oracle's bits, as in the empty scene."""
    img, ref = _fast("no_meshes", 3, 1), _oracle("no_meshes", 3, 1)
    _assert_statistics(img, ref, "no_meshes")
    sky = _oracle("empty", 3, 1)
    is_sky = (_bits(ref) == _bits(sky)).all(axis=-1)
    assert 0 < is_sky.sum() < W * H
    same = (_bits(img) == _bits(ref)).all(axis=-1)
    assert same[is_sky].mean() >= 0.995, "sky pixels differ"
