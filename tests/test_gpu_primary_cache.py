"""Primary cache (WCPT_OPTION_PRIMARY_CACHE) on the GPU: while camera and scene stand still the megakernel keeps every
pixel's primary Intersect record from the first render after frame 0 and resolves the primary segment of the following
frames from it (pt_kernels.hip launch_megakernel, primary_cache_key.h). Same results, so every sequence here must equal,
bit for bit, the same sequence on a second context with the option off, and where named the oracle's accumulation.

The sequences render **without any upload in between** (an upload bumps the context's generation and with it the key),
and every test asserts the (writes, reads) counts of wcpt_primary_cache_stats it expects, so none can pass with the
cache silently never valid. 52x44 leaves partial 8x8 tiles at both edges.
"""
import copy

import numpy as np
import pytest

import wcpt
import oracle

from test_gpu_parity import _variant, assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 52, 44


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def _scene(name):
    if name in ("two_draws", "empty"):
        return _variant("cornell", name)
    return get_scene(name)


class _Run:
    """One context with the cache on or off, a resident scene and a screen; render() takes what scene_data takes."""

    def __init__(self, s, cache, w=W, h=H, overlap=None):
        self.s, self.w, self.h = s, w, h
        self.ctx = wcpt.Context(0)
        self.ctx.set_option(T.OPTION_PRIMARY_CACHE, 1 if cache else 0)
        if overlap is not None:
            self.ctx.set_option(T.OPTION_FRAME_OVERLAP, overlap)
        self.dev = wcpt.DeviceScene(self.ctx, s)
        self.ctx.create_screen(w, h)

    def sd(self, frame, bounces=3, spp=1):
        return self.s.scene_data(self.w, self.h, max_bounce=bounces, samples=spp, frame=frame)

    def render(self, frame, bounces=3, spp=1, sd=None):
        self.ctx.render(self.sd(frame, bounces, spp) if sd is None else sd, *self.dev.addresses())

    def image(self, rows=None):
        self.ctx.sync()
        return self.ctx.readback(self.h if rows is None else rows)

    def stats(self):
        return self.ctx.primary_cache_stats()

    def close(self):
        self.dev.free()
        self.ctx.close()


def _both(s, body, **kw):
    """body(run) on a context with the cache on and on one with it off; returns (on's result, off's result, on's stats)."""
    out = []
    stats = None
    for cache in (True, False):
        r = _Run(s, cache, **kw)
        try:
            out.append(body(r))
            if cache:
                stats = r.stats()
            else:
                assert r.stats() == (0, 0)
        finally:
            r.close()
    return out[0], out[1], stats


def _assert_equal_lists(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), f"image {i} differs from the cache-off context"


def _oracle_acc(s, w, h, specs, init=None):
    """The oracle's accumulation of the frames specs = [(frame, bounces, spp), ...]."""
    acc = init
    for f, b, spp in specs:
        acc, _ = oracle.render_scene(s, w, h, sd=s.scene_data(w, h, max_bounce=b, samples=spp, frame=f), image=acc,
                                     threads=8)
    return acc


# ---- 1. sequence parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bounces", [("cornell", 4), ("default_dielectric", 3), ("reference_init", 3),
                                          ("two_draws", 3), ("empty", 3)])
def test_sequence_parity(name, bounces):
    """Frames 0..5 (plain, write, read x 4) of a pair-record one-draw scene, spheres and glass, the reference's leaves
    of 1-43 triangles, two draw commands (the 12-byte records) and an empty scene (every record a miss): every frame
    equals the cache-off context's, the last one the oracle's."""
    s = _scene(name)

    def body(r):
        imgs = []
        for f in range(6):
            r.render(f, bounces)
            imgs.append(r.image())
        return imgs

    on, off, stats = _both(s, body)
    _assert_equal_lists(on, off)
    assert stats == (1, 4)
    assert_close(on[-1], _oracle_acc(s, W, H, [(f, bounces, 1) for f in range(6)]))


@pytest.mark.parametrize("name", ["cornell", "default_dielectric"])
def test_sequence_without_frame_zero(name):
    """A start at frame 7 with no frame 0 before it (an accumulation picked up from an uploaded image): write, read,
    read."""
    s = _scene(name)
    init = np.random.default_rng(5).random((H, W, 4), dtype=np.float32)
    init[..., 3] = 1.0

    def body(r):
        r.ctx.image_upload(init)
        imgs = []
        for f in (7, 8, 9):
            r.render(f, 3)
            imgs.append(r.image())
        return imgs

    on, off, stats = _both(s, body)
    _assert_equal_lists(on, off)
    assert stats == (1, 2)
    assert_close(on[-1], _oracle_acc(s, W, H, [(f, 3, 1) for f in (7, 8, 9)], init=init.copy()))


# ---- 2. the primary segment as the last segment; samples ------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "default_dielectric"])
@pytest.mark.parametrize("bounces", [0, 1])
def test_read_frames_with_few_bounces(name, bounces):
    """maxBounceCount 0 (the primary segment is the path's last: the last-segment shortcut right after the record) and
    1 in read frames."""
    s = _scene(name)
    specs = [(f, bounces, 1) for f in range(5)]

    def body(r):
        imgs = []
        for f, b, spp in specs:
            r.render(f, b, spp)
            imgs.append(r.image())
        return imgs

    on, off, stats = _both(s, body)
    _assert_equal_lists(on, off)
    assert stats == (1, 3)
    assert_close(on[-1], _oracle_acc(s, W, H, specs))


@pytest.mark.parametrize("name", ["cornell", "two_draws"])
def test_samples_change_inside_a_sequence(name):
    """samples 1 -> 4 -> 1 and maxBounceCount 3 -> 0 -> 3 inside one sequence: neither is in the key, so the record
    written by a one-sample frame serves the four-sample build (every sample's primary segment) and back."""
    s = _scene(name)
    specs = [(0, 3, 1), (1, 3, 1), (2, 3, 4), (3, 0, 4), (4, 3, 1), (5, 1, 2)]

    def body(r):
        imgs = []
        for f, b, spp in specs:
            r.render(f, b, spp)
            imgs.append(r.image())
        return imgs

    on, off, stats = _both(s, body)
    _assert_equal_lists(on, off)
    assert stats == (1, 4)
    assert_close(on[-1], _oracle_acc(s, W, H, specs))


def test_write_by_the_sample_reuse_build():
    """The record written by a four-sample frame (the sample-reuse build stores it) and read by one-sample frames."""
    s = _scene("default_dielectric")
    specs = [(0, 3, 4), (1, 3, 4), (2, 3, 1), (3, 3, 4)]

    def body(r):
        imgs = []
        for f, b, spp in specs:
            r.render(f, b, spp)
            imgs.append(r.image())
        return imgs

    on, off, stats = _both(s, body)
    _assert_equal_lists(on, off)
    assert stats == (1, 2)
    assert_close(on[-1], _oracle_acc(s, W, H, specs))


# ---- 3. invalidation ------------------------------------------------------------------------------------------------
def _changed_sd(r, field, frame):
    sd = r.sd(frame)
    if field == "position":
        sd["position"][0] += np.float32(0.03125)
    elif field == "inverseView":
        sd["inverseView"][0] *= np.float32(1.0625)
    elif field == "inverseProjection":
        sd["inverseProjection"][5] *= np.float32(0.9375)
    elif field == "sphereCount":
        assert sd["sphereCount"] > 1
        sd["sphereCount"] -= 1
    return sd


INVALIDATIONS = ["position", "inverseView", "inverseProjection", "sphereCount", "sphere_upload", "row_range", "resize",
                 "wavefront", "option"]


@pytest.mark.parametrize("case", INVALIDATIONS)
def test_invalidation(case):
    """Frames 0, 1, 2 (plain, write, read), then one item changes and frame 3 renders without resetting the count: it
    must take the write build, not read the stale records, and equal the cache-off context."""
    s = _scene("cornell")
    rows = 24 if case == "row_range" else None

    def body(r):
        if case == "row_range":
            r.ctx.set_row_range(0, 24)
        for f in range(3):
            r.render(f)
        imgs = [r.image(rows)]
        before = r.stats()
        extra_writes = 1
        if case in ("position", "inverseView", "inverseProjection", "sphereCount"):
            r.render(3, sd=_changed_sd(r, case, 3))
        elif case == "sphere_upload":
            sp = s.spheres.copy()
            sp["position"][:, 1] += np.float32(0.125)
            r.ctx.buffer_upload(r.dev.buffers[1], sp)   # DeviceScene: materials, then spheres
            r.render(3)
        elif case == "row_range":
            r.ctx.set_row_range(8, 24)
            r.render(3)
        elif case == "resize":
            r.ctx.resize(W, 40)
            r.h = 40
            r.render(3)
        elif case == "wavefront":
            r.ctx.set_kernel(wcpt.KERNEL_WAVEFRONT)
            r.render(3)
            r.ctx.set_kernel(wcpt.KERNEL_MEGAKERNEL)
            imgs.append(r.image(rows))
            assert r.stats() == before                   # the wavefront kernel neither writes nor reads
            r.render(4)
        elif case == "option":
            if before != (0, 0):                         # the cache-off context stays off
                r.ctx.set_option(T.OPTION_PRIMARY_CACHE, 0)
                r.ctx.set_option(T.OPTION_PRIMARY_CACHE, 1)
            r.render(3)
        imgs.append(r.image(rows))
        if before != (0, 0):
            assert before == (1, 1)
            assert r.stats() == (1 + extra_writes, 1), f"{case}: frame 3 did not take the write build"
        # ... and the new records serve the frame after
        r.render(5, sd=_changed_sd(r, case, 5))
        imgs.append(r.image(rows))
        if before != (0, 0):
            assert r.stats() == (1 + extra_writes, 2)
        return imgs

    on, off, stats = _both(s, body)
    _assert_equal_lists(on, off)


def test_sphere_upload_changes_the_image():
    """The moved spheres of test_invalidation's upload case do change the frame (so that case can fail)."""
    s = _scene("cornell")
    s2 = copy.copy(s)
    s2.spheres = s.spheres.copy()
    s2.spheres["position"][:, 1] += np.float32(0.125)
    a, _ = oracle.render_scene(s, W, H, max_bounce=0, threads=8)
    b, _ = oracle.render_scene(s2, W, H, max_bounce=0, threads=8)
    assert not np.array_equal(_bits(a), _bits(b))


# ---- 4. forced frame overlap ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("counters_at", [None, 10])
def test_forced_frame_overlap(counters_at):
    """20 consecutive frames of the Cornell box at 128x96 as two pipes (the re-sorts after renders 1, 4 and 16 join and
    fork again), read back only after the whole sequence: equal to the sequence with the cache off and the overlap off;
    also with one counting render in the middle (it joins the pipes and leaves the cache alone)."""
    s = _scene("cornell")
    w, h = 128, 96
    res = {}
    for cache, ov in ((True, 2), (False, 0)):
        r = _Run(s, cache, w, h, overlap=ov)
        try:
            for f in range(20):
                if f == counters_at:
                    cnt = r.ctx.render_counters(r.sd(f, 4), *r.dev.addresses())
                    assert cnt["pixels"] == w * h
                r.render(f, 4)
            res[cache] = r.image()
            if cache:
                assert r.stats() == (1, 18)
        finally:
            r.close()
    assert np.array_equal(_bits(res[True]), _bits(res[False]))


# ---- 5. row blocks and stripes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("stripe", [0, 8])
def test_group_rows_equal_one_context(stripe):
    """A one-process group of 2 ranks on one device (COPY), row blocks and 8-row stripes, 80x72 over 6 frames: each
    rank keeps the records of its own rows (y0, rows and the row map are in the key), and the presented frame equals
    the one-context sequence with the cache off."""
    s = _scene("cornell")
    w, h, frames = 80, 72, range(6)
    fmt = T.PAYLOAD_RGBA32F
    with wcpt.Group([0, 0], root=0, transport=T.GROUP_TRANSPORT_COPY) as g:
        if stripe:
            g.set_option(T.GROUP_OPTION_ROW_STRIPE, stripe)
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(2)]
        g.create_screen(w, h)
        rc = g.context(0)
        nbytes = w * h * T.PAYLOAD_PIXEL_BYTES[fmt]
        out = rc.buffer_from(np.full(nbytes // 4, -5.0, np.float32))
        g.set_output(fmt, rc.buffer_address(out), nbytes)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        for f in frames:
            g.render(s.scene_data(w, h, max_bounce=4, frame=f), *addr)
        g.sync()
        raw = rc.buffer_download(out, nbytes)
        stats = [g.context(r).primary_cache_stats() for r in range(2)]
        rc.buffer_free(out)
        for d in devs:
            d.free()
    assert stats == [(1, 4), (1, 4)]
    one = _Run(s, False, w, h)
    try:
        for f in frames:
            one.render(f, 4)
        ref = one.image()
    finally:
        one.close()
    assert np.array_equal(np.frombuffer(raw, np.uint32).reshape(h, w, 4), _bits(ref))


# ---- 6. counters ----------------------------------------------------------------------------------------------------
def test_counters_in_read_state():
    """wcpt_render_counters on a context whose cache is valid counts every segment the reference traces (the counting
    builds never read the cache), and the next render still reads."""
    s = _scene("cornell")
    r = _Run(s, True)
    try:
        for f in range(3):
            r.render(f, 4)
        assert r.stats() == (1, 1)
        cnt = r.ctx.render_counters(r.sd(3, 4), *r.dev.addresses())
        _, ref = oracle.render_scene(s, W, H, sd=r.sd(3, 4), threads=8)
        assert cnt == ref
        assert r.stats() == (1, 1)
        r.render(3, 4)
        img = r.image()
        assert r.stats() == (1, 2)
    finally:
        r.close()
    assert_close(img, _oracle_acc(s, W, H, [(f, 4, 1) for f in range(4)]))


def test_inactive_without_the_triangle_cache():
    """Active only under the triangle cache's promise: with WCPT_OPTION_TRIANGLE_CACHE = 0 nothing is written or read."""
    s = _scene("cornell")
    r = _Run(s, True)
    try:
        r.ctx.set_option(T.OPTION_TRIANGLE_CACHE, 0)
        for f in range(3):
            r.render(f, 4)
        img = r.image()
        assert r.stats() == (0, 0)
    finally:
        r.close()
    assert_close(img, _oracle_acc(s, W, H, [(f, 4, 1) for f in range(3)]))
