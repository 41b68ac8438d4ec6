"""The guided denoise on the GPU: wcpt_composite_denoise (the HIP kernels of csrc/pt_denoise.hip) against
wcpt_denoise_host, the CPU build of the same arithmetic (csrc/wcpt_denoise.h), which test_denoise_host.py ties to the numpy
restatement: bit for bit in both formats, with the guide that wcpt_trace_primary wrote on the device; and its behaviour
towards the rest of the context (the accumulation image, resizes, the frame-overlap pipes, the other display calls, the
primary cache, refusals) and the renderer's guide bookkeeping."""
import ctypes as C

import numpy as np
import pytest

import primary_cases
import wcpt
from wcpt import scene as wscene
from bloom_cases import image as bloom_image
from denoise_cases import GPU_ITERATIONS, GPU_SIZES, assert_same_bits, image

pytestmark = pytest.mark.gpu

T = wcpt._lib
REC = T.PRIMARY_HIT_DTYPE.itemsize


class Guided:
    """A scene resident on `ctx`, a screen, and the frame's records in a device buffer (traced there) and on the host."""

    def __init__(self, ctx, name, width, height):
        self.ctx, self.s, self.w, self.h = ctx, primary_cases.scene(name), width, height
        self.dev = wcpt.DeviceScene(ctx, self.s)
        self.guide_buf = None
        ctx.create_screen(width, height)
        self.trace()

    def sd(self, **kw):
        return self.s.scene_data(self.w, self.h, **kw)

    def trace(self):
        if self.guide_buf is not None:
            self.ctx.buffer_free(self.guide_buf)
        self.nbytes = self.w * self.h * REC
        self.guide_buf = self.ctx.buffer_alloc(self.nbytes)
        self.guide = self.ctx.buffer_address(self.guide_buf)
        self.ctx.trace_primary(self.sd(max_bounce=0, samples=1, frame=0), self.dev.spheres, self.dev.draws, self.guide,
                               self.nbytes)
        self.ctx.sync()
        self.records = np.frombuffer(self.ctx.buffer_download(self.guide_buf, self.nbytes), T.PRIMARY_HIT_DTYPE).reshape(
            self.h, self.w).copy()

    def resize(self, width, height):
        self.w, self.h = width, height
        self.ctx.resize(width, height)
        self.trace()

    def denoise(self, rgba8, params=None, buf=None):
        """wcpt_composite_denoise of the context's image, downloaded: [H][W][4] float32 or uint8."""
        nbytes = self.w * self.h * (4 if rgba8 else 16)
        own = buf is None
        if own:
            buf = self.ctx.buffer_alloc(nbytes)
        try:
            self.ctx.composite(self.ctx.buffer_address(buf), rgba8=rgba8, denoise=params or wcpt.DenoiseParams(),
                               guide=self.guide, guide_bytes=self.nbytes)
            self.ctx.sync()
            raw = self.ctx.buffer_download(buf, nbytes)
        finally:
            if own:
                self.ctx.buffer_free(buf)
        return np.frombuffer(raw, np.uint8 if rgba8 else np.float32).reshape(self.h, self.w, 4)

    def assert_equals_host(self, img, params=None):
        ref32, ref8 = wcpt.denoise_host(img, self.records, params)
        assert_same_bits(self.denoise(False, params), ref32)
        assert np.array_equal(self.denoise(True, params), ref8)

    def close(self):
        self.ctx.buffer_free(self.guide_buf)
        self.dev.free()


@pytest.mark.parametrize("name", ["cornell", "every_kind"])
@pytest.mark.parametrize("size", GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_composite_denoise_matches_host(gpu_ctx, size, name):
    """Device denoise equals the host's bit for bit, rgba32f and RGBA8, at 1, 3 and 6 iterations and with the colour term
    off: one pixel, frames narrower than the steps (9x5, 37x23), blocks cut at both edges (70x44), several blocks with
    every step inside (200x120); HDR noise with a row of 0, 25, NaN, inf and negative values."""
    g = Guided(gpu_ctx, name, *size)
    try:
        if size[0] >= 37:
            assert len(set((g.records["kind"] & 3).ravel())) >= 2          # the frame is cut by identities
        img = image(*size, "special")
        gpu_ctx.image_upload(img)
        for iterations in GPU_ITERATIONS:
            g.assert_equals_host(img, wcpt.DenoiseParams(iterations))
        g.assert_equals_host(img, wcpt.DenoiseParams(3, float("inf")))
        img = image(*size, "noise")
        gpu_ctx.image_upload(img)
        g.assert_equals_host(img, wcpt.DenoiseParams(6))
    finally:
        g.close()


def test_composite_denoise_of_rendered_frame(gpu_ctx):
    """A rendered Cornell frame (72x40, 3 bounces, frame 0): the device denoise equals the host denoise of the readback and
    the downloaded guide, and differs from the plain composite."""
    g = Guided(gpu_ctx, "cornell", 72, 40)
    try:
        gpu_ctx.render(g.sd(max_bounce=3, samples=1, frame=0), *g.dev.addresses())
        gpu_ctx.sync()
        img = gpu_ctx.readback()
        g.assert_equals_host(img)
        nbytes = 72 * 40 * 4
        buf = gpu_ctx.buffer_alloc(nbytes)
        try:
            gpu_ctx.composite(gpu_ctx.buffer_address(buf), rgba8=True)
            gpu_ctx.sync()
            plain = gpu_ctx.buffer_download(buf, nbytes)
        finally:
            gpu_ctx.buffer_free(buf)
        assert g.denoise(True).tobytes() != plain
    finally:
        g.close()


def test_composite_denoise_leaves_the_image(gpu_ctx):
    """The accumulation image and the guide read back identical before and after."""
    W, H = 200, 120
    g = Guided(gpu_ctx, "cornell", W, H)
    try:
        gpu_ctx.image_upload(image(W, H, "special"))
        before = gpu_ctx.readback()
        g.denoise(False)
        g.denoise(True, wcpt.DenoiseParams(1))
        after = gpu_ctx.readback()
        assert before.tobytes() == after.tobytes() == image(W, H, "special").tobytes()
        assert gpu_ctx.buffer_download(g.guide_buf, g.nbytes) == g.records.tobytes()
    finally:
        g.close()


def test_composite_denoise_after_resizes(gpu_ctx):
    """37x23, then 200x120 (the scratch grows), then 16x16 (it is laid out again inside the larger allocation): each result
    equals the host's."""
    g = Guided(gpu_ctx, "cornell", 37, 23)
    try:
        for size in [(37, 23), (200, 120), (16, 16)]:
            g.resize(*size)
            img = image(*size, "noise")
            gpu_ctx.image_upload(img)
            g.assert_equals_host(img)
    finally:
        g.close()


def test_composite_denoise_joins_the_overlap_pipes():
    """Six renders back to back with the frame overlap forced on, then the call with no sync in between: it is ordered
    after both pipes, so it equals the host denoise of the image after all the frames."""
    W, H = 72, 48
    nbytes = W * H * 16
    with wcpt.Context(0) as ctx:
        ctx.set_option(T.OPTION_FRAME_OVERLAP, 2)
        g = Guided(ctx, "cornell", W, H)
        buf = ctx.buffer_alloc(nbytes)
        try:
            for frame in range(6):
                ctx.render(g.sd(max_bounce=4, samples=1, frame=frame), *g.dev.addresses())
            ctx.composite(ctx.buffer_address(buf), denoise=wcpt.DenoiseParams(), guide=g.guide, guide_bytes=g.nbytes)
            ctx.sync()
            got = np.frombuffer(ctx.buffer_download(buf, nbytes), np.float32).reshape(H, W, 4)
            ref32, _ = wcpt.denoise_host(ctx.readback(), g.records)
            assert_same_bits(got, ref32)
        finally:
            ctx.buffer_free(buf)
            g.close()


def test_other_display_calls_are_independent(gpu_ctx):
    """wcpt_composite and wcpt_composite_bloom after a denoise give the bytes they gave before it."""
    W, H = 70, 44
    g = Guided(gpu_ctx, "every_kind", W, H)
    nbytes = W * H * 16
    buf = gpu_ctx.buffer_alloc(nbytes)

    def both():
        out = []
        for bloom in (None, wcpt.BloomParams()):
            gpu_ctx.buffer_upload(buf, np.zeros(nbytes, np.uint8))
            gpu_ctx.composite(gpu_ctx.buffer_address(buf), bloom=bloom)
            gpu_ctx.sync()
            out.append(gpu_ctx.buffer_download(buf, nbytes))
        return out

    try:
        gpu_ctx.image_upload(bloom_image(W, H, "noise"))
        before = both()
        g.denoise(False)
        g.denoise(True)
        assert both() == before and before[0] != before[1]
    finally:
        gpu_ctx.buffer_free(buf)
        g.close()


def test_primary_cache_is_left_alone():
    """A denoise between two still-camera frames: primary_cache_stats and the following render's bits are those of a
    context that made no such call."""
    W, H = 52, 44
    images, stats = [], []
    for call in (False, True):
        with wcpt.Context(0) as ctx:
            g = Guided(ctx, "cornell", W, H)
            buf = ctx.buffer_alloc(W * H * 4)
            try:
                for frame in range(3):
                    ctx.render(g.sd(max_bounce=3, samples=1, frame=frame), *g.dev.addresses())
                ctx.sync()
                mid = ctx.primary_cache_stats()
                if call:
                    ctx.composite(ctx.buffer_address(buf), rgba8=True, denoise=wcpt.DenoiseParams(), guide=g.guide,
                                  guide_bytes=g.nbytes)
                    ctx.sync()
                    assert ctx.primary_cache_stats() == mid
                ctx.render(g.sd(max_bounce=3, samples=1, frame=3), *g.dev.addresses())
                ctx.sync()
                images.append(ctx.readback())
                stats.append((mid, ctx.primary_cache_stats()))
            finally:
                ctx.buffer_free(buf)
                g.close()
    assert stats[0] == stats[1] and stats[0][1][1] > stats[0][0][1]       # the render after it still read the cache
    assert images[0].tobytes() == images[1].tobytes()


@pytest.mark.parametrize("what", ["row range", "row stripes", "null params", "iterations 0", "iterations 7",
                                  "sigma_normal inf", "sigma_depth 0", "sigma_color nan", "null guide", "misaligned guide",
                                  "short guide", "guide in a short buffer", "short dst", "format"])
def test_composite_denoise_refusals(what):
    """Each refusal returns WCPT_ERROR_INVALID_ARGUMENT, writes neither the destination nor the accumulation image, and
    a valid call on the same context afterwards is right."""
    W, H = 37, 23
    img = image(W, H, "noise")
    nbytes = W * H * 16
    with wcpt.Context(0) as ctx:
        g = Guided(ctx, "cornell", W, H)
        buf = ctx.buffer_from(np.full(nbytes // 4, -7.0, np.float32))
        small = ctx.buffer_alloc(g.nbytes - REC)
        dst = ctx.buffer_address(buf)
        guide, guide_bytes = g.guide, g.nbytes
        params = wcpt.DenoiseParams()
        fmt = 0
        rows = H
        if what == "row range":
            ctx.set_row_range(4, 8)
            rows = 8
        elif what == "row stripes":
            ctx.set_row_stripes(0, 8, 2, 4)
            rows = 8
        elif what == "iterations 0":
            params = wcpt.DenoiseParams(0)
        elif what == "iterations 7":
            params = wcpt.DenoiseParams(7)
        elif what == "sigma_normal inf":
            params = wcpt.DenoiseParams(5, 4.0, float("inf"))
        elif what == "sigma_depth 0":
            params = wcpt.DenoiseParams(5, 4.0, 0.5, 0.0)
        elif what == "sigma_color nan":
            params = wcpt.DenoiseParams(5, float("nan"))
        elif what == "null guide":
            guide = 0
        elif what == "misaligned guide":
            guide += 8
        elif what == "short guide":
            guide_bytes -= 1
        elif what == "guide in a short buffer":
            guide = ctx.buffer_address(small)       # the caller claims more than the buffer holds
        elif what == "short dst":
            dst += 16
        elif what == "format":
            fmt = 2
        ctx.image_upload(img[:rows])
        rc = wcpt.lib.wcpt_composite_denoise(ctx.h, guide, guide_bytes, dst, fmt,
                                             None if what == "null params" else C.byref(params))
        assert rc == T.WCPT_ERROR_INVALID_ARGUMENT
        ctx.sync()
        assert (np.frombuffer(ctx.buffer_download(buf, nbytes), np.float32) == -7.0).all()
        assert ctx.readback(rows).tobytes() == img[:rows].tobytes()
        # back to the whole frame: a valid call succeeds and is right
        ctx.set_row_range(0, 0)
        ctx.image_upload(img)
        assert_same_bits(g.denoise(False, buf=buf), wcpt.denoise_host(img, g.records)[0])
        ctx.buffer_free(buf)
        ctx.buffer_free(small)
        g.close()


def test_composite_denoise_without_a_screen():
    with wcpt.Context(0) as ctx:
        buf = ctx.buffer_alloc(4096)
        p = wcpt.DenoiseParams()
        a = ctx.buffer_address(buf)
        assert wcpt.lib.wcpt_composite_denoise(ctx.h, a, 4096, a, 0, C.byref(p)) == T.WCPT_ERROR_NO_SCREEN
        ctx.buffer_free(buf)


def test_renderer_traces_the_guide_only_when_it_is_stale():
    """PathTracingRenderer.Composite(..., denoise=...): the guide is traced on the first call, not again over still frames,
    again after a frame with moved=True, after UpdateMesh and after Resize; the output equals the host's."""
    s = primary_cases.scene("cornell")
    W, H = 72, 40
    pr = wcpt.PathTracingRenderer(0)
    try:
        pr.Init(scene=s)
        pr.CreateScreen((W, H))
        pr.maxBounceCount = 3
        ed = wcpt.Editor(pr, s.camera)
        traces = []
        inner = pr.ctx.trace_primary

        def counting(*a, **kw):
            traces.append(1)
            return inner(*a, **kw)

        pr.ctx.trace_primary = counting
        buf = pr.ctx.buffer_alloc(200 * 120 * 16)
        dst = pr.ctx.buffer_address(buf)
        params = wcpt.DenoiseParams()

        def composite_and_check(w, h):
            cam = wscene.update_camera(s.camera, w / h)
            pr.Composite(cam, dst, denoise=params)
            pr.ctx.sync()
            got = np.frombuffer(pr.ctx.buffer_download(buf, w * h * 16), np.float32).reshape(h, w, 4)
            # the test's own trace goes past the wrapper, so it is not counted
            records = inner(pr.scene_data(cam), pr.ctx.buffer_address(pr._sph_buf), pr.ctx.buffer_address(pr._draw_buf))
            assert_same_bits(got, wcpt.denoise_host(pr.Readback(), records, params)[0])

        ed.frame()                                       # start-up: frame 1
        composite_and_check(W, H)
        assert len(traces) == 1
        for _ in range(3):                               # still frames
            ed.frame()
            composite_and_check(W, H)
        assert len(traces) == 1
        pr.Composite(wscene.update_camera(s.camera, W / H), dst, rgba8=True)   # the plain display step traces nothing
        assert len(traces) == 1
        ed.frame(moved=True)
        composite_and_check(W, H)
        assert len(traces) == 2
        ed.frame()
        composite_and_check(W, H)
        assert len(traces) == 2
        pr.UpdateMesh(0, np.asarray(s.meshes[0].positions, np.float32).reshape(-1, 3) * np.float32(0.98))
        ed.frame(moved=True)
        composite_and_check(W, H)
        assert len(traces) == 3
        pr.Resize((40, 24))
        ed.frame(moved=True)
        composite_and_check(40, 24)
        assert len(traces) == 4
        pr.ctx.buffer_free(buf)
    finally:
        pr.Deinit()
