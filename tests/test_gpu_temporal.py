"""Temporal reprojection on the GPU: wcpt_composite_temporal (the HIP kernels of csrc/pt_temporal.hip) against
wcpt_temporal_host, the CPU build of the same arithmetic (csrc/wcpt_temporal.h), which test_temporal_host.py ties to the
numpy restatement: after every call of a chain the destination equals the host chain's output through the host display
step or the host denoise, bit for bit in both formats, with guides that wcpt_trace_primary wrote on the device; and its
behaviour towards the rest of the context (resets, resizes, the frame-overlap pipes, the primary cache, refusals)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import primary_cases
import temporal_cases as tc
import wcpt

pytestmark = pytest.mark.gpu

T = wcpt._lib
REC = T.PRIMARY_HIT_DTYPE.itemsize
F = np.float32


class Sequence:
    """A scene resident on `ctx`, a screen, the records of each camera in a device buffer (traced there) and on the host,
    and the host chain that mirrors the context's temporal state."""

    def __init__(self, ctx, name, width, height, params=None):
        self.ctx, self.s, self.w, self.h = ctx, primary_cases.scene(name), width, height
        self.params = params or wcpt.TemporalParams()
        self.dev = wcpt.DeviceScene(ctx, self.s)
        self.frames = {}
        self.bufs = []
        ctx.create_screen(width, height)
        self.forget()

    def forget(self):
        """The host chain after anything that drops the context's history."""
        self.history = self.state = self.seq = None

    def resize(self, width, height):
        self.w, self.h = width, height
        self.ctx.resize(width, height)
        self.frames = {}
        self.forget()

    def frame(self, move):
        """(guide address, guide bytes, records, scene data) of the camera after `move`."""
        key = (move, self.w, self.h)
        if key not in self.frames:
            sd = self.s.scene_data(self.w, self.h, max_bounce=0, samples=1, frame=0,
                                   camera=tc.moved_camera(self.s.camera, move))
            nbytes = self.w * self.h * REC
            buf = self.ctx.buffer_alloc(nbytes)
            self.bufs.append(buf)
            guide = self.ctx.buffer_address(buf)
            self.ctx.trace_primary(sd, self.dev.spheres, self.dev.draws, guide, nbytes)
            self.ctx.sync()
            rec = np.frombuffer(self.ctx.buffer_download(buf, nbytes), T.PRIMARY_HIT_DTYPE).reshape(self.h, self.w).copy()
            self.frames[key] = (guide, nbytes, rec, sd)
        return self.frames[key]

    def host(self, img, frames, restart, move, denoise=None):
        """The host chain's next call: (rgba32f, rgba8) of what the device call must store."""
        _, _, rec, sd = self.frame(move)
        if restart or self.history is None:
            base, n_b, rgba, length = wcpt.temporal_host(img, frames, rec, sd, self.params, history=self.history)
            self.seq = (rec, sd)
        else:
            base, n_b, rgba, length = wcpt.temporal_host(img, frames, rec, sd, self.params, restart=False, state=self.state)
        self.state = (base, n_b)
        self.history = (rgba, length, self.seq[0], self.seq[1])
        return oracle.composite(rgba) if denoise is None else wcpt.denoise_host(rgba, rec, denoise)

    def device(self, frames, restart, move, rgba8, denoise=None, buf=None):
        """wcpt_composite_temporal of the context's image, downloaded: [H][W][4] float32 or uint8."""
        guide, guide_bytes, _, sd = self.frame(move)
        nbytes = self.w * self.h * (4 if rgba8 else 16)
        own = buf is None
        if own:
            buf = self.ctx.buffer_alloc(nbytes)
        try:
            self.ctx.composite(self.ctx.buffer_address(buf), rgba8=rgba8, temporal=self.params, scene=sd, frames=frames,
                               restart=restart, denoise=denoise, guide=guide, guide_bytes=guide_bytes)
            self.ctx.sync()
            raw = self.ctx.buffer_download(buf, nbytes)
        finally:
            if own:
                self.ctx.buffer_free(buf)
        return np.frombuffer(raw, np.uint8 if rgba8 else np.float32).reshape(self.h, self.w, 4)

    def call_and_check(self, img, frames, restart, move, rgba8, denoise=None, upload=True, what=""):
        if upload:
            self.ctx.image_upload(img)
        ref32, ref8 = self.host(img, frames, restart, move, denoise)
        got = self.device(frames, restart, move, rgba8, denoise)
        if rgba8:
            assert np.array_equal(got, ref8), what
        else:
            tc.assert_same_bits(got, ref32)

    def close(self):
        for b in self.bufs:
            self.ctx.buffer_free(b)
        self.dev.free()


def images(width, height):
    img0 = tc.image(width, height, "special")
    img1 = (img0 * F(0.75) + F(0.125)).astype(F)
    img2 = tc.image(width, height, "noise")[::-1, ::-1].copy()
    img3 = tc.image(width, height, "noise")
    return img0, img1, img2, img3


@pytest.mark.parametrize("rgba8", [False, True], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("name", ["cornell", "every_kind"])
@pytest.mark.parametrize("size", tc.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_composite_temporal_matches_host(gpu_ctx, size, name, rgba8):
    """After every call of the chain the destination equals wcpt_temporal_host followed by the host display step or the host
    denoise, bit for bit: a restart without history; two frames accumulated; the same call again (a re-blend changes
    nothing); a restart with the camera yawed; one with it shifted, through one denoise iteration; one back at the start,
    through three. One pixel, blocks cut at both edges (70x44), several blocks (200x120); HDR noise, the first image with
    0, 25, NaN, inf and negative values, so the first history holds them."""
    q = Sequence(gpu_ctx, name, *size)
    try:
        img0, img1, img2, img3 = images(*size)
        q.call_and_check(img0, 1, True, "still", rgba8, what="restart")
        q.call_and_check(img1, 2, False, "still", rgba8, what="frames 2")
        q.call_and_check(img1, 2, False, "still", rgba8, upload=False, what="frames 2 again")
        q.call_and_check(img2, 1, True, "yaw", rgba8, what="moved restart")
        if size[0] >= 37:
            assert (q.state[1] > 0).sum() > 0.5 * size[0] * size[1]             # the move did find history
        q.call_and_check(img3, 1, True, "shift", rgba8, wcpt.DenoiseParams(1), what="moved restart, denoise 1")
        q.call_and_check(img0, 1, True, "still", rgba8, wcpt.DenoiseParams(3), what="moved restart, denoise 3")
        q.call_and_check(img1, 2, False, "still", rgba8, wcpt.DenoiseParams(3), what="frames 2, denoise 3")
    finally:
        q.close()


def test_composite_temporal_of_rendered_frames(gpu_ctx):
    """Real wcpt_render frames of cornell at 70x44 with the camera moved between the sequences: two accumulated frames
    from the start camera, one from the yawed camera, two from the shifted one."""
    W, H = 70, 44
    q = Sequence(gpu_ctx, "cornell", W, H)
    try:
        for move, count in [("still", 2), ("yaw", 1), ("shift", 2)]:
            cam = tc.moved_camera(q.s.camera, move)
            for frame in range(count):
                gpu_ctx.render(q.s.scene_data(W, H, max_bounce=3, samples=1, frame=frame, camera=cam), *q.dev.addresses())
                gpu_ctx.sync()
                img = gpu_ctx.readback()
                q.call_and_check(img, frame + 1, frame == 0, move, frame == 1, upload=False, what=(move, frame))
        assert (q.state[1] > 0).sum() > 0.5 * W * H
    finally:
        q.close()


def test_reset_and_resize_drop_the_history(gpu_ctx):
    """wcpt_temporal_reset and wcpt_resize make the next call a restart without history, whatever its flag says, as on a
    fresh context; a larger screen afterwards (the scratch grows) and a smaller one (laid out again) work."""
    q = Sequence(gpu_ctx, "cornell", 37, 23)
    try:
        img0, img1, img2, img3 = images(37, 23)
        q.call_and_check(img0, 3, False, "still", False, what="restart == 0 on a fresh screen")
        assert (q.state[1] == 0).all()
        q.call_and_check(img2, 1, True, "yaw", False)
        assert (q.state[1] > 0).any()
        gpu_ctx.temporal_reset()
        q.forget()
        q.call_and_check(img3, 2, False, "shift", True, what="after the reset")
        assert (q.state[1] == 0).all()
        q.call_and_check(img0, 1, True, "still", True)
        for size in [(200, 120), (16, 16)]:
            q.resize(*size)
            a, b, c, _ = images(*size)
            q.call_and_check(a, 1, True, "still", False, what=("after the resize", size))
            assert (q.state[1] == 0).all()
            q.call_and_check(b, 2, False, "still", False)
            q.call_and_check(c, 1, True, "yaw", False, wcpt.DenoiseParams(2))
            assert (q.state[1] > 0).any()
    finally:
        q.close()


def test_composite_temporal_leaves_the_image_and_the_guide(gpu_ctx):
    W, H = 70, 44
    q = Sequence(gpu_ctx, "cornell", W, H)
    try:
        img = tc.image(W, H, "special")
        gpu_ctx.image_upload(img)
        guide, nbytes, rec, _ = q.frame("still")
        q.device(1, True, "still", False)
        q.device(2, False, "still", True, wcpt.DenoiseParams(1))
        q.device(1, True, "still", True)
        assert gpu_ctx.readback().tobytes() == img.tobytes()
        assert gpu_ctx.buffer_download(q.bufs[0], nbytes) == rec.tobytes()
    finally:
        q.close()


def test_the_rest_of_the_context_is_left_alone():
    """render, render, composite_temporal, render: the primary cache's counts, wcpt_last_kernel, wcpt_last_arith and the last
    render's bits are those of the same sequence with wcpt_composite in its place."""
    W, H = 52, 44
    seen = []
    for temporal in (False, True):
        with wcpt.Context(0) as ctx:
            q = Sequence(ctx, "cornell", W, H)
            buf = ctx.buffer_alloc(W * H * 4)
            try:
                guide, nbytes, _, sd0 = q.frame("still")
                for frame in range(3):
                    ctx.render(q.s.scene_data(W, H, max_bounce=3, samples=1, frame=frame), *q.dev.addresses())
                ctx.sync()
                mid = (ctx.primary_cache_stats(), ctx.last_kernel(), ctx.last_arith())
                if temporal:
                    ctx.composite(ctx.buffer_address(buf), rgba8=True, temporal=wcpt.TemporalParams(), scene=sd0, frames=3,
                                  restart=True, guide=guide, guide_bytes=nbytes)
                    ctx.composite(ctx.buffer_address(buf), rgba8=True, temporal=wcpt.TemporalParams(), scene=sd0, frames=3,
                                  restart=True, guide=guide, guide_bytes=nbytes, denoise=wcpt.DenoiseParams(2))
                else:
                    ctx.composite(ctx.buffer_address(buf), rgba8=True)
                ctx.sync()
                assert (ctx.primary_cache_stats(), ctx.last_kernel(), ctx.last_arith()) == mid
                ctx.render(q.s.scene_data(W, H, max_bounce=3, samples=1, frame=3), *q.dev.addresses())
                ctx.sync()
                seen.append((mid, ctx.primary_cache_stats(), ctx.last_kernel(), ctx.readback().tobytes()))
            finally:
                ctx.buffer_free(buf)
                q.close()
    assert seen[0] == seen[1]
    assert seen[0][1][1] > seen[0][0][0][1]          # the render after it still read the cache


def test_composite_temporal_joins_the_overlap_pipes():
    """Six renders back to back with the frame overlap forced on, then the call with no sync in between: it is ordered
    after both pipes, so it equals the host chain on the image after all the frames."""
    W, H = 72, 48
    with wcpt.Context(0) as ctx:
        ctx.set_option(T.OPTION_FRAME_OVERLAP, 2)
        q = Sequence(ctx, "cornell", W, H)
        nbytes = W * H * 16
        buf = ctx.buffer_alloc(nbytes)
        try:
            guide, guide_bytes, _, sd = q.frame("still")
            for frame in range(6):
                ctx.render(q.s.scene_data(W, H, max_bounce=4, samples=1, frame=frame), *q.dev.addresses())
            ctx.composite(ctx.buffer_address(buf), temporal=q.params, scene=sd, frames=6, restart=True, guide=guide,
                          guide_bytes=guide_bytes)
            ctx.sync()
            got = np.frombuffer(ctx.buffer_download(buf, nbytes), F).reshape(H, W, 4)
            tc.assert_same_bits(got, q.host(ctx.readback(), 6, True, "still")[0])
        finally:
            ctx.buffer_free(buf)
            q.close()


REFUSALS = ["row range", "row stripes", "null scene", "null params", "max_history 0", "max_history 65537", "normal_min nan",
            "normal_min > 1", "depth_tol 0", "depth_tol inf", "frames 0", "singular inverseProjection",
            "singular inverseView", "orthographic", "iterations 0", "sigma_depth 0", "null guide", "misaligned guide",
            "short guide", "guide in a short buffer", "null dst", "short dst", "format"]


@pytest.mark.parametrize("what", REFUSALS)
def test_composite_temporal_refusals(what):
    """Each refusal returns WCPT_ERROR_INVALID_ARGUMENT and writes neither the destination nor the accumulation image nor
    the history: the valid call that follows on the same context equals the host chain that never saw the refused call."""
    W, H = 37, 23
    img0, img1, img2, _ = images(W, H)
    nbytes = W * H * 16
    with wcpt.Context(0) as ctx:
        q = Sequence(ctx, "cornell", W, H)
        q.call_and_check(img0, 1, True, "still", False)                        # a history to leave untouched
        buf = ctx.buffer_from(np.full(nbytes // 4, -7.0, F))
        guide, guide_bytes, _, sd = q.frame("yaw")
        sd = np.ascontiguousarray(sd)
        small = ctx.buffer_alloc(guide_bytes - REC)
        dst = ctx.buffer_address(buf)
        t = wcpt.TemporalParams()
        d = None
        fmt, frames, rows = 0, 1, H
        nan, inf = float("nan"), float("inf")
        if what == "row range":
            ctx.set_row_range(4, 8)
            rows = 8
        elif what == "row stripes":
            ctx.set_row_stripes(0, 8, 2, 4)
            rows = 8
        elif what == "max_history 0":
            t = wcpt.TemporalParams(0)
        elif what == "max_history 65537":
            t = wcpt.TemporalParams(65537)
        elif what == "normal_min nan":
            t = wcpt.TemporalParams(32, nan)
        elif what == "normal_min > 1":
            t = wcpt.TemporalParams(32, 1.25)
        elif what == "depth_tol 0":
            t = wcpt.TemporalParams(32, 0.9, 0.0)
        elif what == "depth_tol inf":
            t = wcpt.TemporalParams(32, 0.9, inf)
        elif what == "frames 0":
            frames = 0
        elif what.startswith("singular"):
            m = np.asarray(sd[what.split()[1]]).copy().reshape(4, 4)
            m[1] = m[0]
            sd = sd.copy()
            sd[what.split()[1]] = m.reshape(16)
        elif what == "orthographic":
            proj = np.diag([0.5, 0.5, -0.01, 1.0])
            proj[2, 3] = -1.0
            sd = sd.copy()
            sd["inverseProjection"] = np.linalg.inv(proj).T.reshape(16).astype(F)
        elif what == "iterations 0":
            d = wcpt.DenoiseParams(0)
        elif what == "sigma_depth 0":
            d = wcpt.DenoiseParams(5, 4.0, 0.5, 0.0)
        elif what == "null guide":
            guide = 0
        elif what == "misaligned guide":
            guide += 8
        elif what == "short guide":
            guide_bytes -= 1
        elif what == "guide in a short buffer":
            guide = ctx.buffer_address(small)       # the caller claims more than the buffer holds
        elif what == "null dst":
            dst = 0
        elif what == "short dst":
            dst += 16
        elif what == "format":
            fmt = 2
        if rows != H:                               # a new layout drops the history by itself: the chain starts again
            q.forget()
        ctx.image_upload(img2[:rows])
        rc = wcpt.lib.wcpt_composite_temporal(ctx.h, None if what == "null scene" else sd.ctypes.data, frames, 1, guide,
                                              guide_bytes, dst, fmt, None if what == "null params" else C.byref(t),
                                              None if d is None else C.byref(d))
        assert rc == T.WCPT_ERROR_INVALID_ARGUMENT
        ctx.sync()
        assert (np.frombuffer(ctx.buffer_download(buf, nbytes), F) == -7.0).all()
        assert ctx.readback(rows).tobytes() == img2[:rows].tobytes()
        # back to the whole frame: a call that is no restart still finds the first call's sequence (or, after a new
        # layout, starts one), and a restart its history
        ctx.set_row_range(0, 0) if rows != H else None
        q.call_and_check(img1, 2, False, "still", False, what="the call after the refusal")
        q.call_and_check(img2, 1, True, "yaw", True, wcpt.DenoiseParams(1), what="the restart after the refusal")
        assert (q.state[1] > 0).any()
        ctx.buffer_free(buf)
        ctx.buffer_free(small)
        q.close()


def test_composite_temporal_without_a_screen():
    with wcpt.Context(0) as ctx:
        buf = ctx.buffer_alloc(4096)
        t = wcpt.TemporalParams()
        a = ctx.buffer_address(buf)
        sd = np.ascontiguousarray(primary_cases.scene("cornell").scene_data(8, 8))
        assert wcpt.lib.wcpt_composite_temporal(ctx.h, sd.ctypes.data, 1, 1, a, 4096, a, 0, C.byref(t),
                                                None) == T.WCPT_ERROR_NO_SCREEN
        assert wcpt.lib.wcpt_temporal_reset(ctx.h) == 0
        ctx.buffer_free(buf)


def test_renderer_restarts_the_history_when_the_guide_is_stale():
    """PathTracingRenderer.Composite(..., temporal=...): the call after a frame with moved=True is a restart, the calls over
    still frames are not, a moved sphere keeps the history, changed materials, UpdateMesh and Resize drop it; the output equals the host chain's."""
    s = primary_cases.scene("cornell")
    W, H = 72, 40
    pr = wcpt.PathTracingRenderer(0)
    try:
        pr.Init(scene=s)
        pr.CreateScreen((W, H))
        pr.maxBounceCount = 3
        ed = wcpt.Editor(pr, s.camera)
        buf = pr.ctx.buffer_alloc(W * H * 16)
        dst = pr.ctx.buffer_address(buf)
        params = wcpt.TemporalParams()
        chain = {"history": None, "state": None, "seq": None}
        restarts = []
        inner = pr.ctx.composite

        def recording(*a, **kw):
            restarts.append(bool(kw.get("restart")))
            return inner(*a, **kw)

        pr.ctx.composite = recording

        def composite_and_check(w, h, expect_restart, expect_history):
            cam = wcpt.scene.update_camera(ed.camera, w / h)
            pr.Composite(cam, dst, temporal=params)
            pr.ctx.sync()
            assert restarts[-1] == expect_restart
            got = np.frombuffer(pr.ctx.buffer_download(buf, w * h * 16), F).reshape(h, w, 4)
            sd = pr.scene_data(cam)
            img = pr.Readback()
            if expect_restart:
                rec = pr.ctx.trace_primary(sd, pr.ctx.buffer_address(pr._sph_buf), pr.ctx.buffer_address(pr._draw_buf))
                if not expect_history:
                    chain["history"] = None
                base, n_b, rgba, length = wcpt.temporal_host(img, pr.renderedFramesCount, rec, sd, params,
                                                             history=chain["history"])
                chain["seq"] = (rec, sd)
                assert (n_b > 0).any() == expect_history
            else:
                base, n_b, rgba, length = wcpt.temporal_host(img, pr.renderedFramesCount, chain["seq"][0], sd, params,
                                                             restart=False, state=chain["state"])
            chain["state"] = (base, n_b)
            chain["history"] = (rgba, length, chain["seq"][0], chain["seq"][1])
            tc.assert_same_bits(got, oracle.composite(rgba)[0])

        ed.frame()                                       # start-up: frame 1
        composite_and_check(W, H, True, False)
        ed.frame()
        composite_and_check(W, H, False, False)
        ed.camera.yaw += 1.5
        ed.frame(moved=True)
        composite_and_check(W, H, True, True)
        ed.frame()
        composite_and_check(W, H, False, True)
        pr.spheres["position"][0][0] += 0.05              # a moved sphere keeps the history: the depth test sees to it
        ed.frame(moved=True)
        composite_and_check(W, H, True, True)
        pr.materials["albedo"][1] = (0.1, 0.9, 0.1)       # nothing the records show: the history is dropped
        ed.frame(moved=True)                             # (the editor's frame uploads the materials)
        composite_and_check(W, H, True, False)
        pr.UpdateMesh(0, np.asarray(s.meshes[0].positions, F).reshape(-1, 3) * F(0.98))
        ed.frame(moved=True)
        composite_and_check(W, H, True, False)
        ed.frame(moved=True)
        composite_and_check(W, H, True, True)
        pr.Resize((40, 24))
        ed.frame(moved=True)
        composite_and_check(40, 24, True, False)
        pr.ctx.buffer_free(buf)
    finally:
        pr.Deinit()
