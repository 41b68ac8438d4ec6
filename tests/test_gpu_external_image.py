"""Rendering into caller-owned memory on the caller's stream: wcpt_set_external_image, wcpt_image_device_ptr and
wcpt_set_stream, the calls through which bench.py's torch path and any host that hands a tensor to RCCL render.

In-process part: the caller's memory is a context buffer allocated larger than declared, its tail filled with a byte
pattern as a guard. 67x45 frames: the 8x8 tiles overhang both edges, so a store past the declared image would land in
the guard. Every result is compared with the oracle's accumulation, bit for bit.

Child-process part (torch imported before wcpt, one spawned process per test): the external image is a torch tensor
and the context renders on a torch stream; the order of the tensor's upload, the renders and its clone on that stream
is what decides the result."""
import json
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import wcpt
import oracle

from bloom_cases import assert_same_bits
from test_gpu_parity import KERNELS, assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H, BOUNCES = 67, 45, 3
N = W * H * 16
GUARD = np.full(8192, 0xA5, np.uint8)            # longer than any overrun a case here could make if its refusal failed
OVERLAP_FORCED = 2                                # as tests/test_gpu_overlap.py forces it


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_acc = {}


def acc(upto, w=W, h=H, first=0, init=None):
    """The oracle's accumulation of cornell frames first..upto of a w x h screen (from `init`: a key and an image)."""
    key = (upto, w, h, first, init[0] if init else None)
    if key not in _acc:
        prev = acc(upto - 1, w, h, first, init) if upto > first else (init[1] if init else None)
        img, _ = oracle.render_scene(get_scene("cornell"), w, h, max_bounce=BOUNCES, frame=upto, image=prev, threads=8)
        img.setflags(write=False)
        _acc[key] = img
    return _acc[key]


def known_image(seed, rows=H):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (rows, W, 4)).astype(np.float32)


class Rig:
    """A context of its own with the Cornell box uploaded, a 67x45 screen, and caller-owned images with guards."""

    def __init__(self, kernel, overlap=None, screen=True):
        self.ctx = wcpt.Context(0)
        self.ctx.set_kernel(kernel)
        if kernel == wcpt.KERNEL_WAVEFRONT and overlap:   # three per-bounce pipelines, as test_gpu_overlap.py sets them
            self.ctx.set_option(T.OPTION_WF_PERSIST, 0)
            self.ctx.set_option(T.OPTION_WF_PIPES, 3)
        if overlap:
            self.ctx.set_option(T.OPTION_FRAME_OVERLAP, overlap)
        self.scene = get_scene("cornell")
        self.dev = wcpt.DeviceScene(self.ctx, self.scene)
        if screen:
            self.ctx.create_screen(W, H)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def caller_image(self, nbytes, fill=None):
        """(buffer, address) of nbytes of caller-owned memory followed by the guard."""
        buf = self.ctx.buffer_alloc(nbytes + GUARD.size)
        self.ctx.buffer_upload(buf, GUARD, offset=nbytes)
        if fill is not None:
            assert fill.nbytes == nbytes
            self.ctx.buffer_upload(buf, fill)
        return buf, self.ctx.buffer_address(buf)

    def guard_intact(self, buf, nbytes):
        return self.ctx.buffer_download(buf, GUARD.size, offset=nbytes) == GUARD.tobytes()

    def image(self, buf, rows=H):
        return np.frombuffer(self.ctx.buffer_download(buf, W * rows * 16), np.float32).reshape(rows, W, 4)

    def render(self, frames, w=W, h=H):
        for f in frames:
            self.ctx.render(self.scene.scene_data(w, h, max_bounce=BOUNCES, frame=f), *self.dev.addresses())


def refused(call, code=T.WCPT_ERROR_INVALID_ARGUMENT):
    with pytest.raises(wcpt.WcptError) as e:
        call()
    assert e.value.code == code


# ---- in-process ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_progressive_frames_into_external_image(kernel):
    """Frames 0, 1, 2 accumulate in the caller's memory (exactly W * rows * 16 bytes declared); image_ptr and readback
    follow it; the context's own image is not written meanwhile and is back, as it was, after the revert; renders after
    the revert leave the caller's memory alone."""
    with Rig(kernel) as r:
        ctx = r.ctx
        own = ctx.image_ptr()
        before = known_image(1)
        ctx.image_upload(before)
        buf, addr = r.caller_image(N)
        ctx.set_external_image(addr, N)
        assert ctx.image_ptr() == addr != own
        r.render((0, 1, 2))
        ctx.sync()
        got = r.image(buf)
        assert_close(got, acc(2), exact=True)
        assert ctx.readback().tobytes() == got.tobytes()
        assert r.guard_intact(buf, N)
        ctx.set_external_image(0, 0)
        assert ctx.image_ptr() == own
        assert ctx.readback().tobytes() == before.tobytes()
        r.render((0, 1))
        ctx.sync()
        assert_close(ctx.readback(), acc(1), exact=True)
        assert r.image(buf).tobytes() == got.tobytes() and r.guard_intact(buf, N)


@pytest.mark.parametrize("kernel", KERNELS)
def test_external_image_is_not_zeroed(kernel):
    """wcpt_create_screen and wcpt_resize zero the context's own image only: the caller's holds its bytes through both,
    and frame 3 blends with them."""
    init = known_image(2)
    with Rig(kernel) as r:
        ctx = r.ctx
        buf, addr = r.caller_image(N, fill=init)
        ctx.set_external_image(addr, N)
        ctx.create_screen(W, H)
        ctx.resize(40, 30)
        ctx.resize(W, H)
        assert r.image(buf).tobytes() == init.tobytes()
        r.render((3,))
        ctx.sync()
        assert_close(r.image(buf), acc(3, first=3, init=("known2", init)), exact=True)
        assert r.guard_intact(buf, N)


@pytest.mark.parametrize("kernel", KERNELS)
def test_external_image_sizes(kernel):
    """One byte too few, no bytes, and a resize the caller's memory cannot hold are WCPT_ERROR_INVALID_ARGUMENT and
    change nothing: the image attached before stays in use, and the old size still renders exactly."""
    with Rig(kernel) as r:
        ctx = r.ctx
        a, addr_a = r.caller_image(N)
        b, addr_b = r.caller_image(N, fill=known_image(3))
        ctx.set_external_image(addr_a, N)
        refused(lambda: ctx.set_external_image(addr_b, N - 1))
        refused(lambda: ctx.set_external_image(addr_b, 0))
        assert ctx.image_ptr() == addr_a
        refused(lambda: ctx.resize(W + 1, H))
        refused(lambda: ctx.resize(W, H + 1))
        assert ctx.image_ptr() == addr_a
        r.render((0, 1))
        ctx.sync()
        assert_close(r.image(a), acc(1), exact=True)
        assert ctx.readback().shape == (H, W, 4)
        assert r.guard_intact(a, N) and r.guard_intact(b, N)
        assert r.image(b).tobytes() == known_image(3).tobytes()


@pytest.mark.parametrize("kernel", KERNELS)
def test_external_image_of_a_row_block_and_of_stripes(kernel):
    """With a row range or row stripes the block's W * rows * 16 bytes suffice, and the guard right behind them stays."""
    with Rig(kernel) as r:
        ctx = r.ctx
        y0, rows = 10, 20
        ctx.set_row_range(y0, rows)
        nb = W * rows * 16
        blk, addr = r.caller_image(nb)
        refused(lambda: ctx.set_external_image(addr, nb - 1))
        ctx.set_external_image(addr, nb)
        r.render((0, 1))
        ctx.sync()
        assert_close(r.image(blk, rows), acc(1)[y0:y0 + rows], exact=True)
        assert r.guard_intact(blk, nb)
        y_first, srows, stripe, period = 3, 16, 4, 12           # frame rows 3..6, 15..18, 27..30, 39..42
        ctx.set_row_stripes(y_first, srows, stripe, period)
        ns = W * srows * 16
        stp, saddr = r.caller_image(ns)
        ctx.set_external_image(saddr, ns)
        r.render((0, 1))
        ctx.sync()
        want = [y_first + ly + (ly // stripe) * (period - stripe) for ly in range(srows)]
        assert_close(r.image(stp, srows), acc(1)[want], exact=True)
        assert r.guard_intact(stp, ns) and r.guard_intact(blk, nb)
        # rows the caller's memory cannot hold are refused and the stripes stay (20 rows would end 4288 bytes past it)
        refused(lambda: ctx.set_row_range(y0, rows))
        r.render((2,))
        ctx.sync()
        assert_close(r.image(stp, srows), acc(2)[want], exact=True)
        assert r.guard_intact(stp, ns)


@pytest.mark.parametrize("kernel", KERNELS)
def test_external_image_before_the_first_screen_then_reverted(kernel):
    with Rig(kernel, screen=False) as r:
        ctx = r.ctx
        fill = known_image(4)
        buf, addr = r.caller_image(N, fill=fill)
        ctx.set_external_image(addr, N)
        assert ctx.image_ptr() == addr
        ctx.set_external_image(0, 0)
        ctx.create_screen(W, H)
        assert ctx.image_ptr() not in (0, addr)
        r.render((0, 1))
        ctx.sync()
        assert_close(ctx.readback(), acc(1), exact=True)
        assert r.image(buf).tobytes() == fill.tobytes() and r.guard_intact(buf, N)


@pytest.mark.parametrize("kernel", KERNELS)
def test_readers_of_an_external_image(kernel):
    """The display step (both formats, plain and with bloom) reads the caller's memory, and the gather payloads written
    beside it (formats 3, 4 and 8) are those of a render into the context's own image."""
    with Rig(kernel) as r:
        ctx = r.ctx
        payloads = {}
        buf, addr = r.caller_image(N)
        pay = ctx.buffer_alloc(N)
        for where in ("own", "external"):
            if where == "external":
                ctx.set_external_image(addr, N)
            for ch in (T.PAYLOAD_RGB32F, T.PAYLOAD_RGBA32F, T.PAYLOAD_DISPLAY_RGBA8):
                nbytes = W * H * T.PAYLOAD_PIXEL_BYTES[ch]
                ctx.buffer_upload(pay, np.zeros(N, np.uint8))
                ctx.set_gather_output(ctx.buffer_address(pay), nbytes, ch)
                r.render((0, 1, 2))
                ctx.sync()
                payloads[where, ch] = ctx.buffer_download(pay, nbytes)
            ctx.set_gather_output(0, 0)
        for ch in (T.PAYLOAD_RGB32F, T.PAYLOAD_RGBA32F, T.PAYLOAD_DISPLAY_RGBA8):
            assert payloads["external", ch] == payloads["own", ch]
        rgb = np.frombuffer(payloads["external", T.PAYLOAD_RGB32F], np.float32).reshape(H, W, 3)
        assert np.array_equal(_bits(rgb), _bits(acc(2)[..., :3]))
        assert_close(r.image(buf), acc(2), exact=True)
        ref32, ref8 = oracle.composite(acc(2))
        bloom32, bloom8 = wcpt.bloom_host(acc(2), wcpt.BloomParams())
        assert (bloom32 != ref32).any()                       # the light blooms: the two references differ
        dst = ctx.buffer_alloc(N)
        for bloom, (want32, want8) in ((None, (ref32, ref8)), (wcpt.BloomParams(), (bloom32, bloom8))):
            for rgba8 in (False, True):
                nbytes = W * H * (4 if rgba8 else 16)
                ctx.composite(ctx.buffer_address(dst), rgba8=rgba8, bloom=bloom)
                ctx.sync()
                raw = ctx.buffer_download(dst, nbytes)
                if rgba8:
                    assert np.array_equal(np.frombuffer(raw, np.uint8).reshape(H, W, 4), want8)
                else:
                    assert_same_bits(np.frombuffer(raw, np.float32).reshape(H, W, 4), want32)
        assert r.guard_intact(buf, N)


@pytest.mark.parametrize("kernel", KERNELS)
def test_overlapped_renders_into_an_external_image(kernel):
    """Frame overlap forced on, the context's own stream: five renders back to back into the caller's memory, then a
    download with no sync between (the download joins the pipes)."""
    with Rig(kernel, overlap=OVERLAP_FORCED) as r:
        buf, addr = r.caller_image(N)
        r.ctx.set_external_image(addr, N)
        r.render(range(5))
        got = r.image(buf)
        assert_close(got, acc(4), exact=True)
        assert r.guard_intact(buf, N)


@pytest.mark.parametrize("kernel", KERNELS)
def test_misaligned_external_image_is_refused(kernel):
    """The kernels store float4 texels: an address that is no multiple of 16 is refused, as wcpt_set_gather_output
    refuses it for RGBA, and nothing is rendered into it."""
    with Rig(kernel) as r:
        ctx = r.ctx
        own = ctx.image_ptr()
        fill = np.full(N + 16, 0x3C, np.uint8)
        buf, addr = r.caller_image(N + 16, fill=fill)
        assert addr % 16 == 0
        for off in (4, 8, 1):
            refused(lambda: ctx.set_external_image(addr + off, N))
        assert ctx.image_ptr() == own
        r.render((0,))
        ctx.sync()
        assert_close(ctx.readback(), acc(0), exact=True)
        assert ctx.buffer_download(buf, N + 16) == fill.tobytes() and r.guard_intact(buf, N + 16)
        ctx.set_external_image(addr + 16, N)                    # any multiple of 16 is fine
        assert ctx.image_ptr() == addr + 16


def test_null_context():
    assert wcpt.lib.wcpt_set_external_image(None, 0, 0) == T.WCPT_ERROR_INVALID_HANDLE
    assert wcpt.lib.wcpt_set_external_image(None, 4096, 4096) == T.WCPT_ERROR_INVALID_HANDLE
    assert wcpt.lib.wcpt_set_stream(None, None) == T.WCPT_ERROR_INVALID_HANDLE
    assert wcpt.lib.wcpt_image_device_ptr(None) == 0


# ---- child processes: a torch tensor on a torch stream ------------------------------------------------------------------
CW, CH = 48, 32
COMBOS = [(k, ov) for k in (wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT) for ov in (0, OVERLAP_FORCED)]


def _child_setup(w, kernel, overlap):
    ctx = w.Context(0)
    ctx.set_kernel(kernel)
    if kernel == w.KERNEL_WAVEFRONT:
        ctx.set_option(w._lib.OPTION_WF_PERSIST, 0)
        ctx.set_option(w._lib.OPTION_WF_PIPES, 3)
    if overlap:
        ctx.set_option(w._lib.OPTION_FRAME_OVERLAP, overlap)
    return ctx


def _sleep_cycles(torch, s, ms):
    """torch.cuda._sleep's argument for about `ms` on stream s: its clock differs between builds, so a million cycles are
    timed first. (The caller measures the delay it really gets.)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record(s)
        torch.cuda._sleep(1_000_000)
        b.record(s)
    s.synchronize()
    return int(ms * 1.0e6 / max(a.elapsed_time(b), 1.0e-3))


STREAMS = 2   # torch streams tried per case: the runtime maps streams onto a few hardware queues (4 by default), and two
              # streams that share one run in submission order whatever the program asked for, which would hide a
              # render on the wrong stream; two streams created in a row do not both share a pipe stream's queue


def _child_callers_stream(rank, init_path, out_path):
    """For each kernel, overlap off and forced, and each of STREAMS torch streams s: on s a delay, then the upload of
    the oracle's frames 0..2 into the tensor, then two renders (frames 3, 4) with no sync, then a clone on s."""
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "wc-path-tracer_amd")]
    import wcpt as w
    from wcpt import scene as wscene
    scene = wscene.generate("cornell")
    init = torch.from_numpy(np.load(init_path)).pin_memory()
    sds = [scene.scene_data(CW, CH, max_bounce=BOUNCES, frame=f) for f in range(5)]
    streams = [torch.cuda.Stream() for _ in range(STREAMS)]
    cycles = _sleep_cycles(torch, streams[0], 30.0)
    out, times = {}, {}
    for kernel, overlap in COMBOS:
        for i, s in enumerate(streams):
            ctx = _child_setup(w, kernel, overlap)
            ctx.set_stream(s.cuda_stream)
            dev = w.DeviceScene(ctx, scene)
            ctx.create_screen(CW, CH)
            shard = torch.zeros((CH, CW, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.set_external_image(shard.data_ptr(), shard.numel() * 4)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            # five renders first: the kernels are loaded, the frame's preparation is cached, the megakernel's tiles are
            # cost-ordered (the overlap's precondition) and its re-sorts after renders 1 and 4, which join the pipes,
            # are behind; the last one is timed. Then the tensor is zeroed, so a render that ran ahead of the upload
            # below would blend with zeros.
            for f in range(5):
                if f == 4:
                    ev[0].record(s)
                ctx.render(sds[f], *dev.addresses())
            ev[1].record(s)
            with torch.cuda.stream(s):
                shard.zero_()
            s.synchronize()
            with torch.cuda.stream(s):
                ev[2].record(s)
                torch.cuda._sleep(cycles)
                ev[3].record(s)
                shard.copy_(init, non_blocking=True)
            ctx.render(sds[3], *dev.addresses())
            ctx.render(sds[4], *dev.addresses())
            with torch.cuda.stream(s):
                got = shard.clone()
            s.synchronize()
            torch.cuda.synchronize()
            key = f"k{kernel}_ov{overlap}_s{i}"
            out[key] = got.cpu().numpy()
            times[key] = {"render_ms": ev[0].elapsed_time(ev[1]), "delay_ms": ev[2].elapsed_time(ev[3])}
            ctx.set_external_image(0, 0)
            ctx.set_stream(None)
            dev.free()
            ctx.close()
    np.savez(out_path, **out)
    with open(out_path + ".json", "w") as f:
        json.dump(times, f)


def test_callers_stream_orders_the_render(gpu_ctx, tmp_path):
    """wcpt_set_stream(s): the renders are ordered on s behind the tensor's upload and before its clone, with no
    wcpt_sync anywhere; WCPT_OPTION_FRAME_OVERLAP forced on is ignored on a caller's stream (render_common), or its
    pipes would start before the upload and end after the clone. The delay in front of the upload must be long against a
    render for the result to say anything: both are measured in the child, printed, and the test fails as inconclusive
    unless delay >= 5 x render."""
    init_path, out_path = str(tmp_path / "init.npy"), str(tmp_path / "out.npz")
    np.save(init_path, acc(2, CW, CH))
    mp.spawn(_child_callers_stream, args=(init_path, out_path), nprocs=1, join=True)
    got = np.load(out_path)
    with open(out_path + ".json") as f:
        times = json.load(f)
    wrong = []
    for kernel, overlap in COMBOS:
        for i in range(STREAMS):
            key = f"k{kernel}_ov{overlap}_s{i}"
            t = times[key]
            same = np.array_equal(_bits(got[key]), _bits(acc(4, CW, CH)))
            print(f"caller's stream {key}: render {t['render_ms']:.3f} ms, delay {t['delay_ms']:.3f} ms, exact {same}")
            assert t["delay_ms"] >= 5.0 * t["render_ms"], f"inconclusive: delay {t['delay_ms']} ms, render {t['render_ms']} ms"
            if not same:
                wrong.append(key)
    assert not wrong, f"not the oracle's accumulation through frame 4: {wrong}"


def _child_own_stream(rank, out_path):
    """A caller's stream, then wcpt_set_stream(None): forced-overlap renders and a readback; then torch's default stream
    handle 0, which selects the context's own stream too: a render, wcpt_sync, a readback."""
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "wc-path-tracer_amd")]
    import wcpt as w
    from wcpt import scene as wscene
    scene = wscene.generate("cornell")
    sds = [scene.scene_data(CW, CH, max_bounce=BOUNCES, frame=f) for f in range(7)]
    out = {}
    for kernel in (w.KERNEL_MEGAKERNEL, w.KERNEL_WAVEFRONT):
        ctx = _child_setup(w, kernel, OVERLAP_FORCED)
        dev = w.DeviceScene(ctx, scene)
        ctx.create_screen(CW, CH)
        s = torch.cuda.Stream()
        ctx.set_stream(s.cuda_stream)
        ctx.render(sds[0], *dev.addresses())
        ctx.set_stream(None)
        for f in range(1, 6):
            ctx.render(sds[f], *dev.addresses())
        out[f"k{kernel}_none"] = ctx.readback()
        assert torch.cuda.default_stream().cuda_stream == 0
        ctx.set_stream(s.cuda_stream)
        ctx.set_stream(torch.cuda.default_stream().cuda_stream)
        ctx.render(sds[6], *dev.addresses())
        ctx.sync()
        out[f"k{kernel}_zero"] = ctx.readback()
        dev.free()
        ctx.close()
    np.savez(out_path, **out)


def test_set_stream_none_and_zero_return_to_the_own_stream(gpu_ctx, tmp_path):
    out_path = str(tmp_path / "own.npz")
    mp.spawn(_child_own_stream, args=(out_path,), nprocs=1, join=True)
    got = np.load(out_path)
    for kernel in KERNELS:
        assert_close(got[f"k{kernel}_none"], acc(5, CW, CH), exact=True)
        assert_close(got[f"k{kernel}_zero"], acc(6, CW, CH), exact=True)
