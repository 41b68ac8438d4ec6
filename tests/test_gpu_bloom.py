"""Bloom on the GPU: wcpt_composite_bloom (the HIP pyramid of csrc/pt_bloom.hip) against wcpt_bloom_host, the CPU build of
the same arithmetic (csrc/wcpt_bloom.h), which test_bloom_host.py ties to the numpy restatement of bloom.comp: bit for
bit in both formats, and its behaviour towards the rest of the context (the accumulation image, a resize, the
frame-overlap pipes, refusals)."""
import ctypes as C
import functools

import numpy as np
import pytest

import wcpt
from bloom_cases import INPUTS, SIZES, assert_same_bits, image
from test_gpu_parity import get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib


@functools.lru_cache(maxsize=None)
def host_reference(width, height, kind):
    return wcpt.bloom_host(image(width, height, kind))


def device_bloom(ctx, rgba8, params=None, buf=None):
    """wcpt_composite_bloom of the context's image, downloaded: [H][W][4] float32 or uint8."""
    W, H = ctx.width, ctx.height
    nbytes = W * H * (4 if rgba8 else 16)
    own = buf is None
    if own:
        buf = ctx.buffer_alloc(nbytes)
    try:
        ctx.composite(ctx.buffer_address(buf), rgba8=rgba8, bloom=params or wcpt.BloomParams())
        ctx.sync()
        raw = ctx.buffer_download(buf, nbytes)
    finally:
        if own:
            ctx.buffer_free(buf)
    return np.frombuffer(raw, np.uint8 if rgba8 else np.float32).reshape(H, W, 4)


def assert_device_equals(ctx, ref32, ref8):
    assert_same_bits(device_bloom(ctx, False), ref32)
    assert np.array_equal(device_bloom(ctx, True), ref8)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_composite_bloom_matches_host(gpu_ctx, size, kind):
    """Device bloom equals the host's bit for bit, rgba32f and RGBA8: every ratio 2 (16x16), odd at every level (37x23),
    the minimum with a level one texel high (9x5), six levels over several workgroups (200x120); HDR noise, a row of 0,
    > 20, NaN, inf and negative values, one bright pixel."""
    gpu_ctx.create_screen(*size)
    gpu_ctx.image_upload(image(*size, kind))
    assert_device_equals(gpu_ctx, *host_reference(*size, kind))


def test_composite_bloom_of_rendered_frame(gpu_ctx):
    """A rendered Cornell frame (72x40, 3 bounces, frame 0): device bloom equals host bloom of the readback, with the
    defaults and with a threshold the room's walls exceed."""
    s = get_scene("cornell")
    W, H = 72, 40
    dev = wcpt.DeviceScene(gpu_ctx, s)
    try:
        gpu_ctx.create_screen(W, H)
        gpu_ctx.render(s.scene_data(W, H, max_bounce=3, samples=1, frame=0), *dev.addresses())
        gpu_ctx.sync()
        img = gpu_ctx.readback()
        assert (img[..., :3] > 1.0).any()                      # the light exceeds the default threshold
        for params in (wcpt.BloomParams(), wcpt.BloomParams(0.25, 0.2, 3)):
            ref32, ref8 = wcpt.bloom_host(img, params)
            assert_same_bits(device_bloom(gpu_ctx, False, params), ref32)
            assert np.array_equal(device_bloom(gpu_ctx, True, params), ref8)
    finally:
        dev.free()


@pytest.mark.parametrize("rgba8", [False, True])
def test_composite_bloom_below_threshold_is_composite(gpu_ctx, rgba8):
    """Every channel below threshold - knee: the bytes wcpt_composite writes."""
    W, H = 37, 23
    nbytes = W * H * (4 if rgba8 else 16)
    buf = gpu_ctx.buffer_alloc(nbytes)
    try:
        gpu_ctx.create_screen(W, H)
        gpu_ctx.image_upload(image(W, H, "below"))
        gpu_ctx.composite(gpu_ctx.buffer_address(buf), rgba8=rgba8)
        gpu_ctx.sync()
        plain = gpu_ctx.buffer_download(buf, nbytes)
        gpu_ctx.buffer_upload(buf, np.zeros(nbytes, np.uint8))
        got = device_bloom(gpu_ctx, rgba8, buf=buf)
        assert got.tobytes() == plain
    finally:
        gpu_ctx.buffer_free(buf)


def test_composite_bloom_after_resize(gpu_ctx):
    """Stale pyramids: bloom at 37x23, then a resize to 200x120 (the pyramids grow), then to 16x16 (they are laid out
    again inside the larger allocation): each result stays equal to the host's."""
    gpu_ctx.create_screen(37, 23)
    for size in [(37, 23), (200, 120), (16, 16)]:
        gpu_ctx.resize(*size)
        gpu_ctx.image_upload(image(*size, "noise"))
        assert_device_equals(gpu_ctx, *host_reference(*size, "noise"))


def test_composite_bloom_leaves_the_image(gpu_ctx):
    """The accumulation image reads back identical before and after a bloom composite."""
    W, H = 200, 120
    gpu_ctx.create_screen(W, H)
    gpu_ctx.image_upload(image(W, H, "special"))
    before = gpu_ctx.readback()
    device_bloom(gpu_ctx, False)
    device_bloom(gpu_ctx, True)
    after = gpu_ctx.readback()
    assert before.tobytes() == after.tobytes() == image(W, H, "special").tobytes()


def test_composite_bloom_joins_the_overlap_pipes():
    """Renders back to back with the frame overlap forced on, then the bloom composite with no sync in between: it is
    ordered after both pipes, so it equals the host bloom of the image after all the frames."""
    s = get_scene("cornell")
    W, H = 72, 48
    nbytes = W * H * 16
    with wcpt.Context(0) as ctx:
        ctx.set_option(T.OPTION_FRAME_OVERLAP, 2)
        dev = wcpt.DeviceScene(ctx, s)
        buf = ctx.buffer_alloc(nbytes)
        try:
            ctx.create_screen(W, H)
            for frame in range(6):
                ctx.render(s.scene_data(W, H, max_bounce=4, samples=1, frame=frame), *dev.addresses())
            ctx.composite(ctx.buffer_address(buf), bloom=wcpt.BloomParams())
            ctx.sync()
            got = np.frombuffer(ctx.buffer_download(buf, nbytes), np.float32).reshape(H, W, 4)
            ref32, _ = wcpt.bloom_host(ctx.readback())
            assert_same_bits(got, ref32)
        finally:
            ctx.buffer_free(buf)
            dev.free()


@pytest.mark.parametrize("what", ["row range", "row stripes", "short dst", "knee 0", "null params", "format", "levels 13",
                                  "nan threshold"])
def test_composite_bloom_refusals(what):
    """Each refusal returns WCPT_ERROR_INVALID_ARGUMENT, writes neither the destination nor the accumulation image, and
    a valid call on the same context still succeeds afterwards."""
    W, H = 37, 23
    img = image(W, H, "noise")
    nbytes = W * H * 16
    with wcpt.Context(0) as ctx:
        ctx.create_screen(W, H)
        buf = ctx.buffer_from(np.full(nbytes // 4, -7.0, np.float32))
        dst = ctx.buffer_address(buf)
        params = wcpt.BloomParams()
        fmt = 0
        rows = H
        if what == "row range":
            ctx.set_row_range(4, 8)
            rows = 8
        elif what == "row stripes":
            ctx.set_row_stripes(0, 8, 2, 4)
            rows = 8
        elif what == "short dst":
            dst += 16
        elif what == "knee 0":
            params = wcpt.BloomParams(1.0, 0.0, 6)
        elif what == "format":
            fmt = 2
        elif what == "levels 13":
            params = wcpt.BloomParams(1.0, 0.1, 13)
        elif what == "nan threshold":
            params = wcpt.BloomParams(float("nan"), 0.1, 6)
        ctx.image_upload(img[:rows])
        rc = wcpt.lib.wcpt_composite_bloom(ctx.h, dst, fmt, None if what == "null params" else C.byref(params))
        assert rc == T.WCPT_ERROR_INVALID_ARGUMENT
        ctx.sync()
        assert (np.frombuffer(ctx.buffer_download(buf, nbytes), np.float32) == -7.0).all()
        assert ctx.readback(rows).tobytes() == img[:rows].tobytes()
        # back to the whole frame: a valid call succeeds and is right
        ctx.set_row_range(0, 0)
        ctx.image_upload(img)
        assert_same_bits(device_bloom(ctx, False, buf=buf), host_reference(W, H, "noise")[0])
        ctx.buffer_free(buf)
