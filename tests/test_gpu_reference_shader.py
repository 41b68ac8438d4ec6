"""The kernels against the reference's own shaders, executed -- not through the oracle. Both render kernels (megakernel and
wavefront) against the compiled pathTracer.comp on every case of tests/ref_cases.py that fits the reference's
nodeStack[32] (dropped by that guard: deep_chain_40, deep_chain_33), and wcpt_composite and wcpt_composite_bloom against
the compiled composite.comp and bloom.comp. Bit patterns of every channel of every pixel, no tolerance; a NaN must meet
a NaN (payloads are not compared: x86 vs AMD).

Only the library built under oracle/_ref/ is loaded; the reference checkout is not read. One ordinary render per test, on
the existing ABI; the compiled shader's image of a case is computed once and shared by both kernels."""
import numpy as np
import pytest

import bloom_cases
import bloom_ref
import ref_cases
import wcpt
from ref_cases import assert_same_bits

pytestmark = pytest.mark.gpu

KERNELS = [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT]


@pytest.fixture(scope="module")
def ref():
    return ref_cases.reference_library()


def device_render(ctx, case, kernel):
    """One wcpt_render of the case, read back: its rows as [rows][W][4]."""
    dev = wcpt.DeviceScene(ctx, ref_cases.scene_of(case.id))
    ctx.set_kernel(kernel)
    try:
        ctx.create_screen(case.W, case.H)
        ctx.set_row_range(case.y0, case.rows or 0)
        init = ref_cases.init_image(case)
        if init is not None:
            ctx.image_upload(init)
        sd = ref_cases.scene_of(case.id).scene_data(case.W, case.H, max_bounce=case.bounces, samples=case.spp,
                                                      frame=case.frame)
        ctx.render(sd, *dev.addresses())
        ctx.sync()
        return ctx.readback(case.rows or case.H)
    finally:
        ctx.set_row_range(0, 0)
        ctx.set_kernel(wcpt.KERNEL_MEGAKERNEL)
        dev.free()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case_id", ref_cases.KEPT)
def test_kernels_match_reference_shader(gpu_ctx, ref, case_id, kernel):
    want = ref_cases.reference_result(ref, case_id)
    got = device_render(gpu_ctx, ref_cases.ALL[case_id], kernel)
    assert gpu_ctx.last_kernel() == kernel
    assert_same_bits(got, want, case_id)


def device_composite(ctx, img, bloom=None):
    """wcpt_composite / wcpt_composite_bloom (rgba32f) of an uploaded image."""
    h, w = img.shape[:2]
    nbytes = w * h * 16
    buf = ctx.buffer_alloc(nbytes)
    try:
        ctx.create_screen(w, h)
        ctx.image_upload(img)
        ctx.composite(ctx.buffer_address(buf), rgba8=False, bloom=bloom)
        ctx.sync()
        return np.frombuffer(ctx.buffer_download(buf, nbytes), np.float32).reshape(h, w, 4)
    finally:
        ctx.buffer_free(buf)


def test_composite_matches_reference_shader(gpu_ctx, ref):
    """wcpt_composite against composite.comp on the synthetic HDR set (0, 1, NaN, inf, negative, every tonemap branch), on
    the 37x23 set with values above 20, and on the shader's own render of the Cornell case."""
    for img in (ref_cases.hdr_image(), bloom_cases.image(37, 23, "special"), ref_cases.reference_result(ref, "cornell")):
        assert_same_bits(device_composite(gpu_ctx, img), ref.composite(img), "wcpt_composite")


@pytest.mark.parametrize("kind", bloom_cases.INPUTS)
@pytest.mark.parametrize("size", [(16, 16), (37, 23), (9, 5), (72, 40)], ids=lambda s: "%dx%d" % s)
def test_composite_bloom_matches_reference_shaders(gpu_ctx, ref, size, kind):
    """wcpt_composite_bloom against bloom.comp's chain and composite.comp's Bloom branch: every ratio 2, odd at every
    level, the minimum with a one-texel level, and several workgroups with four levels."""
    img = bloom_cases.image(*size, kind)
    _, _, want = ref_cases.reference_bloom_chain(ref, img, bloom_ref.level_sizes(*size, 6))
    assert_same_bits(device_composite(gpu_ctx, img, bloom=wcpt.BloomParams()), want, "wcpt_composite_bloom")


def test_composite_bloom_parameters_match_reference_shaders(gpu_ctx, ref):
    img = bloom_cases.image(37, 23, "noise")
    for threshold, knee, levels in [(2.5, 0.1, 6), (1.0, 0.75, 2), (0.0, 0.001, 3)]:
        _, _, want = ref_cases.reference_bloom_chain(ref, img, bloom_ref.level_sizes(37, 23, levels), threshold, knee)
        got = device_composite(gpu_ctx, img, bloom=wcpt.BloomParams(threshold, knee, levels))
        assert_same_bits(got, want, f"wcpt_composite_bloom({threshold}, {knee}, {levels})")
