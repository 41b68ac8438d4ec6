"""Bloom on the CPU (no GPU): wcpt_bloom_levels and wcpt_bloom_host, the host build of csrc/wcpt_bloom.h, against the
independent numpy restatement of bloom.comp and composite.comp in bloom_ref.py, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import bloom_ref
import oracle
import wcpt
from bloom_cases import INPUTS, SIZES, assert_same_bits, image, pixel_position

INVALID = wcpt._lib.WCPT_ERROR_INVALID_ARGUMENT


@functools.lru_cache(maxsize=None)
def reference(width, height, kind):
    return bloom_ref.bloom(image(width, height, kind))


@pytest.mark.parametrize("frame, requested, expected", [
    ((1920, 1080), 6, [(960, 540), (480, 270), (240, 135), (120, 67), (60, 33), (30, 16)]),
    ((200, 120), 6, [(100, 60), (50, 30), (25, 15), (12, 7), (6, 3), (3, 1)]),
    ((37, 23), 6, [(18, 11), (9, 5), (4, 2), (2, 1)]),
    ((9, 5), 6, [(4, 2), (2, 1)]),
    ((9, 5), 2, [(4, 2), (2, 1)]),
    ((1920, 1080), 12, [(1920 >> l, 1080 >> l) for l in range(1, 11)]),
])
def test_bloom_levels(frame, requested, expected):
    """wcpt_bloom_levels: half resolution and its mips, the request clipped to 1 + floor(log2(min(w_0, h_0)))."""
    assert wcpt.bloom_levels(*frame, requested) == expected
    assert bloom_ref.level_sizes(*frame, requested) == expected


@pytest.mark.parametrize("frame, requested", [((7, 3), 6), ((3, 200), 6), ((1, 1), 2), ((0, 0), 6), ((200, 120), 1),
                                              ((200, 120), 0), ((200, 120), 13)])
def test_bloom_levels_refused(frame, requested):
    """A frame whose clipped level count is below 2 and a request outside 2..12 are refused, the outputs untouched."""
    n = C.c_uint32(77)
    w = (C.c_uint32 * 16)(*[77] * 16)
    h = (C.c_uint32 * 16)(*[77] * 16)
    assert wcpt.lib.wcpt_bloom_levels(*frame, requested, C.byref(n), w, h) == INVALID
    assert n.value == 77 and list(w) == [77] * 16 and list(h) == [77] * 16
    assert wcpt.lib.wcpt_bloom_levels(200, 120, 6, None, w, h) == INVALID
    assert bloom_ref.level_sizes(*frame, requested) is None
    with pytest.raises(wcpt.WcptError):
        wcpt.bloom_levels(*frame, requested)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bloom_host_matches_reference(size, kind):
    """wcpt_bloom_host equals the numpy restatement bit for bit in both formats: HDR noise, noise with a row of 0, > 20,
    NaN, inf and negative values, and one bright pixel on black."""
    img = image(*size, kind)
    got32, got8 = wcpt.bloom_host(img)
    ref32, ref8 = reference(*size, kind)
    assert_same_bits(got32, ref32)
    assert np.array_equal(got8, ref8)
    # either output may be NULL
    only32 = np.empty_like(got32)
    only8 = np.empty_like(got8)
    p = wcpt.BloomParams()
    assert wcpt.lib.wcpt_bloom_host(img.ctypes.data, size[0], size[1], C.byref(p), only32.ctypes.data, None) == 0
    assert wcpt.lib.wcpt_bloom_host(img.ctypes.data, size[0], size[1], C.byref(p), None, only8.ctypes.data) == 0
    assert_same_bits(only32, ref32)
    assert np.array_equal(only8, ref8)


@pytest.mark.parametrize("size", [(37, 23), (200, 120)], ids=lambda s: "%dx%d" % s)
def test_bloom_of_one_pixel_spreads_and_is_asymmetric(size):
    """One pixel of value 50 on black: the glow reaches more than 4 pixels away, and because DownsampleBox13 reads the taps
    (2, 2) and (-2, -2) twice and never (2, -2) or (-2, 2) (bloom.comp:39-46), the response along the diagonal differs
    from the one along the anti-diagonal."""
    x, y = pixel_position(*size)
    got32, _ = wcpt.bloom_host(image(*size, "pixel"))
    black32, _ = oracle.composite(np.zeros((1, 1, 4), np.float32))
    assert not black32[0, 0, :3].any()                       # the display value of black is 0: what is left is bloom
    for d in (5, 6, 8):
        assert got32[y, x + d, 0] > 0 and got32[y, x - d, 0] > 0 and got32[y + d, x, 0] > 0 and got32[y - d, x, 0] > 0
    diagonal = np.array([got32[y + d, x + d, 0] for d in range(1, 9)])
    anti = np.array([got32[y + d, x - d, 0] for d in range(1, 9)])
    assert not np.array_equal(diagonal, anti)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bloom_below_threshold_is_composite(size):
    """A finite image with every channel below threshold - knee: the pyramid is all zeros and the output equals the
    existing oracle's composite of the image bit for bit, in both formats."""
    img = image(*size, "below")
    assert not bloom_ref.pyramid(img).any()
    got32, got8 = wcpt.bloom_host(img)
    ref32, ref8 = oracle.composite(img)
    assert np.array_equal(got32.view(np.uint32), ref32.view(np.uint32))
    assert np.array_equal(got8, ref8)


def test_bloom_parameters_change_the_result():
    """threshold, knee and levels reach the arithmetic: each equals the restatement with the same parameters, and differs
    from the defaults' result."""
    img = image(37, 23, "noise")
    base32, _ = reference(37, 23, "noise")
    for threshold, knee, levels in [(2.5, 0.1, 6), (1.0, 0.75, 6), (1.0, 0.1, 2), (0.0, 0.001, 3)]:
        got32, got8 = wcpt.bloom_host(img, wcpt.BloomParams(threshold, knee, levels))
        ref32, ref8 = bloom_ref.bloom(img, threshold, knee, levels)
        assert_same_bits(got32, ref32)
        assert np.array_equal(got8, ref8)
        assert not np.array_equal(got32, base32)


@pytest.mark.parametrize("what", ["null params", "null image", "nan threshold", "inf threshold", "nan knee", "inf knee",
                                  "knee 0", "knee < 0", "levels 1", "levels 0", "levels 13", "frame 7x3"])
def test_bloom_host_refusals(what):
    """Every refusal returns WCPT_ERROR_INVALID_ARGUMENT and leaves both outputs untouched."""
    width, height = (7, 3) if what == "frame 7x3" else (37, 23)
    img = image(37, 23, "noise")[:height, :width].copy()
    p = {
        "nan threshold": wcpt.BloomParams(float("nan"), 0.1, 6), "inf threshold": wcpt.BloomParams(float("inf"), 0.1, 6),
        "nan knee": wcpt.BloomParams(1.0, float("nan"), 6), "inf knee": wcpt.BloomParams(1.0, float("inf"), 6),
        "knee 0": wcpt.BloomParams(1.0, 0.0, 6), "knee < 0": wcpt.BloomParams(1.0, -0.1, 6),
        "levels 1": wcpt.BloomParams(1.0, 0.1, 1), "levels 0": wcpt.BloomParams(1.0, 0.1, 0),
        "levels 13": wcpt.BloomParams(1.0, 0.1, 13),
    }.get(what, wcpt.BloomParams())
    out32 = np.full((height, width, 4), -7.0, np.float32)
    out8 = np.full((height, width, 4), 7, np.uint8)
    rc = wcpt.lib.wcpt_bloom_host(None if what == "null image" else img.ctypes.data, width, height,
                                  None if what == "null params" else C.byref(p), out32.ctypes.data, out8.ctypes.data)
    assert rc == INVALID
    assert (out32 == -7.0).all() and (out8 == 7).all()
    if what not in ("null params", "null image"):
        with pytest.raises(wcpt.WcptError):
            wcpt.bloom_host(img, p)
    # the same call with valid arguments succeeds
    good = image(37, 23, "noise")
    assert wcpt.lib.wcpt_bloom_host(good.ctypes.data, 37, 23, C.byref(wcpt.BloomParams()), None, None) == 0
