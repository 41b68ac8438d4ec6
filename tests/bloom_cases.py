"""The sizes and input images shared by test_bloom_host.py and test_gpu_bloom.py (test infrastructure; not a test module)."""
import functools

import numpy as np

# 16x16: every ratio exactly 2; 37x23: odd at every level (general weights, edge clamps); 9x5: the minimum (two levels,
# the last one texel high); 200x120: six levels, several workgroups
SIZES = [(16, 16), (37, 23), (9, 5), (200, 120)]
INPUTS = ["noise", "special", "pixel"]


def pixel_position(width, height):
    """An off-centre pixel (x, y)."""
    return width * 5 // 8, height * 3 // 8


@functools.lru_cache(maxsize=None)
def _image(width, height, kind):
    rng = np.random.default_rng(11)
    img = np.ones((height, width, 4), np.float32)
    if kind == "pixel":       # one pixel of value 50 on black
        img[..., :3] = 0.0
        x, y = pixel_position(width, height)
        img[y, x, :3] = 50.0
        return img
    img[..., :3] = (rng.random((height, width, 3)) ** 4 * 16.0).astype(np.float32)   # the composite test's HDR noise
    if kind == "special":     # one row with 0, > 20, NaN, inf and negative values
        img[1, :6, :3] = [[0, 0, 0], [25, 30, 1], [np.nan, 0.5, 0.5], [np.inf, 0, 0], [-1, 0.2, 0.2], [0.05, 0.07, 0.9]]
    elif kind == "below":     # finite, every channel below threshold - knee of the defaults (0.9), a few negative
        img[..., :3] = (rng.random((height, width, 3)) * 0.875).astype(np.float32)
        img[0, :3, :3] = [[-1, 0.2, 0.2], [0, 0, 0], [-0.5, -0.25, -2]]
    return img


def image(width, height, kind):
    """A fresh copy of the float4 test image [height][width][4]."""
    return _image(width, height, kind).copy()


def assert_same_bits(got32, ref32):
    """Bit equality of float images; NaN positions must agree, NaN payloads are not compared (x86 vs AMD)."""
    nan = np.isnan(ref32)
    assert np.array_equal(np.isnan(got32), nan)
    assert np.array_equal(got32.view(np.uint32)[~nan], ref32.view(np.uint32)[~nan])
