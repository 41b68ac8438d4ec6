"""The sizes, images and guides shared by test_denoise_host.py and test_gpu_denoise.py (test infrastructure; not a test
module). Guides on the CPU are primary_ref.trace of the primary-hit tests' scenes, computed once per (scene, size) and
left unchanged."""
import functools

import numpy as np

import bloom_cases
import primary_cases
import primary_ref

# 1x1: every tap but the centre is outside; 9x5: narrower than step 4's reach; 37x23: every step beyond 8 reaches outside
CPU_SIZES = [(1, 1), (9, 5), (37, 23)]
CPU_ITERATIONS = [1, 3, 5]
GUIDES = ["cornell", "every_kind", "two_draws"]
# on the GPU also 70x44 (32x8 blocks cut at both edges) and 200x120 (several blocks, every step of six inside)
GPU_SIZES = CPU_SIZES + [(70, 44), (200, 120)]
GPU_ITERATIONS = [1, 3, 6]
PROPERTY_SIZE = (70, 44)   # primary_cases.W, H: the frame every_kind's spheres are placed for


def guide(name, width, height):
    """The records [height, width] of scene `name` (read-only, shared)."""
    return primary_ref.reference(name, primary_cases.scene(name), width, height)[0]


@functools.lru_cache(maxsize=None)
def _image(width, height, kind):
    img = bloom_cases.image(width, height, "noise")          # the bloom tests' HDR noise
    if kind == "special" and height > 1:  # a row of 0, 25, NaN, inf and negative values (as far as the frame is wide)
        row = np.array([[0, 0, 0], [25, 30, 1], [np.nan, 0.5, 0.5], [np.inf, 0, 0], [-1, 0.2, 0.2], [0.05, 0.07, 0.9]],
                       np.float32)
        n = min(width, len(row))
        img[1, :n, :3] = row[:n]
    elif kind == "special":
        img[0, 0, :3] = [np.nan, 0.5, 25.0]
    img[..., 3] = np.linspace(0.25, 2.0, width * height, dtype=np.float32).reshape(height, width)   # alpha passes through
    return img


def image(width, height, kind):
    """A fresh copy of the float4 test image [height][width][4]: "noise" or "special"."""
    return _image(width, height, kind).copy()


assert_same_bits = bloom_cases.assert_same_bits


def surfaces(rec):
    """(kind, key) per pixel as one integer array, for telling surfaces apart in a test."""
    kind = (rec["kind"] & 3).astype(np.int64)
    key = np.where(kind == 1, rec["index"], np.where(kind == 2, rec["draw"], 0)).astype(np.int64)
    return kind * (1 << 32) + key
