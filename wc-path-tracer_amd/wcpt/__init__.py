"""wcpt — MI355X-native path-tracing compute path (drop-in for pathTracer.comp of myri4/WC-Path-tracer).

The compute lives in libwcpt.so (hand-written HIP for gfx950 behind the C-ABI of include/wcpt.h); this
package is the Python host mirror used by tests and the benchmark.
"""
from ._lib import (BloomParams, DenoiseParams, TemporalParams, COUNTER_FIELDS, DRAW_COMMAND_DTYPE, EXPORTED_SYMBOLS, KERNEL_AUTO, KERNEL_MEGAKERNEL,
                   KERNEL_WAVEFRONT, LIB_PATH, MATERIAL_DIELECTRIC, MATERIAL_DTYPE, MATERIAL_METAL, NODE_DTYPE,
                   SCENE_DATA_DTYPE, SPHERE_DTYPE, PRIMARY_HIT_DTYPE, HIT_MISS, HIT_SPHERE, HIT_TRIANGLE, HIT_KIND_MASK,
                   HIT_FRONT, Camera, WcptError, lib)
from .renderer import Context, DeviceScene, Editor, Group, PathTracingRenderer, group_unique_id
from . import scene
from . import _lib

__all__ = [
    "COUNTER_FIELDS", "DRAW_COMMAND_DTYPE", "EXPORTED_SYMBOLS", "KERNEL_AUTO", "KERNEL_MEGAKERNEL",
    "KERNEL_WAVEFRONT", "LIB_PATH", "MATERIAL_DIELECTRIC", "MATERIAL_DTYPE", "MATERIAL_METAL", "NODE_DTYPE",
    "SCENE_DATA_DTYPE", "SPHERE_DTYPE", "Camera", "WcptError", "lib", "Context", "DeviceScene",
    "PathTracingRenderer", "Editor", "Group", "group_unique_id", "scene", "device_count", "device_pci_bus_id", "runtime_version", "build_id",
    "BloomParams", "bloom_levels", "bloom_host", "DenoiseParams", "denoise_host", "TemporalParams", "temporal_host",
    "PRIMARY_HIT_DTYPE", "HIT_MISS", "HIT_SPHERE", "HIT_TRIANGLE", "HIT_KIND_MASK", "HIT_FRONT",
]


def device_count() -> int:
    import ctypes as C
    n = C.c_int()
    lib.wcpt_device_count(C.byref(n))
    return n.value


def device_pci_bus_id(device: int) -> str:
    """wcpt_device_pci_bus_id: the GPU's PCI bus id, the same in every process whatever its device ordinals."""
    import ctypes as C
    buf = C.create_string_buffer(64)
    _lib.check(lib.wcpt_device_pci_bus_id(device, buf, 64))
    return buf.value.decode()


def build_id() -> str:
    """wcpt_build_id: hash of the library's sources and compile flags (profiles record the build they measured)."""
    return lib.wcpt_build_id().decode()


def runtime_version() -> int:
    """hipRuntimeGetVersion of the HIP runtime libwcpt.so is bound to (e.g. 70226090 = ROCm 7.2)."""
    import ctypes as C
    v = C.c_int()
    _lib.check(lib.wcpt_runtime_version(C.byref(v)))
    return v.value


def bloom_levels(width: int, height: int, requested: int = 6) -> list:
    """wcpt_bloom_levels: the (w, h) of each level of the bloom pyramid of a width x height frame, `requested` levels
    clipped to what the frame admits; raises WcptError where wcpt_composite_bloom would refuse."""
    import ctypes as C
    n = C.c_uint32()
    w = (C.c_uint32 * _lib.BLOOM_MAX_LEVELS)()
    h = (C.c_uint32 * _lib.BLOOM_MAX_LEVELS)()
    _lib.check(lib.wcpt_bloom_levels(width, height, requested, C.byref(n), w, h))
    return [(int(w[i]), int(h[i])) for i in range(n.value)]


def bloom_host(img, params=None):
    """wcpt_bloom_host: what Context.composite(dst, bloom=params) stores for the float4 image `img` [H][W][4], computed
    on the CPU by the same arithmetic (no GPU needed): returns (rgba32f, rgba8)."""
    import numpy as np
    a = np.ascontiguousarray(img, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("bloom_host: an image of shape (height, width, 4)")
    params = BloomParams() if params is None else params
    out32 = np.empty(a.shape, np.float32)
    out8 = np.empty(a.shape, np.uint8)
    import ctypes as C
    _lib.check(lib.wcpt_bloom_host(_lib.ptr(a), a.shape[1], a.shape[0], C.byref(params), _lib.ptr(out32), _lib.ptr(out8)))
    return out32, out8


def denoise_host(img, guide, params=None):
    """wcpt_denoise_host: what Context.composite(dst, denoise=params, guide=...) stores for the float4 image `img`
    [H][W][4] and the primary-hit records `guide` [H][W] (PRIMARY_HIT_DTYPE), computed on the CPU by the same arithmetic
    (no GPU needed): returns (rgba32f, rgba8)."""
    import ctypes as C
    import numpy as np
    a = np.ascontiguousarray(img, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("denoise_host: an image of shape (height, width, 4)")
    g = np.ascontiguousarray(guide, dtype=PRIMARY_HIT_DTYPE)
    if g.shape != a.shape[:2]:
        raise ValueError("denoise_host: one record per pixel, shape (height, width)")
    params = DenoiseParams() if params is None else params
    out32 = np.empty(a.shape, np.float32)
    out8 = np.empty(a.shape, np.uint8)
    _lib.check(lib.wcpt_denoise_host(_lib.ptr(a), _lib.ptr(g), a.shape[1], a.shape[0], C.byref(params), _lib.ptr(out32),
                                     _lib.ptr(out8)))
    return out32, out8


def temporal_host(img, frames, guide, sd, params=None, restart=True, history=None, state=None):
    """wcpt_temporal_host: one call of Context.composite(dst, temporal=params, ...)'s state sequence on the CPU by the same
    arithmetic (no GPU needed), stateless. `img` is the accumulation image [H][W][4] of `frames` samples, `guide` its
    primary-hit records [H][W] and `sd` its scene data. A restart takes `history`, None or (rgba, length, guide, sd) of the
    previous sequence's last call -- that call's outputs with the records and scene data it was given at its restart; any
    other call takes `state` = (base, n_b) as the sequence's restart returned them. Returns (base [H][W][3], n_b [H][W],
    rgba [H][W][4], length [H][W]); rgba is what then goes through the display step or denoise_host."""
    import ctypes as C
    import numpy as np
    a = np.ascontiguousarray(img, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("temporal_host: an image of shape (height, width, 4)")
    h, w = a.shape[:2]
    g = np.ascontiguousarray(guide, dtype=PRIMARY_HIT_DTYPE)
    if g.shape != (h, w):
        raise ValueError("temporal_host: one record per pixel, shape (height, width)")
    s = np.ascontiguousarray(sd, dtype=SCENE_DATA_DTYPE)
    params = TemporalParams() if params is None else params
    hist = [None] * 4
    if restart:
        base, n_b = np.empty((h, w, 3), np.float32), np.empty((h, w), np.float32)
        if history is not None:
            hist = [np.ascontiguousarray(history[0], dtype=np.float32), np.ascontiguousarray(history[1], dtype=np.float32),
                    np.ascontiguousarray(history[2], dtype=PRIMARY_HIT_DTYPE),
                    np.ascontiguousarray(history[3], dtype=SCENE_DATA_DTYPE)]
            if hist[0].shape != a.shape or hist[1].shape != (h, w) or hist[2].shape != (h, w):
                raise ValueError("temporal_host: a history of the image's size")
    else:
        if state is None:
            raise ValueError("temporal_host: a call that is no restart needs the sequence's (base, n_b)")
        base = np.ascontiguousarray(state[0], dtype=np.float32)
        n_b = np.ascontiguousarray(state[1], dtype=np.float32)
        if base.shape != (h, w, 3) or n_b.shape != (h, w):
            raise ValueError("temporal_host: base of shape (height, width, 3), n_b of shape (height, width)")
    out = np.empty(a.shape, np.float32)
    length = np.empty((h, w), np.float32)
    _lib.check(lib.wcpt_temporal_host(_lib.ptr(a), frames, 1 if restart else 0, _lib.ptr(g), _lib.ptr(s), w, h,
                                      C.byref(params), *[None if x is None else _lib.ptr(x) for x in hist], _lib.ptr(base),
                                      _lib.ptr(n_b), _lib.ptr(out), _lib.ptr(length)))
    return base, n_b, out, length
