"""The reference's own compute shaders, compiled for the CPU (test infrastructure only) — ctypes wrapper of
oracle/_ref/libwcpt_ref.so (oracle/ref_driver.cpp; built by `make -C oracle ref` where a checkout of the reference is
present, and by __graft_entry__.build()). Only the library is loaded here; the checkout is never read.

The reference's traversal stack is a real uint[32] in this library: render() must only be given cases for which the
oracle's counters say ref_stack_max <= 32 and ref_stack_overflow_segments == 0 (fits_reference_stack).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libwcpt_ref.so")
REPORT_PATH = os.path.join(HERE, "_ref", "translate_report.txt")
MODE_PREFILTER, MODE_DOWNSAMPLE, MODE_UPSAMPLE_FIRST, MODE_UPSAMPLE = 0, 1, 2, 3


def reference_dir():
    """Where build() looks for the reference checkout: $WCPT_REFERENCE, or a directory `reference` that holds src/shaders
    beside this repository or beside one of the directories above it (the nearest one; beside the repository if none)."""
    if os.environ.get("WCPT_REFERENCE"):
        return os.environ["WCPT_REFERENCE"]
    beside = up = os.path.dirname(os.path.dirname(HERE))
    while True:
        candidate = os.path.join(up, "reference")
        if os.path.isdir(os.path.join(candidate, "src", "shaders")):
            return candidate
        if os.path.dirname(up) == up:
            return os.path.join(beside, "reference")
        up = os.path.dirname(up)


def reference_present():
    return os.path.isdir(os.path.join(reference_dir(), "src", "shaders"))


class _Draw(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("indices", C.c_void_p), ("bvh", C.c_void_p)]


class _Texture(C.Structure):
    _fields_ = [("data", C.c_void_p * 16), ("w", C.c_int * 16), ("h", C.c_int * 16)]


def load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(f"{path} missing: run build() (or `make -C oracle ref`) where the reference checkout is present")
    lib = C.CDLL(path)
    u32, u64, vp, f = C.c_uint32, C.c_uint64, C.c_void_p, C.c_float
    lib.ref_render.restype = None
    lib.ref_render.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, u32, u32]
    lib.ref_composite.restype = None
    lib.ref_composite.argtypes = [vp, vp, u32, u32, u32, u32, vp]
    lib.ref_bloom_dispatch.restype = None
    lib.ref_bloom_dispatch.argtypes = [C.c_int, vp, f, vp, vp, vp, u32, u32]
    lib.ref_pcg_hash.restype = u32
    lib.ref_pcg_hash.argtypes = [u32]
    lib.ref_rand.restype = f
    lib.ref_rand.argtypes = [C.POINTER(u32)]
    lib.ref_random_direction.restype = None
    lib.ref_random_direction.argtypes = [C.POINTER(u32), vp]
    for name, n in (("ref_ray_box", 6), ("ref_ray_sphere", 5), ("ref_ray_triangle", 6), ("ref_reflectance", 5),
                    ("ref_reflect_refract", 4)):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [vp] * n + [u64]
    return lib


class RefShader:
    """The library's calls on numpy arrays. `lib` is a loaded library (load()); the default is the built one."""

    def __init__(self, lib=None):
        self.lib = load() if lib is None else lib

    # ---- pathTracer.comp ---------------------------------------------------------------------------------------------
    def render(self, sd, materials, spheres, meshes, width, height, y0=0, rows=None, image=None):
        """oracle.render's arguments and image convention, through the shader's main."""
        rows = height - y0 if rows is None else rows
        sd = np.ascontiguousarray(sd)
        assert sd.dtype.itemsize == 164
        mats, sph = np.ascontiguousarray(materials), np.ascontiguousarray(spheres)
        keep = []
        draws = (_Draw * max(1, len(meshes)))()
        for i, (pos, idx, nodes) in enumerate(meshes):
            p = np.ascontiguousarray(pos, dtype=np.float32)
            ix = np.ascontiguousarray(idx, dtype=np.uint32)
            nd = np.ascontiguousarray(nodes)
            assert nd.dtype.itemsize == 32
            keep += [p, ix, nd]
            draws[i] = _Draw(p.ctypes.data, ix.ctypes.data, nd.ctypes.data)
        if image is None:
            image = np.zeros((rows, width, 4), np.float32)
        else:
            image = np.ascontiguousarray(image, dtype=np.float32).copy()
            assert image.shape == (rows, width, 4)
        self.lib.ref_render(sd.ctypes.data, mats.ctypes.data if mats.size else None, sph.ctypes.data if sph.size else None,
                            C.addressof(draws), len(meshes), image.ctypes.data, width, height, y0, rows)
        return image

    def render_scene(self, scene, width, height, max_bounce=3, samples=1, frame=0, y0=0, rows=None, image=None, sd=None):
        if sd is None:
            sd = scene.scene_data(width, height, max_bounce=max_bounce, samples=samples, frame=frame)
        meshes = [(m.positions, m.indices, m.nodes) for m in scene.meshes]
        return self.render(sd, scene.materials, scene.spheres, meshes, width, height, y0=y0, rows=rows, image=image)

    # ---- composite.comp and bloom.comp -------------------------------------------------------------------------------
    def composite(self, img, bloom=None):
        """composite.comp on a float4 image [H, W, 4]; bloom: the float4 texture it adds (Bloom set), or None."""
        a = np.ascontiguousarray(img, dtype=np.float32)
        h, w = a.shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        b = None if bloom is None else np.ascontiguousarray(bloom, dtype=np.float32)
        assert b is None or (b.ndim == 3 and b.shape[2] == 4)
        self.lib.ref_composite(a.ctypes.data, None if b is None else b.ctypes.data, 0 if b is None else b.shape[1],
                               0 if b is None else b.shape[0], w, h, out.ctypes.data)
        return out

    @staticmethod
    def _texture(levels, keep):
        t = _Texture()
        for l, a in enumerate(levels):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.ndim == 3 and a.shape[2] == 4
            keep.append(a)
            t.data[l], t.w[l], t.h[l] = a.ctypes.data, a.shape[1], a.shape[0]
        return t

    def bloom_dispatch(self, mode, params, lod, texture, bloom_texture, out_w, out_h):
        """One dispatch of bloom.comp: `texture` / `bloom_texture` are lists of float4 levels (None for a level that the
        dispatch does not read), the result is the (out_h, out_w, 4) image it writes."""
        keep = []
        tex, btex = self._texture(texture, keep), self._texture(bloom_texture or [], keep)
        p = np.ascontiguousarray(params, dtype=np.float32).reshape(4)
        out = np.zeros((out_h, out_w, 4), np.float32)
        self.lib.ref_bloom_dispatch(mode, p.ctypes.data, float(lod), C.addressof(tex), C.addressof(btex), out.ctypes.data,
                                    out_w, out_h)
        return out

    # ---- the shader's functions --------------------------------------------------------------------------------------
    def pcg_hash(self, x):
        return int(self.lib.ref_pcg_hash(x & 0xFFFFFFFF))

    def rand_stream(self, seed, n):
        s = C.c_uint32(seed & 0xFFFFFFFF)
        vals, states = [], []
        for _ in range(n):
            vals.append(self.lib.ref_rand(C.byref(s)))
            states.append(s.value)
        return np.array(vals, np.float32), states

    def random_direction(self, seed):
        s = C.c_uint32(seed & 0xFFFFFFFF)
        out = np.zeros(3, np.float32)
        self.lib.ref_random_direction(C.byref(s), out.ctypes.data)
        return out, s.value

    def _items(self, name, arrays, out_words):
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        n = len(arrays[0])
        out = np.zeros((n, out_words), np.float32)
        getattr(self.lib, name)(*[a.ctypes.data for a in arrays], out.ctypes.data, n)
        return out

    def ray_box(self, o, d, inv, bmin, bmax):
        """rayBoxIntersect on n items ([n, 3] each): (t0, t1) as [n, 2]."""
        return self._items("ref_ray_box", [o, d, inv, bmin, bmax], 2)

    def ray_sphere(self, o, d, c, r):
        return self._items("ref_ray_sphere", [o, d, c, r], 2)

    def ray_triangle(self, o, d, a, b, c):
        """rayTriangleIntersect: (t or -1, u, v) as [n, 3]."""
        return self._items("ref_ray_triangle", [o, d, a, b, c], 3)

    def reflectance(self, i, n, ior_a, ior_b):
        return self._items("ref_reflectance", [i, n, ior_a, ior_b], 1)[:, 0]

    def reflect_refract(self, i, n, eta):
        return self._items("ref_reflect_refract", [i, n, eta], 6)


def fits_reference_stack(counters):
    """Whether a render with these oracle counters stays inside the reference's uint nodeStack[32]."""
    return counters["ref_stack_max"] <= 32 and counters["ref_stack_overflow_segments"] == 0
