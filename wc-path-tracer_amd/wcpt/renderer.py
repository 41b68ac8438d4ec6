"""Device context and the host-side mirror of the reference renderer, over the C-ABI (libwcpt.so).

:class:`Context` is a thin 1:1 wrapper of the C entry points. :class:`PathTracingRenderer` mirrors the Jai
procedures of src/PathTracingRenderer.jai (Init :272, CreateScreen :345, Resize :393, Render :399,
UpdateMaterials :459, Deinit :473, PushMaterial :492) with the same names, fields and frame-counter
sequencing, so that a test reads like driving the reference editor (src/editor.jai:60-80,155-158).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (COUNTER_FIELDS, DRAW_COMMAND_DTYPE, GROUP_OPTION_ROW_STRIPE, GROUP_TRANSPORT_RCCL,
                   GROUP_UNIQUE_ID_BYTES, ARITH_EXACT, OPTION_ARITH, OPTION_DIAGNOSTICS,
                   HIT_KIND_MASK, HIT_SPHERE, MATERIAL_DTYPE, NODE_DTYPE, PRIMARY_HIT_DTYPE, SCENE_DATA_DTYPE, SPHERE_DTYPE, Camera, Counters, GroupInfo, WcptError, WfPlanInfo, check, lib, ptr)
from . import scene as _scene


class Context:
    """One HIP device context (one stream). Not thread-safe, like the reference's single render thread."""

    def __init__(self, device: int = 0, _handle=None):
        self.owned = _handle is None
        if _handle is None:
            h = C.c_void_p()
            check(lib.wcpt_create(device, C.byref(h)))
            _handle = h
        self.h = _handle
        self.device = device

    @classmethod
    def borrowed(cls, handle, device: int) -> "Context":
        """A context owned by someone else (a Group's rank context): close() leaves it alone."""
        return cls(device, _handle=C.c_void_p(handle))

    # -- lifetime -----------------------------------------------------------------------------------
    def close(self):
        if self.h and self.owned:
            lib.wcpt_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        return check(rc, self.h)

    # -- configuration -------------------------------------------------------------------------------
    def set_kernel(self, variant: int):
        self._chk(lib.wcpt_set_kernel(self.h, variant))

    def last_kernel(self) -> int:
        """The variant the last render ran (WCPT_KERNEL_AUTO resolved per render)."""
        v = C.c_int()
        self._chk(lib.wcpt_last_kernel(self.h, C.byref(v)))
        return v.value

    def last_arith(self) -> int:
        """The arithmetic the last render ran (ARITH_FAST only after a megakernel render with OPTION_ARITH set to it)."""
        v = C.c_int()
        self._chk(lib.wcpt_last_arith(self.h, C.byref(v)))
        return v.value

    def set_option(self, option: int, value: int):
        self._chk(lib.wcpt_set_option(self.h, option, value))

    def set_stream(self, stream_handle: int | None):
        self._chk(lib.wcpt_set_stream(self.h, stream_handle or None))

    # -- buffers ---------------------------------------------------------------------------------------
    def buffer_alloc(self, nbytes: int) -> int:
        out = C.c_uint64()
        self._chk(lib.wcpt_buffer_alloc(self.h, nbytes, C.byref(out)))
        return out.value

    def buffer_upload(self, buf: int, arr: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(arr)
        self._chk(lib.wcpt_buffer_upload(self.h, buf, ptr(a) if a.nbytes else None, a.nbytes, offset))

    def buffer_download(self, buf: int, nbytes: int, offset: int = 0) -> bytes:
        out = np.empty(nbytes, np.uint8)
        self._chk(lib.wcpt_buffer_download(self.h, buf, ptr(out), nbytes, offset))
        return out.tobytes()

    def buffer_size(self, buf: int) -> int:
        out = C.c_uint64()
        self._chk(lib.wcpt_buffer_size(self.h, buf, C.byref(out)))
        return out.value

    def buffer_address(self, buf: int) -> int:
        a = lib.wcpt_buffer_device_address(self.h, buf)
        if a == 0 and self.buffer_size(buf) > 0:
            raise WcptError(-1001, lib.wcpt_last_error(self.h).decode())
        return a

    def buffer_free(self, buf: int):
        self._chk(lib.wcpt_buffer_free(self.h, buf))

    def buffer_from(self, arr: np.ndarray) -> int:
        a = np.ascontiguousarray(arr)
        b = self.buffer_alloc(max(a.nbytes, 0))
        if a.nbytes:
            self.buffer_upload(b, a)
        return b

    def bvh_build_device(self, vb: int, vertex_count: int, ib: int, index_count: int, nb: int,
                         builder: str = "midpoint") -> int:
        """wcpt_bvh_build_device: the midpoint BVH of the index buffer `ib` over the vertex buffer `vb`, built on the
        device into the node buffer `nb` (at least 2 * index_count / 3 nodes), `ib` permuted in place -- the bytes of
        wcpt_bvh_build. With builder="sah", wcpt_bvh_build_sah_device: the bytes of wcpt_bvh_build_sah. Returns the
        node count."""
        if builder not in ("midpoint", "sah"):
            raise ValueError(f"unknown BVH builder {builder!r}")
        fn = lib.wcpt_bvh_build_device if builder == "midpoint" else lib.wcpt_bvh_build_sah_device
        used = C.c_uint32()
        self._chk(fn(self.h, vb, vertex_count, ib, index_count, nb, C.byref(used)))
        return used.value

    def bvh_refit_device(self, vb: int, vertex_count: int, ib: int, index_count: int, nb: int, nodes_used: int):
        """wcpt_bvh_refit_device: the boxes of the first `nodes_used` nodes of `nb` recomputed on the device from the
        vertex buffer's current contents -- the bytes of wcpt_bvh_refit; the tree's shape and `ib` are not written."""
        self._chk(lib.wcpt_bvh_refit_device(self.h, vb, vertex_count, ib, index_count, nb, nodes_used))

    # -- image ----------------------------------------------------------------------------------------
    def create_screen(self, width: int, height: int):
        self._chk(lib.wcpt_create_screen(self.h, width, height))
        self.width, self.height = width, height

    def resize(self, width: int, height: int):
        self._chk(lib.wcpt_resize(self.h, width, height))
        self.width, self.height = width, height

    def set_row_range(self, y0: int, rows: int):
        self._chk(lib.wcpt_set_row_range(self.h, y0, rows))

    def set_row_stripes(self, y_first: int, rows: int, stripe: int, period: int):
        """Interleaved stripes (wcpt_set_row_stripes): `rows` rows, stripes of `stripe` rows every `period` rows from
        frame row y_first, stored back to back."""
        self._chk(lib.wcpt_set_row_stripes(self.h, y_first, rows, stripe, period))

    def set_external_image(self, device_ptr: int, nbytes: int):
        self._chk(lib.wcpt_set_external_image(self.h, device_ptr, nbytes))

    def set_gather_output(self, device_ptr: int, nbytes: int, channels: int = 3):
        """The render also writes each pixel into its payload at device_ptr (0 = off): channels = 3 / 4 (float RGB /
        RGBA of the accumulation) or 8 (PAYLOAD_DISPLAY_RGBA8: composite.comp's display value as RGBA8)."""
        self._chk(lib.wcpt_set_gather_output(self.h, device_ptr, nbytes, channels))

    def image_ptr(self) -> int:
        return lib.wcpt_image_device_ptr(self.h)

    def readback(self, rows: int | None = None) -> np.ndarray:
        rows = self.height if rows is None else rows
        out = np.empty((rows, self.width, 4), np.float32)
        self._chk(lib.wcpt_readback(self.h, ptr(out), out.nbytes))
        return out

    def image_upload(self, img: np.ndarray):
        a = np.ascontiguousarray(img, dtype=np.float32)
        self._chk(lib.wcpt_image_upload(self.h, ptr(a), a.nbytes))

    # -- dispatch ---------------------------------------------------------------------------------------
    def composite(self, dst: int, rgba8: bool = False, bloom=None, denoise=None, guide: int | None = None,
                  guide_bytes: int | None = None, temporal=None, scene=None, frames: int | None = None,
                  restart: bool = False):
        """composite.comp into device memory at `dst` (asynchronous); with `bloom` (a BloomParams) its Bloom branch is
        taken: bloom.comp's pyramid of the image is added before gamma and the tonemap (wcpt_composite_bloom). With
        `denoise` (a DenoiseParams) the image goes through the guided a-trous filter first (wcpt_composite_denoise):
        `guide` is the device address of the frame's primary-hit records (trace_primary) and `guide_bytes` the size of
        the memory there (default width * height * 48). Denoise and bloom in one call are not provided.
        With `temporal` (a TemporalParams) the image is first blended with the previous result reprojected to this
        frame (wcpt_composite_temporal), then displayed or, with `denoise`, filtered: `scene` is the scene data of the
        accumulated frames, `frames` the samples in the image (the last render's renderedFramesCount + 1), `restart`
        whether the accumulation restarted since the previous such call, `guide` the records for this camera. Temporal
        and bloom in one call are not provided."""
        if temporal is not None:
            if bloom is not None:
                raise ValueError("composite: temporal and bloom in one call are not provided")
            if guide is None or scene is None or frames is None:
                raise ValueError("composite: temporal needs the guide (the records of trace_primary), the scene data and "
                                 "the number of accumulated frames")
            if guide_bytes is None:
                guide_bytes = self.width * self.height * PRIMARY_HIT_DTYPE.itemsize
            sd = np.ascontiguousarray(scene, dtype=SCENE_DATA_DTYPE)
            self._chk(lib.wcpt_composite_temporal(self.h, ptr(sd), frames, 1 if restart else 0, guide, guide_bytes, dst,
                                                  1 if rgba8 else 0, C.byref(temporal),
                                                  None if denoise is None else C.byref(denoise)))
        elif denoise is not None:
            if bloom is not None:
                raise ValueError("composite: denoise and bloom in one call are not provided")
            if guide is None:
                raise ValueError("composite: denoise needs the guide (the records of trace_primary)")
            if guide_bytes is None:
                guide_bytes = self.width * self.height * PRIMARY_HIT_DTYPE.itemsize
            self._chk(lib.wcpt_composite_denoise(self.h, guide, guide_bytes, dst, 1 if rgba8 else 0, C.byref(denoise)))
        elif bloom is None:
            self._chk(lib.wcpt_composite(self.h, dst, 1 if rgba8 else 0))
        else:
            self._chk(lib.wcpt_composite_bloom(self.h, dst, 1 if rgba8 else 0, C.byref(bloom)))

    def temporal_reset(self):
        """wcpt_temporal_reset: the next composite(temporal=...) starts without history (a material, light or mesh
        change, which the records cannot see)."""
        self._chk(lib.wcpt_temporal_reset(self.h))

    def render(self, sd: np.ndarray, materials: int, spheres: int, draws: int):
        sd = np.ascontiguousarray(sd, dtype=SCENE_DATA_DTYPE)
        self._chk(lib.wcpt_render(self.h, ptr(sd), materials, spheres, draws))

    def sync(self):
        self._chk(lib.wcpt_sync(self.h))

    def trace_primary(self, sd: np.ndarray, spheres: int, draws: int, dst: int | None = None, nbytes: int | None = None,
                      rows: int | None = None):
        """wcpt_trace_primary: the primary hit of every pixel of the context's rows (PRIMARY_HIT_DTYPE: depth, normal
        and the identity of the sphere or triangle). With a device address `dst` (16-byte aligned) the pass is only
        queued; `nbytes` is then the size of the caller's memory at `dst`, which the library checks against width * rows
        * 48 -- the wrapper does not make it up. With dst=None it runs into a buffer of the context's, is waited for, and
        the records come back as a structured array [rows, width]; `rows` are the rows the context holds (default the
        whole frame: like readback, the wrapper does not track a row range or stripes)."""
        sd = np.ascontiguousarray(sd, dtype=SCENE_DATA_DTYPE)
        if dst is not None:
            if nbytes is None:
                raise ValueError("trace_primary: with a device address, pass the size of its memory as nbytes")
            self._chk(lib.wcpt_trace_primary(self.h, ptr(sd), spheres, draws, dst, nbytes))
            return None
        rows = self.height if rows is None else rows
        nbytes = rows * self.width * PRIMARY_HIT_DTYPE.itemsize
        buf = self.buffer_alloc(nbytes)
        try:
            self._chk(lib.wcpt_trace_primary(self.h, ptr(sd), spheres, draws, self.buffer_address(buf), nbytes))
            self.sync()
            out = np.frombuffer(self.buffer_download(buf, nbytes), PRIMARY_HIT_DTYPE)
        finally:
            self.buffer_free(buf)
        return out.reshape(rows, self.width).copy()

    def pick(self, sd: np.ndarray, spheres: int, draws: int, x: int, y: int) -> np.ndarray:
        """wcpt_pick: the primary hit of frame pixel (x, y), a one-element PRIMARY_HIT_DTYPE array. Synchronous."""
        sd = np.ascontiguousarray(sd, dtype=SCENE_DATA_DTYPE)
        out = np.zeros(1, PRIMARY_HIT_DTYPE)
        self._chk(lib.wcpt_pick(self.h, ptr(sd), spheres, draws, x, y, ptr(out)))
        return out

    def primary_cache_stats(self) -> tuple:
        """(writes, reads): the renders that stored / read the primary cache (WCPT_OPTION_PRIMARY_CACHE)."""
        w, r = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib.wcpt_primary_cache_stats(self.h, C.byref(w), C.byref(r)))
        return int(w.value), int(r.value)

    def mk_split_stats(self) -> int:
        """The renders that ran as a head and a tail launch (WCPT_OPTION_MK_SPLIT)."""
        n = C.c_uint64(0)
        self._chk(lib.wcpt_mk_split_stats(self.h, C.byref(n)))
        return int(n.value)

    def mk_tiny_tree_stats(self) -> int:
        """The renders that walked a tiny tree without the traversal loop (WCPT_OPTION_MK_TINY_TREE)."""
        n = C.c_uint64(0)
        self._chk(lib.wcpt_mk_tiny_tree_stats(self.h, C.byref(n)))
        return int(n.value)

    def wf_last_plan(self) -> dict:
        """wcpt_wf_last_plan: what the last wavefront launch did (WfPlanInfo.as_dict()). Host only: it joins nothing, so
        reading it between renders leaves a frame-overlap continuation running."""
        out = WfPlanInfo()
        self._chk(lib.wcpt_wf_last_plan(self.h, C.byref(out)))
        return out.as_dict()

    def render_counters(self, sd: np.ndarray, materials: int, spheres: int, draws: int,
                        diagnostics: bool = False) -> dict:
        """Reference-algorithm work counters of one frame (COUNTER_FIELDS); with diagnostics=True also the
        implementation's SIMD-efficiency step counters (DIAG_FIELDS)."""
        sd = np.ascontiguousarray(sd, dtype=SCENE_DATA_DTYPE)
        c = Counters()
        self._chk(lib.wcpt_set_option(self.h, OPTION_DIAGNOSTICS, 1 if diagnostics else 0))
        try:
            self._chk(lib.wcpt_render_counters(self.h, ptr(sd), materials, spheres, draws, C.byref(c)))
        finally:
            lib.wcpt_set_option(self.h, OPTION_DIAGNOSTICS, 0)
        return c.as_dict(diagnostics)

    def read_diagnostics(self) -> list:
        out = (C.c_uint64 * 8)()
        self._chk(lib.wcpt_read_diagnostics(self.h, out, 8))
        return [int(v) for v in out]

    def profile_begin(self):
        self._chk(lib.wcpt_profile_begin(self.h))

    def profile_end(self):
        ms, n = C.c_double(), C.c_uint32()
        self._chk(lib.wcpt_profile_end(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def selftest(self, fn: int, x: np.ndarray, x2: np.ndarray | None = None) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.uint32)
        per = {1: 4, 7: 3, 22: 3}.get(fn, 1)
        out = np.empty(x.size * per, np.uint32)
        x2p = None
        if x2 is not None:
            x2 = np.ascontiguousarray(x2, dtype=np.uint32)
            x2p = ptr(x2)
        self._chk(lib.wcpt_selftest_device(self.h, fn, ptr(x), x2p, ptr(out), x.size))
        return out

    GEOMETRY_WORDS = {0: (15, 1), 1: (24, 4), 2: (24, 4), 3: (10, 1), 4: (11, 7), 5: (8, 7), 6: (3, 6), 7: (33, 10),
                      8: (19, 6)}

    def selftest_geometry(self, fn: int, arith: int, x: np.ndarray, out_words: int | None = None) -> np.ndarray:
        """wcpt_selftest_geometry on the items x[n, in_words] (32-bit words): the output words, [n, out_words]."""
        x = np.ascontiguousarray(x, dtype=np.uint32)
        assert x.ndim == 2
        if out_words is None:
            out_words = self.GEOMETRY_WORDS[fn][1]
        out = np.empty((x.shape[0], out_words), np.uint32)
        self._chk(lib.wcpt_selftest_geometry(self.h, fn, arith, ptr(x), x.shape[1], ptr(out), out_words, x.shape[0]))
        return out


class DeviceScene:
    """A HostScene resident in device buffers: the six DBufferManagers of PathTracingRenderer.jai:110-117."""

    def __init__(self, ctx: Context, scene: "_scene.HostScene"):
        self.ctx = ctx
        self.scene = scene
        self.buffers = []
        self.materials = self._buf(scene.materials)
        self.spheres = self._buf(scene.spheres)
        draws = np.zeros(len(scene.meshes), dtype=DRAW_COMMAND_DTYPE)
        for i, m in enumerate(scene.meshes):
            draws[i] = (self._buf(m.positions), self._buf(m.indices), self._buf(m.nodes), m.indices.size, 0)
        self.draws = self._buf(draws)

    def _buf(self, arr: np.ndarray) -> int:
        b = self.ctx.buffer_from(arr)
        self.buffers.append(b)
        return self.ctx.buffer_address(b)

    def addresses(self):
        return self.materials, self.spheres, self.draws

    def free(self):
        for b in self.buffers:
            self.ctx.buffer_free(b)
        self.buffers = []


def group_unique_id() -> bytes:
    """wcpt_group_unique_id: the 128-byte RCCL id the root's process hands to every process of a rank group."""
    buf = (C.c_uint8 * GROUP_UNIQUE_ID_BYTES)()
    check(lib.wcpt_group_unique_id(buf))
    return bytes(buf)


class Group:
    """One frame on several devices (include/wcpt.h wcpt_group_*): rank r renders rows
    [r*H/N, (r+1)*H/N) on its device, and a set output gathers every frame's blocks to the root.

    ``Group(devices, root, transport)`` holds every rank in this process (one host thread, like the reference's
    host); ``Group.rank(device, nranks, rank, root, uid)`` holds one rank of a one-process-per-device group. The
    local ranks are ``self.ranks``; ``context(r)`` is rank r's context (None for a rank of another process)."""

    def __init__(self, devices=None, root: int = 0, transport: int = GROUP_TRANSPORT_RCCL, _rank=None):
        h = C.c_void_p()
        if _rank is None:
            devs = (C.c_int * len(devices))(*devices)
            check(lib.wcpt_group_create_ex(devs, len(devices), root, transport, C.byref(h)))
            self.ranks = list(range(len(devices)))
            self.devices = list(devices)
            self.nranks = len(devices)
        else:
            device, nranks, rank, uid = _rank
            idp = None
            if uid is not None:
                assert len(uid) == GROUP_UNIQUE_ID_BYTES
                idp = (C.c_uint8 * GROUP_UNIQUE_ID_BYTES).from_buffer_copy(uid)
            check(lib.wcpt_group_create_rank(device, nranks, rank, root, idp, C.byref(h)))
            self.ranks = [rank]
            self.devices = [device]
            self.nranks = nranks
        self.h = h
        self.root = root
        self._ctx = {r: Context.borrowed(lib.wcpt_group_context(h, r), d) for r, d in zip(self.ranks, self.devices)}
        self.contexts = [self._ctx[r] for r in self.ranks]

    @classmethod
    def rank(cls, device: int, nranks: int, rank: int, root: int = 0, uid: bytes | None = None) -> "Group":
        return cls(root=root, _rank=(device, nranks, rank, uid))

    def close(self):
        if self.h:
            for c in self.contexts:
                c.h = None
            lib.wcpt_group_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def context(self, rank: int) -> Context | None:
        return self._ctx.get(rank)

    def set_option(self, option: int, value: int):
        check(lib.wcpt_group_set_option(self.h, option, value))
        if option == GROUP_OPTION_ROW_STRIPE:
            self.stripe = value
            if getattr(self, "width", None):
                self._set_rows()

    def info(self) -> dict:
        out = GroupInfo()
        check(lib.wcpt_group_info_get(self.h, C.byref(out)))
        return out.as_dict()

    def create_screen(self, width: int, height: int):
        check(lib.wcpt_group_create_screen(self.h, width, height))
        self.width, self.height = width, height
        self._set_rows()

    def _set_rows(self):
        from .dist import row_stripes
        for r, c in self._ctx.items():   # a rank's context holds only its rows (a block, or interleaved stripes)
            c.width, c.height = self.width, row_stripes(self.height, self.nranks, r, getattr(self, "stripe", 0))[1]

    def set_output(self, fmt: int, dst: int, nbytes: int):
        check(lib.wcpt_group_set_output(self.h, fmt, dst, nbytes))

    def render(self, sd: np.ndarray, materials, spheres, draws):
        """materials / spheres / draws: one device address per local rank, in rank order."""
        n = len(self.ranks)
        sd = np.ascontiguousarray(sd, dtype=SCENE_DATA_DTYPE)
        arr = [(C.c_uint64 * n)(*[int(v) for v in a]) for a in (materials, spheres, draws)]
        check(lib.wcpt_group_render(self.h, ptr(sd), *arr))

    def sync(self):
        check(lib.wcpt_group_sync(self.h))


class PathTracingRenderer:
    """Host mirror of ``PathTracingRenderer`` (src/PathTracingRenderer.jai:92-123) over the C-ABI."""

    def __init__(self, device: int = 0, arith: int = ARITH_EXACT):
        """arith: ARITH_EXACT (default, bit-identical to the oracle) or ARITH_FAST (WCPT_OPTION_ARITH: the megakernel's
        fast-arithmetic instances, for display)."""
        self.renderSize = (0, 0)
        self.samples = 1                 # :119
        self.maxBounceCount = 3          # :120
        self.renderedFramesCount = 0     # :121
        self.boxID = 0                   # :122
        self.materials = np.zeros(0, dtype=MATERIAL_DTYPE)
        self.spheres = np.zeros(0, dtype=SPHERE_DTYPE)
        self.meshes = []
        self.build = "host"              # Init's `build`: where LoadModel builds each mesh's BVH
        self.bvh = "midpoint"            # Init's `bvh`: which tree
        self.ctx = Context(device)
        if arith != ARITH_EXACT:
            self.ctx.set_option(OPTION_ARITH, arith)
        self._mat_buf = self._sph_buf = self._draw_buf = None
        self._mesh_bufs = []
        self._mesh_info = []             # per mesh: (vb, ib, nb, vertex count, index count, nodes used), for UpdateMesh
        self._guide_buf = None           # Composite(denoise=...): the primary-hit records of the accumulated frames
        self._guide_bytes = 0
        self._guide_stale = True
        self._temporal_restart = True    # Composite(temporal=...): the guide was retraced since the last temporal call
        self._mat_uploaded = None        # the materials of the last UpdateMaterials, as bytes

    # Init :272-343 — LoadModel + materials/spheres + UpdateMaterials
    def Init(self, model_path: str | None = None, scene: "_scene.HostScene | None" = None, build: str = "host",
             bvh: str = "midpoint"):
        """build: "host" (default) uploads trees built by wcpt_bvh_build; "device" uploads each mesh's positions and
        indices as they are and builds the same tree there (wcpt_bvh_build_device), so a model is loaded without the
        host builder's stall.
        bvh: "midpoint" (default, the reference's tree) or "sah", the binned-SAH tree: built by wcpt_bvh_build_sah on
        the host or by wcpt_bvh_build_sah_device, from each mesh's positions and indices as they are (a `scene` whose
        meshes carry nodes of their own has those nodes uploaded only with build="host", bvh="midpoint")."""
        if build not in ("host", "device"):
            raise ValueError(f"unknown build {build!r}")
        if bvh not in ("midpoint", "sah"):
            raise ValueError(f"unknown bvh {bvh!r}")
        self.build = build
        self.bvh = bvh
        if scene is None:
            scene = _scene.generate("default")
            if model_path is not None:
                mesh = _scene.obj_load(model_path)
                scene.meshes = [mesh if build == "device" or bvh == "sah" else _scene.bvh_build(mesh)]
        self.materials = scene.materials.copy()
        self.spheres = scene.spheres.copy()
        self.meshes = list(scene.meshes)
        self.LoadModel()
        self.UpdateMaterials()

    # LoadModel :219-270 — vertex/index/BVH uploads + one DrawCommand per mesh
    def LoadModel(self):
        draws = np.zeros(len(self.meshes), dtype=DRAW_COMMAND_DTYPE)
        self._mesh_info = []
        for i, m in enumerate(self.meshes):
            if self.build == "device":
                vb, ib, nb, used = _scene.device_bvh_build(self.ctx, _scene.HostMesh(m.positions, m.indices), self.bvh)
            else:
                if self.bvh == "sah":
                    m = _scene.bvh_build(_scene.HostMesh(m.positions, m.indices), "sah")
                vb, ib, nb = (self.ctx.buffer_from(m.positions), self.ctx.buffer_from(m.indices),
                              self.ctx.buffer_from(m.nodes))
                used = len(m.nodes)
            self._mesh_bufs += [vb, ib, nb]
            self._mesh_info.append((vb, ib, nb, int(np.asarray(m.positions).reshape(-1, 3).shape[0]), int(m.indices.size), used))
            draws[i] = (self.ctx.buffer_address(vb), self.ctx.buffer_address(ib), self.ctx.buffer_address(nb),
                        m.indices.size, 0)
        if self._draw_buf is None:
            self._draw_buf = self.ctx.buffer_alloc(0)
        self.ctx.buffer_upload(self._draw_buf, draws)

    def UpdateMesh(self, i: int, positions: np.ndarray, refit: str = "device"):
        """New positions for mesh i, its triangles unchanged (an editor's drag, an animation's frame): uploads them,
        refits that mesh's tree -- refit="device": wcpt_bvh_refit_device in place; "host": wcpt_bvh_refit over the
        device's indices and nodes, uploaded back -- and restarts the accumulation, as the reference's editor does
        whenever something moves. After Init with either `build` and either `bvh`."""
        if refit not in ("device", "host"):
            raise ValueError(f"unknown refit {refit!r}")
        vb, ib, nb, vertex_count, index_count, used = self._mesh_info[i]
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        if pos.shape[0] != vertex_count:
            raise ValueError(f"mesh {i} has {vertex_count} vertices, got {pos.shape[0]}")
        if refit == "device":
            _scene.device_bvh_refit(self.ctx, vb, ib, nb, pos, index_count, used)
        else:
            idx = np.frombuffer(self.ctx.buffer_download(ib, 4 * index_count), np.uint32)
            nodes = np.frombuffer(self.ctx.buffer_download(nb, NODE_DTYPE.itemsize * used), NODE_DTYPE)
            new = _scene.bvh_refit(_scene.HostBVH(pos, idx, nodes), pos)
            self.ctx.buffer_upload(vb, pos)
            self.ctx.buffer_upload(nb, new.nodes)
        self.renderedFramesCount = 0
        self._guide_stale = True
        self.ctx.temporal_reset()

    # PushMaterial :492-496
    def PushMaterial(self) -> int:
        m = np.zeros(1, dtype=MATERIAL_DTYPE)
        m["absorptionStrength"] = 1.0
        m["ior"] = 1.0
        self.materials = np.concatenate([self.materials, m])
        return len(self.materials) - 1

    # UpdateMaterials :459-471 — re-upload materials and spheres (grow-on-demand)
    def UpdateMaterials(self):
        if self._mat_buf is None:
            self._mat_buf = self.ctx.buffer_alloc(0)
            self._sph_buf = self.ctx.buffer_alloc(0)
        self.ctx.buffer_upload(self._mat_buf, self.materials)
        self.ctx.buffer_upload(self._sph_buf, self.spheres)
        # Composite(temporal=...): changed materials are nothing the records show, so they drop the history. The editor
        # uploads every frame (editor.jai:154-158); an upload of the same materials keeps it, and so do moved spheres:
        # the depth test rejects what moved
        uploaded = self.materials.tobytes()
        if self._mat_uploaded is not None and uploaded != self._mat_uploaded:
            self.ctx.temporal_reset()
        self._mat_uploaded = uploaded

    # CreateScreen :345-385
    def CreateScreen(self, size):
        w, h = int(size[0]), int(size[1])
        self.renderSize = (w, h)
        self.ctx.create_screen(w, h)

    # Resize :393-397
    def Resize(self, size):
        self.CreateScreen(size)
        self.renderedFramesCount = 0
        self._guide_stale = True

    def scene_data(self, camera: Camera) -> np.ndarray:
        """SceneData as Render fills it (:410-422); the camera's matrices must be up to date (Update :22)."""
        sd = np.zeros((), dtype=SCENE_DATA_DTYPE)
        sd["inverseProjection"] = np.ctypeslib.as_array(camera.inverseProjection)
        sd["inverseView"] = np.ctypeslib.as_array(camera.inverseView)
        sd["position"] = np.ctypeslib.as_array(camera.position)
        sd["maxBounceCount"] = self.maxBounceCount
        sd["samples"] = self.samples
        sd["sphereCount"] = len(self.spheres)
        sd["drawCommandCount"] = len(self.meshes)
        sd["renderedFramesCount"] = self.renderedFramesCount
        sd["boxID"] = self.boxID
        return sd

    # Render :399-457
    def Render(self, camera: Camera):
        sd = self.scene_data(camera)
        if self.renderedFramesCount == 0:
            self._guide_stale = True     # the accumulation restarts: something moved
        self.renderedFramesCount += 1    # :423 (the editor adds its own +1 when the camera is still)
        self.ctx.render(sd, self.ctx.buffer_address(self._mat_buf), self.ctx.buffer_address(self._sph_buf),
                        self.ctx.buffer_address(self._draw_buf))

    def Readback(self) -> np.ndarray:
        return self.ctx.readback()

    def Composite(self, camera: Camera, dst: int, rgba8: bool = False, denoise=None, temporal=None):
        """The display step into device memory at `dst` (Context.composite). With `denoise` (a DenoiseParams) or
        `temporal` (a TemporalParams) the renderer keeps a guide buffer of its own and traces it with
        Context.trace_primary only when it is stale: on first use, after Resize, after UpdateMesh, and after any Render
        whose renderedFramesCount was 0 -- the editor's protocol: whatever moves, the count restarts. That moment is also
        the temporal stage's restart; Resize, UpdateMesh and an UpdateMaterials with changed materials drop its history (a
        moved sphere does not: the depth test rejects what moved)."""
        if denoise is None and temporal is None:
            self.ctx.composite(dst, rgba8=rgba8)
            return
        w, h = self.renderSize
        nbytes = w * h * PRIMARY_HIT_DTYPE.itemsize
        if self._guide_buf is None or self._guide_bytes < nbytes:
            if self._guide_buf is not None:
                self.ctx.buffer_free(self._guide_buf)
            self._guide_buf = self.ctx.buffer_alloc(nbytes)
            self._guide_bytes = nbytes
            self._guide_stale = True
        guide = self.ctx.buffer_address(self._guide_buf)
        sd = self.scene_data(camera)
        if self._guide_stale:
            self.ctx.trace_primary(sd, self.ctx.buffer_address(self._sph_buf), self.ctx.buffer_address(self._draw_buf), guide,
                                   self._guide_bytes)
            self._guide_stale = False
            self._temporal_restart = True
        if temporal is None:
            self.ctx.composite(dst, rgba8=rgba8, denoise=denoise, guide=guide, guide_bytes=self._guide_bytes)
            return
        self.ctx.composite(dst, rgba8=rgba8, denoise=denoise, guide=guide, guide_bytes=self._guide_bytes, temporal=temporal,
                           scene=sd, frames=max(1, self.renderedFramesCount), restart=self._temporal_restart)
        self._temporal_restart = False

    def Pick(self, camera: Camera, x: int, y: int):
        """What pixel (x, y) of the frame shows from `camera` (wcpt_pick): (record, position) -- the PRIMARY_HIT_DTYPE
        record of the pixel's primary ray and the hit point origin + t * direction in float32 (of no meaning on a miss).
        The frame counter and the accumulation are left alone."""
        sd = self.scene_data(camera)
        rec = self.ctx.pick(sd, self.ctx.buffer_address(self._sph_buf), self.ctx.buffer_address(self._draw_buf), x, y)[0]
        origin = np.asarray(sd["position"], np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            position = origin + np.float32(rec["t"]) * np.asarray(rec["direction"], np.float32)
        return rec, position

    # Deinit :473-490
    def Deinit(self):
        for b in self._mesh_bufs:
            self.ctx.buffer_free(b)
        self._mesh_bufs = []
        for b in (self._mat_buf, self._sph_buf, self._draw_buf, self._guide_buf):
            if b is not None:
                self.ctx.buffer_free(b)
        self._mat_buf = self._sph_buf = self._draw_buf = self._guide_buf = None
        self.ctx.close()


class Editor:
    """The editor's per-frame protocol around the renderer (src/editor.jai:118-158), for frame sequencing:

    - camera input: ``moved`` resets ``renderedFramesCount`` to 0, otherwise the editor adds 1 (:149-152);
    - UpdateEditor (:154-158): camera Update (aspect of the viewport), UpdateMaterials, Render, which uploads
      SceneData with the current count and adds its own 1 (PathTracingRenderer.jai:423).

    So while the camera is still the shader sees every second frame number (1, 3, 5, ... from start-up; 0, 2,
    4, ... after a move), and the progressive ``mix`` weights follow that sequence. ``frame`` returns the
    count the dispatch used.
    """

    def __init__(self, renderer: PathTracingRenderer, camera: Camera):
        self.renderer = renderer
        self.camera = camera
        self.selectedSphere = -1     # editor.jai: the selected sphere's index, -1 = nothing selected

    def select(self, x: int, y: int):
        """A click on pixel (x, y) of the viewport: ``selectedSphere`` becomes the index of the sphere the pixel shows,
        or -1 when it shows the mesh or the sky. Returns the pixel's record (PathTracingRenderer.Pick); no frame counter
        changes, so the accumulation goes on."""
        r = self.renderer
        w, h = r.renderSize
        cam = _scene.update_camera(self.camera, w / h)
        rec, _ = r.Pick(cam, x, y)
        is_sphere = (int(rec["kind"]) & HIT_KIND_MASK) == HIT_SPHERE
        self.selectedSphere = int(rec["index"]) if is_sphere else -1
        return rec

    def frame(self, moved: bool = False) -> int:
        r = self.renderer
        if moved:
            r.renderedFramesCount = 0
        else:
            r.renderedFramesCount += 1
        w, h = r.renderSize
        cam = _scene.update_camera(self.camera, w / h)
        r.UpdateMaterials()
        used = r.renderedFramesCount
        r.Render(cam)
        return used


__all__ = ["Context", "DeviceScene", "Group", "group_unique_id", "PathTracingRenderer", "Editor", "COUNTER_FIELDS"]
