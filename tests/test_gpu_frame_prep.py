"""Frame preparation on the GPU (wcpt_render.hip prepare_tri_records, csrc/frame_prep.h): one context renders a sequence
of frames that takes each preparation path in turn -- a miss, an unchanged frame, a moved camera, an option change that
reuses the records, a re-uploaded mesh that rebuilds them, the triangle cache off and on again -- and every frame equals,
bit for bit, the same frame rendered by a context created fresh for it, which can only take the miss path. The fresh
context gets the sequence's options and the image accumulated so far (wcpt_image_upload).

The Cornell box at 64x64, one sample, three bounces: one draw with every table flag set, pair records and the megakernel
under WCPT_KERNEL_AUTO, so each path's effect on the plan (pair records, the kernel, the primary-ray records of both
frame-overlap pipes) shows in the image or in wcpt_last_kernel."""
import copy

import numpy as np
import pytest

import wcpt
from wcpt import scene as wscene

from test_gpu_parity import get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 64, 64
BOUNCES = 3


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def _moved(s):
    p = [float(v) for v in s.camera.position]
    return wscene.make_camera(position=(p[0] + 0.05, p[1] - 0.03, p[2] + 0.02), yaw=s.camera.yaw + 3.0,
                              pitch=s.camera.pitch, fov=s.camera.fov)


def _shrunk(s):
    """the scene with its first mesh scaled a little towards the origin (and its BVH rebuilt): another image"""
    m = s.meshes[0]
    s2 = copy.copy(s)
    s2.meshes = [wscene.bvh_build(wscene.HostMesh(np.asarray(m.positions, np.float32) * np.float32(0.95), m.indices))]
    s2.meshes += s.meshes[1:]
    assert s2.meshes[0].indices.size == m.indices.size and len(s2.meshes[0].nodes) == len(m.nodes)
    return s2


class _Sequence:
    """The long-lived context, and per frame the fresh one it is compared with."""

    def __init__(self, scene, kernel):
        self.scene, self.kernel, self.options, self.frame_no = scene, kernel, {}, 0
        self.ctx = wcpt.Context(0)
        self.ctx.set_kernel(kernel)
        self.dev = wcpt.DeviceScene(self.ctx, scene)
        self.ctx.create_screen(W, H)

    def close(self):
        self.dev.free()
        self.ctx.close()

    def set_option(self, option, value):
        self.options[option] = value
        self.ctx.set_option(option, value)

    def upload_mesh(self, scene):
        """draw 0's vertex, index and BVH buffers rewritten through wcpt_buffer_upload (DeviceScene's buffers: materials,
        spheres, then per mesh positions, indices, nodes)"""
        m = scene.meshes[0]
        for handle, arr in zip(self.dev.buffers[2:5], (m.positions, m.indices, m.nodes)):
            self.ctx.buffer_upload(handle, arr)
        self.scene = scene

    def frame(self, camera=None, kernel=None, what=""):
        """Render the next frame here and on a fresh context; the images must be the same bits. Returns the image."""
        sd = self.scene.scene_data(W, H, max_bounce=BOUNCES, samples=1, frame=self.frame_no, camera=camera)
        before = self.ctx.readback()
        self.ctx.render(sd, *self.dev.addresses())
        self.ctx.sync()
        img, ran = self.ctx.readback(), self.ctx.last_kernel()
        with wcpt.Context(0) as fresh:
            fresh.set_kernel(self.kernel)
            for option, value in self.options.items():
                fresh.set_option(option, value)
            dev = wcpt.DeviceScene(fresh, self.scene)
            fresh.create_screen(W, H)
            fresh.image_upload(before)
            fresh.render(sd, *dev.addresses())
            fresh.sync()
            ref, ref_ran = fresh.readback(), fresh.last_kernel()
            dev.free()
        label = f"frame {self.frame_no} ({what})"
        assert ran == ref_ran, label
        if kernel is not None:
            assert ran == kernel, label
        assert np.array_equal(_bits(img), _bits(ref)), f"{label}: differs from a fresh context's frame"
        assert not np.array_equal(_bits(img), _bits(before)), f"{label}: nothing rendered"
        self.frame_no += 1
        return img


def _first_four(seq, kernel):
    s = seq.scene
    seq.frame(kernel=kernel, what="miss")
    seq.frame(kernel=kernel, what="hit")
    a = seq.frame(camera=_moved(s), kernel=kernel, what="camera moved")
    b = seq.frame(camera=_moved(s), kernel=kernel, what="hit at the new position")
    return a, b


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_AUTO, wcpt.KERNEL_MEGAKERNEL])
def test_every_preparation_path_renders_a_fresh_contexts_frame(kernel):
    MK, WF = wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT
    s = get_scene("cornell")
    assert len(s.meshes) == 1 and s.meshes[0].indices.size == 102 and len(s.meshes[0].nodes) == 3
    seq = _Sequence(s, kernel)
    try:
        _first_four(seq, MK)
        cam = _moved(s)
        # singles: a miss that keeps the triangle records; WCPT_KERNEL_AUTO now takes the wavefront kernel
        seq.set_option(T.OPTION_PAIR_RECORDS, 0)
        singles = WF if kernel == wcpt.KERNEL_AUTO else MK
        seq.frame(camera=cam, kernel=singles, what="pair records off")
        seq.frame(camera=cam, kernel=singles, what="hit")
        # other geometry in the same buffers: the generation bump rebuilds the records
        seq.upload_mesh(_shrunk(s))
        seq.frame(camera=cam, kernel=singles, what="mesh re-uploaded")
        seq.frame(camera=cam, kernel=singles, what="hit")
        # the cache off: draw commands read from the device, nothing cached
        seq.set_option(T.OPTION_TRIANGLE_CACHE, 0)
        seq.frame(camera=cam, kernel=singles, what="triangle cache off")
        seq.frame(camera=cam, kernel=singles, what="triangle cache off, again")
        seq.set_option(T.OPTION_TRIANGLE_CACHE, 1)
        seq.frame(camera=cam, kernel=singles, what="triangle cache on again")
        seq.frame(kernel=singles, what="camera back")
        # and pair records again, on the rebuilt records
        seq.set_option(T.OPTION_PAIR_RECORDS, -1)
        seq.frame(kernel=MK, what="pair records automatic")
        seq.frame(camera=cam, kernel=MK, what="camera moved")
    finally:
        seq.close()


def test_the_first_four_steps_under_the_wavefront_kernel():
    seq = _Sequence(get_scene("cornell"), wcpt.KERNEL_WAVEFRONT)
    try:
        _first_four(seq, wcpt.KERNEL_WAVEFRONT)
    finally:
        seq.close()


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT, wcpt.KERNEL_AUTO])
def test_two_draws(kernel):
    """the Cornell mesh and a shrunk copy of it: two table entries, neither one-draw fast path"""
    s = copy.copy(get_scene("cornell"))
    s.meshes = [s.meshes[0], _shrunk(s).meshes[0]]
    expect = wcpt.KERNEL_MEGAKERNEL if kernel == wcpt.KERNEL_AUTO else kernel
    seq = _Sequence(s, kernel)
    try:
        seq.frame(kernel=expect, what="miss")
        seq.frame(kernel=expect, what="hit")
        seq.frame(camera=_moved(s), kernel=expect, what="camera moved")
    finally:
        seq.close()
