"""Split renders (WCPT_OPTION_MK_SPLIT) on the GPU: a one-sample megakernel render cut before segment k into a head
launch, which appends the surviving paths to a queue, and a tail launch, which finishes them one per lane
(pt_kernels.hip pt_mk_tail, csrc/mk_split_rule.h). Same arithmetic per path, so every sequence here equals, bit for bit,
the same sequence on a context with the option at 0, and where named the CPU oracle's accumulation.

Every test asserts the number of split renders it expects (wcpt_mk_split_stats), so none can pass with the split
silently never taken. 70x45 leaves partial 8x8 tiles at both edges. The unsplit sequences and the oracle's images are
computed once per module and shared.
"""
import copy

import numpy as np
import pytest

import wcpt
import oracle
from wcpt import scene as wscene

from test_gpu_parity import _variant, assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 70, 45
AUTO = -1


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def _closed_box():
    """The Cornell materials and no spheres inside a closed cube around the camera: no path ever leaves."""
    s = copy.copy(get_scene("cornell"))
    s.spheres = s.spheres[:0]
    c = np.array([[x, y, z] for x in (-2, 2) for y in (-2, 2) for z in (-2, 2)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([v for a, b, cc, d in quads for v in (a, b, cc, a, cc, d)], np.uint32)
    s.meshes = [wscene.bvh_build(wscene.HostMesh(c, idx))]
    s.camera = wscene.make_camera(position=(0.25, -0.5, 0.125), yaw=0.3, pitch=0.1, fov=90.0)
    return s


_built = {}


def _scene(name):
    if name not in _built:
        if name in ("two_draws", "empty"):
            _built[name] = _variant("cornell", name)
        elif name == "closed_box":
            _built[name] = _closed_box()
        else:
            _built[name] = get_scene(name)
    return _built[name]


class _Run:
    def __init__(self, s, split, w=W, h=H, overlap=None, cache=True, arith=0):
        self.s, self.w, self.h = s, w, h
        self.ctx = wcpt.Context(0)
        self.ctx.set_option(T.OPTION_MK_SPLIT, split)
        self.ctx.set_option(T.OPTION_PRIMARY_CACHE, 1 if cache else 0)
        self.ctx.set_option(T.OPTION_ARITH, arith)
        if overlap is not None:
            self.ctx.set_option(T.OPTION_FRAME_OVERLAP, overlap)
        self.dev = wcpt.DeviceScene(self.ctx, s)
        self.ctx.create_screen(w, h)

    def sd(self, frame, bounces=4, spp=1, camera=None):
        return self.s.scene_data(self.w, self.h, max_bounce=bounces, samples=spp, frame=frame, camera=camera)

    def render(self, frame, bounces=4, spp=1, camera=None):
        self.ctx.render(self.sd(frame, bounces, spp, camera), *self.dev.addresses())

    def image(self):
        self.ctx.sync()
        return self.ctx.readback(self.h)

    def close(self):
        self.dev.free()
        self.ctx.close()


def _sequence(s, split, frames=range(6), bounces=4, **kw):
    """The image after each frame, and the split renders the context counted."""
    r = _Run(s, split, **kw)
    try:
        imgs = []
        for f in frames:
            r.render(f, bounces)
            imgs.append(r.image())
        return imgs, r.ctx.mk_split_stats(), r.ctx.primary_cache_stats()
    finally:
        r.close()


_refs = {}


def _unsplit(name, bounces=4, **kw):
    key = (name, bounces, tuple(sorted(kw.items())))
    if key not in _refs:
        imgs, n, _ = _sequence(_scene(name), 0, bounces=bounces, **kw)
        assert n == 0
        _refs[key] = imgs
    return _refs[key]


_oracles = {}


def _oracle_acc(name, w, h, bounces, frames=6):
    key = (name, w, h, bounces, frames)
    if key not in _oracles:
        s, acc = _scene(name), None
        for f in range(frames):
            acc, _ = oracle.render_scene(s, w, h, sd=s.scene_data(w, h, max_bounce=bounces, frame=f), image=acc, threads=8)
        _oracles[key] = acc
    return _oracles[key]


def _assert_equal_lists(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), f"image {i} differs from the unsplit context"


# ---- 1. every cut, all three head builds ----------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [1, 2, 3, 4, AUTO])
def test_cornell_every_cut(cut):
    """Frames 0..5 at 4 bounces: frame 0 renders plainly, frame 1 writes the primary cache, the rest read it, so the
    head runs in its three primary-cache builds. The automatic rule leaves a frame of 54 tiles whole (it wants 3
    rounds of resident waves; test_automatic_rule_at_full_size renders one it splits)."""
    imgs, n, pc = _sequence(_scene("cornell"), cut)
    assert n == (0 if cut == AUTO else 6) and pc == (1, 4)
    _assert_equal_lists(imgs, _unsplit("cornell"))
    assert_close(imgs[-1], _oracle_acc("cornell", W, H, 4))


def test_cut_past_the_last_segment_renders_whole():
    """Segments are 0..maxBounceCount: a cut before a segment that does not exist is one launch."""
    imgs, n, _ = _sequence(_scene("cornell"), 4, bounces=3)
    assert n == 0
    _assert_equal_lists(imgs, _unsplit("cornell", bounces=3))
    imgs, n, _ = _sequence(_scene("cornell"), 3, bounces=3)
    assert n == 6
    _assert_equal_lists(imgs, _unsplit("cornell", bounces=3))


def test_samples_and_scratch_stack_render_whole():
    s = _scene("cornell")
    r = _Run(s, 2)
    try:
        r.render(0, 4, spp=2)
        assert r.ctx.mk_split_stats() == 0
        r.ctx.set_option(T.OPTION_STACK, 0)
        r.render(1, 4)
        assert r.ctx.mk_split_stats() == 0
        r.ctx.set_option(T.OPTION_STACK, 1)
        r.render(2, 4)
        r.image()
        assert r.ctx.mk_split_stats() == 1
    finally:
        r.close()


def test_automatic_rule_at_full_size():
    """1920x1080 (32400 tiles, 7.9 rounds of resident waves): the automatic rule splits every frame -- the first
    unpiped, the later ones as the frame overlap's two pipes, each with its own queue -- and the accumulated image is
    the unsplit context's."""
    s = _scene("cornell")
    res = {}
    for split in (AUTO, 0):
        r = _Run(s, split, 1920, 1080)
        try:
            for f in range(4):
                r.render(f, 4)
            res[split] = r.image()
            assert r.ctx.mk_split_stats() == (4 if split == AUTO else 0)
        finally:
            r.close()
    assert np.array_equal(_bits(res[AUTO]), _bits(res[0]))


def test_automatic_rule_leaves_a_large_mesh_whole():
    """The reference's scene at the same size: more than 64 triangles, so the automatic rule renders it in one launch
    (its tail waves would mix unrelated tiles: measured slower at every cut); a forced cut still splits it, same bits."""
    s = get_scene("reference_init")
    res = {}
    for split in (AUTO, 3, 0):
        r = _Run(s, split, 1920, 1080)
        try:
            for f in range(2):
                r.render(f, 3)
            res[split] = r.image()
            assert r.ctx.mk_split_stats() == (2 if split == 3 else 0)
        finally:
            r.close()
    assert np.array_equal(_bits(res[AUTO]), _bits(res[0])) and np.array_equal(_bits(res[3]), _bits(res[0]))


# ---- 2. primary cache off, fast arithmetic --------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [1, 3])
def test_primary_cache_off(cut):
    imgs, n, pc = _sequence(_scene("cornell"), cut, cache=False)
    assert n == 6 and pc == (0, 0)
    _assert_equal_lists(imgs, _unsplit("cornell"))


@pytest.mark.parametrize("cut", [1, 3])
def test_fast_arithmetic(cut):
    """arith = 1 against an unsplit arith = 1 context: the fast head and tail keep the fast kernel's bits."""
    imgs, n, _ = _sequence(_scene("cornell"), cut, arith=1)
    assert n == 6
    _assert_equal_lists(imgs, _unsplit("cornell", arith=1))


# ---- 3. the queue's extremes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [1, 3])
def test_zero_survivors(cut):
    """No draw command and no sphere: every path ends at the sky in segment 0, the tail launches and every wave
    exits."""
    imgs, n, _ = _sequence(_scene("empty"), cut)
    assert n == 6
    _assert_equal_lists(imgs, _unsplit("empty"))
    assert_close(imgs[-1], _oracle_acc("empty", W, H, 4))


@pytest.mark.parametrize("cut", [1, 4])
def test_all_pixels_survive(cut):
    """A camera inside a closed cube at 64x40 (whole tiles): every path reaches the tail, so the queue is filled to
    its capacity."""
    s = _scene("closed_box")
    w, h = 64, 40
    r = _Run(s, 0, w, h)
    try:
        cnt = r.ctx.render_counters(r.sd(0, 4), *r.dev.addresses())
    finally:
        r.close()
    assert cnt["segments"] == 5 * w * h, "a path left the closed cube"
    imgs, n, _ = _sequence(s, cut, w=w, h=h)
    assert n == 6
    _assert_equal_lists(imgs, _unsplit("closed_box", w=w, h=h))
    assert_close(imgs[-1], _oracle_acc("closed_box", w, h, 4))


@pytest.mark.parametrize("cut", [1, 3])
def test_two_draw_commands(cut):
    """The multi-draw builds (12-byte primary-cache records, the draw loop in head and tail) at 64x40."""
    imgs, n, _ = _sequence(_scene("two_draws"), cut, w=64, h=40)
    assert n == 6
    _assert_equal_lists(imgs, _unsplit("two_draws", w=64, h=40))
    assert_close(imgs[-1], _oracle_acc("two_draws", 64, 40, 4))


# ---- 4. frame overlap, moving camera --------------------------------------------------------------------------------
def test_forced_frame_overlap_across_resorts():
    """20 frames at 64x48 as two pipes (the re-sorts after renders 1, 4 and 16 join and fork again; each pipe has its
    own queue and counters), with a readback every fifth frame."""
    s = _scene("cornell")
    res = {}
    for split, ov in ((3, 2), (0, 0)):
        r = _Run(s, split, 64, 48, overlap=ov)
        try:
            imgs = []
            for f in range(20):
                r.render(f, 4)
                if f % 5 == 4:
                    imgs.append(r.image())
            res[split] = imgs
            assert r.ctx.mk_split_stats() == (20 if split else 0)
        finally:
            r.close()
    _assert_equal_lists(res[3], res[0])


def test_moving_camera_then_still():
    """Six frames of a moving camera (renderedFramesCount 0 each: the head without the primary cache), then the
    camera stands and frames 1..3 accumulate (write, read, read)."""
    s = _scene("cornell")
    cams = []
    for i in range(6):
        c = wscene.update_camera(s.camera, W / H)
        c.yaw = s.camera.yaw + 0.02 * (i + 1)
        cams.append(c)
    res = {}
    for split in (3, 0):
        r = _Run(s, split)
        try:
            imgs = []
            for c in cams:
                r.render(0, 4, camera=c)
                imgs.append(r.image())
            for f in (1, 2, 3):
                r.render(f, 4, camera=cams[-1])
                imgs.append(r.image())
            res[split] = imgs
            assert r.ctx.mk_split_stats() == (9 if split else 0)
            assert r.ctx.primary_cache_stats() == (1, 2)
        finally:
            r.close()
    _assert_equal_lists(res[3], res[0])
    assert not np.array_equal(_bits(res[0][0]), _bits(res[0][5]))   # the camera did move


# ---- 5. groups: row blocks and stripes, payloads --------------------------------------------------------------------
def _group_payload(s, split, stripe, fmt, w, h, frames):
    with wcpt.Group([0, 0], root=0, transport=T.GROUP_TRANSPORT_COPY) as g:
        if stripe:
            g.set_option(T.GROUP_OPTION_ROW_STRIPE, stripe)
        for r in range(2):
            g.context(r).set_option(T.OPTION_MK_SPLIT, split)
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(2)]
        g.create_screen(w, h)
        rc = g.context(0)
        nbytes = w * h * T.PAYLOAD_PIXEL_BYTES[fmt]
        out = rc.buffer_from(np.full(nbytes // 4, -5.0, np.float32))
        g.set_output(fmt, rc.buffer_address(out), nbytes)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        for f in frames:
            g.render(s.scene_data(w, h, max_bounce=4, frame=f), *addr)
        g.sync()
        raw = rc.buffer_download(out, nbytes)
        stats = [g.context(r).mk_split_stats() for r in range(2)]
        rc.buffer_free(out)
        for d in devs:
            d.free()
    return np.frombuffer(raw, np.uint8).copy(), stats


@pytest.mark.parametrize("fmt", [T.PAYLOAD_RGB32F, T.PAYLOAD_DISPLAY_RGBA8])
@pytest.mark.parametrize("stripe", [0, 8])
def test_group_payload_rows(stripe, fmt):
    """A one-process group of 2 ranks on one device (COPY), row blocks and stripes of 8 rows, 80x72 over 4 frames: the
    payload rows the tail writes land where the whole kernel writes them."""
    s = _scene("cornell")
    frames = range(4)
    got, stats = _group_payload(s, 3, stripe, fmt, 80, 72, frames)
    ref, none = _group_payload(s, 0, stripe, fmt, 80, 72, frames)
    assert stats == [4, 4] and none == [0, 0]
    assert np.array_equal(got, ref)


# ---- 6. counters ----------------------------------------------------------------------------------------------------
def test_counters_on_a_split_context():
    """wcpt_render_counters takes the whole counting kernel whatever the option says."""
    s = _scene("cornell")
    out = {}
    for split in (3, 0):
        r = _Run(s, split)
        try:
            r.render(0, 4)
            r.render(1, 4)
            out[split] = r.ctx.render_counters(r.sd(2, 4), *r.dev.addresses())
            r.render(2, 4)
            r.image()
            assert r.ctx.mk_split_stats() == (3 if split else 0)
        finally:
            r.close()
    assert out[3] == out[0]
    _, ref = oracle.render_scene(s, W, H, sd=s.scene_data(W, H, max_bounce=4, frame=2), threads=8)
    assert out[3] == ref


def test_option_values():
    r = _Run(_scene("cornell"), 0)
    try:
        for bad in (-2, 16):
            with pytest.raises(wcpt.WcptError):
                r.ctx.set_option(T.OPTION_MK_SPLIT, bad)
        r.ctx.set_option(T.OPTION_MK_SPLIT, 15)
    finally:
        r.close()
