"""The primary-hit buffer and the pick on the GPU (wcpt_trace_primary, wcpt_pick; csrc/pt_primary.hip): per pixel, what
Intersect leaves for the primary ray, with the identity of the primitive. Every comparison is on uint32 views, all 12
words of every record, `_pad` included, against tests/primary_ref.py -- the CPU restatement that tests/test_primary_ref.py
pins to the C oracle. Frames are 70x44 (partial 8x8 tiles on both edges) unless stated. The reference of a scene is
computed once per session and shared.

The kernel has one instance, on the multi-draw loop; the record layout its leaves read (pair or single records, the
frame plan's choice) is a run-time switch inside it, so there is no instance to assert as taken: WCPT_OPTION_PAIR_RECORDS 0
and 1 run its two branches, and WCPT_OPTION_TRIANGLE_CACHE and WCPT_OPTION_PACKED_REFS change what the frame preparation
hands it (the leaf scan's packed stack entries or node indices). The same records are required under each."""
import copy

import numpy as np
import pytest

import oracle
import wcpt
from wcpt import scene as wscene

import primary_cases as cases
import primary_ref
from deep_tree import deep_chain_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = cases.W, cases.H
REC = T.PRIMARY_HIT_DTYPE
SENTINEL = 0xA5


def words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(rec.shape + (12,))


def assert_same(got, want, what=""):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = (g != w).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} records differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{g[bad][0]} != {w[bad][0]}"


def ref(name):
    return primary_ref.reference(name, cases.scene(name), W, H)[0]


class Run:
    """One context with a resident scene and a screen."""

    def __init__(self, s, w=W, h=H, options=()):
        self.s, self.w, self.h = s, w, h
        self.ctx = wcpt.Context(0)
        for o, v in options:
            self.ctx.set_option(o, v)
        self.dev = wcpt.DeviceScene(self.ctx, s)
        self.ctx.create_screen(w, h)

    def sd(self, frame=0, bounces=2):
        return self.s.scene_data(self.w, self.h, max_bounce=bounces, samples=1, frame=frame)

    def trace(self, rows=None):
        return self.ctx.trace_primary(self.sd(), self.dev.spheres, self.dev.draws, rows=rows)

    def pick(self, x, y):
        return self.ctx.pick(self.sd(), self.dev.spheres, self.dev.draws, x, y)[0]

    def render(self, frame, bounces=2):
        self.ctx.render(self.sd(frame, bounces), *self.dev.addresses())

    def image(self, rows=None):
        self.ctx.sync()
        return self.ctx.readback(self.h if rows is None else rows)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dev.free()
        self.ctx.close()


_gpu = {}


def gpu_frame(name):
    """The whole-frame pass of a scene on the GPU, run once per session."""
    if name not in _gpu:
        with Run(cases.scene(name)) as r:
            _gpu[name] = r.trace()
        _gpu[name].setflags(write=False)
    return _gpu[name]


# ---- the whole frame ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.SCENES)
def test_whole_frame_matches_reference(name):
    """Every record of the frame, and -- from the reference -- that the scene carries the kinds it is there for. The two
    tie scenes are among them: two coincident quads in two draw commands report draw 0, a sphere at two indices the first."""
    want = ref(name)
    cases.assert_kinds(name, want)
    got = gpu_frame(name)
    assert got.dtype == REC and got.shape == (H, W)
    assert_same(got, want, name)
    assert not got["_pad"].any()


def test_two_different_draws_are_told_apart():
    """mixed_draws on the GPU's own records: triangle hits of draw 0 (the Cornell mesh) and of draw 1 (the two quads, one
    facing the camera and one facing away), each with the normal of its own draw's triangle."""
    g = gpu_frame("mixed_draws")
    cases.assert_kinds("mixed_draws", g)
    tri = (g["kind"] & T.HIT_KIND_MASK) == T.HIT_TRIANGLE
    assert set(g["draw"][tri]) == {0, 1}
    # with the quads taken away the pixels that showed them show draw 0 or nothing, and every other record stays
    c = gpu_frame("cornell")
    quad = tri & (g["draw"] == 1)
    assert_same(g[~quad], c[~quad], "beside the quads")
    assert (words(g[quad]) != words(c[quad])).any(axis=-1).all()


def test_ties_report_the_earlier_primitive():
    q = gpu_frame("tie_quads")
    tri = (q["kind"] & T.HIT_KIND_MASK) == T.HIT_TRIANGLE
    assert tri.sum() > 100 and not q["draw"][tri].any()
    assert_same(q, gpu_frame("behind_quad"), "the second, coincident draw changes nothing")
    s = gpu_frame("tie_spheres")
    sph = (s["kind"] & T.HIT_KIND_MASK) == T.HIT_SPHERE
    assert (s["index"][sph] == 1).sum() > 100 and not (s["index"][sph] == 2).any()
    assert not s["material"][sph & (s["index"] == 1)].any()       # index 1's material 0, not the duplicate's 2


# ---- layouts -----------------------------------------------------------------------------------------------------------
def _frame_rows(layout):
    y_first, rows, stripe, period = layout
    ly = np.arange(rows)
    return y_first + ly + ((ly // stripe) * (period - stripe) if stripe else 0)


@pytest.mark.parametrize("layout", [(8, 24, 0, 0), (4, 24, 8, 16), (12, 16, 8, 16)])
def test_row_range_and_stripes(layout):
    """A row block and interleaved stripes: the context's rows back to back equal the whole-frame pass's rows."""
    with Run(cases.scene("cornell")) as r:
        if layout[2]:
            r.ctx.set_row_stripes(*layout)
        else:
            r.ctx.set_row_range(layout[0], layout[1])
        got = r.trace(rows=layout[1])
    assert got.shape == (layout[1], W)
    assert_same(got, ref("cornell")[_frame_rows(layout)], str(layout))


@pytest.mark.parametrize("size", [(1, 1), (9, 3), (8, 8)])
def test_small_frames(size):
    """One pixel, a frame of two slivers, exactly one tile."""
    w, h = size
    s = cases.scene("cornell")
    with Run(s, w, h) as r:
        got = r.trace()
    assert_same(got, primary_ref.trace(s, w, h)[0], str(size))


# ---- the pick ------------------------------------------------------------------------------------------------------------
def _pick_pixels(want):
    """Corners, edge pixels and pixels of every kind and facing the reference holds: about 40."""
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2),
          (7, 7), (8, 8), (63, 39), (64, 40), (69, 43)]
    k = want["kind"] & T.HIT_KIND_MASK
    front = (want["kind"] & T.HIT_FRONT) != 0
    rng = np.random.default_rng(5)
    for kind in (T.HIT_MISS, T.HIT_SPHERE, T.HIT_TRIANGLE):
        for f in (False, True):
            ys, xs = np.nonzero((k == kind) & (front == f))
            for i in rng.permutation(len(ys))[:5]:
                px.append((int(xs[i]), int(ys[i])))
    ys, xs = np.nonzero((k == T.HIT_TRIANGLE) & (want["draw"] == 1))      # a second draw's triangles, where there is one
    for i in rng.permutation(len(ys))[:4]:
        px.append((int(xs[i]), int(ys[i])))
    return px


@pytest.mark.parametrize("name", ["every_kind", "two_draws", "mixed_draws"])
def test_pick_equals_the_frames_record(name):
    want = ref(name)
    frame = gpu_frame(name)
    px = _pick_pixels(want)
    assert 25 <= len(px) <= 50
    if name == "mixed_draws":
        assert {int(want["draw"][y, x]) for x, y in px} == {0, 1}
    kinds = set()
    with Run(cases.scene(name)) as r:
        for x, y in px:
            got = r.pick(x, y)
            assert_same(np.array([got]), np.array([frame[y, x]]), f"{name} ({x}, {y})")
            assert_same(np.array([got]), np.array([want[y, x]]), f"{name} ({x}, {y}) against the reference")
            kinds.add(int(got["kind"]))
        # a context that holds rows [8, 32) only: pixels inside and outside its rows
        r.ctx.set_row_range(8, 24)
        for x, y in px[:13] + [(3, 8), (3, 31), (3, 7), (3, 32), (66, 20)]:
            got = r.pick(x, y)
            assert_same(np.array([got]), np.array([frame[y, x]]), f"{name} rows [8, 32) ({x}, {y})")
    assert {v & T.HIT_KIND_MASK for v in kinds} == {T.HIT_MISS, T.HIT_SPHERE, T.HIT_TRIANGLE}


# ---- what the frame preparation hands the kernel -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "two_draws", "mixed_draws", "reference_init"])
@pytest.mark.parametrize("options", [((T.OPTION_PAIR_RECORDS, 0),), ((T.OPTION_PAIR_RECORDS, 1),),
                                     ((T.OPTION_TRIANGLE_CACHE, 0),), ((T.OPTION_PACKED_REFS, 0),)],
                         ids=["singles", "pairs", "no_triangle_cache", "node_refs"])
def test_record_layout_options(name, options):
    """Both record layouts (with WCPT_OPTION_PAIR_RECORDS 1 the pass reads pair records, the primary-ray ones where the
    preparation made them; with 0 single records), no triangle cache (no leaf scan: node-index stack entries), and one
    and two draws: the same records."""
    with Run(cases.scene(name), options=options) as r:
        got = r.trace()
        r.render(0)          # a render of the same preparation in between
        again = r.trace()
    assert_same(got, ref(name), f"{name} {options}")
    assert_same(again, ref(name), f"{name} {options}, after a render")


# ---- non-interference ----------------------------------------------------------------------------------------------------
def _frames(overlap, interleave):
    """Frames 0-4 of cornell, optionally with a pass and a pick between every two renders: the images, the statistics, what
    wcpt_last_kernel / wcpt_last_arith said after each step, and the passes' records."""
    options = () if overlap is None else ((T.OPTION_FRAME_OVERLAP, overlap),)
    with Run(cases.scene("cornell"), options=options) as r:
        nbytes = W * H * REC.itemsize
        buf = r.ctx.buffer_alloc(nbytes)      # before frame 0: an allocation is a new generation of the scene
        imgs, said, recs, picks = [], [], [], []
        for f in range(5):
            r.render(f)
            said.append((r.ctx.last_kernel(), r.ctx.last_arith()))
            if interleave:
                r.ctx.trace_primary(r.sd(), r.dev.spheres, r.dev.draws, dst=r.ctx.buffer_address(buf), nbytes=nbytes)
                said.append((r.ctx.last_kernel(), r.ctx.last_arith()))
                picks.append(r.pick(W // 2, H // 2))
                said.append((r.ctx.last_kernel(), r.ctx.last_arith()))
                recs.append(np.frombuffer(r.ctx.buffer_download(buf, nbytes), REC).reshape(H, W))
            imgs.append(r.image())
        stats = (r.ctx.primary_cache_stats(), r.ctx.mk_split_stats(), r.ctx.mk_tiny_tree_stats())
        r.ctx.buffer_free(buf)
    return imgs, stats, said, recs, picks


@pytest.mark.parametrize("overlap", [None, 2], ids=["overlap_default", "overlap_forced"])
def test_renders_are_left_alone(overlap):
    plain_imgs, plain_stats, plain_said, _, _ = _frames(overlap, False)
    imgs, stats, said, recs, picks = _frames(overlap, True)
    for f, (a, b) in enumerate(zip(imgs, plain_imgs)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"frame {f}"
    assert stats[0] == plain_stats[0] == (1, 3)
    assert stats[1:] == plain_stats[1:]
    assert len(set(plain_said)) == 1 and set(said) == set(plain_said)      # the renders', after every step
    for f in range(5):
        assert_same(recs[f], ref("cornell"), f"pass after frame {f}")
        assert_same(np.array([picks[f]]), np.array([ref("cornell")[H // 2, W // 2]]), f"pick after frame {f}")


def test_always_exact():
    """WCPT_OPTION_ARITH 1 permits the renders' fast instances; the pass stays exact and says nothing about arithmetic."""
    with Run(cases.scene("cornell"), options=((T.OPTION_ARITH, T.ARITH_FAST),)) as r:
        got = r.trace()
        assert r.ctx.last_arith() == T.ARITH_EXACT       # no render yet
        r.render(0)
        assert r.ctx.last_arith() == T.ARITH_FAST
        again = r.trace()
        assert r.ctx.last_arith() == T.ARITH_FAST        # the render's
        p = r.pick(20, 30)
    assert_same(got, ref("cornell"), "fast arithmetic permitted")
    assert_same(again, ref("cornell"), "after a fast render")
    assert_same(np.array([p]), np.array([ref("cornell")[30, 20]]))


def test_follows_a_moved_sphere_and_a_refit():
    """The records are the current scene's: after a wcpt_buffer_upload that moves a sphere, and after
    wcpt_bvh_refit_device with moved vertices."""
    s = cases.scene("cornell")
    with Run(s) as r:
        assert_same(r.trace(), ref("cornell"), "before")
        moved = copy.copy(s)
        sp = s.spheres.copy()
        sp["position"][0] += np.array([0.21, 0.13, -0.17], np.float32)
        sp["radius"][0] *= np.float32(1.3)
        moved.spheres = sp
        r.ctx.buffer_upload(r.dev.buffers[1], sp)           # DeviceScene: materials, spheres, then each mesh's three
        want = primary_ref.trace(moved, W, H)[0]
        assert (words(want) != words(ref("cornell"))).any()
        assert_same(r.trace(), want, "sphere moved")
        m = s.meshes[0]
        pos = (np.asarray(m.positions, np.float32).reshape(-1, 3) * np.array([1.0, 0.85, 1.0], np.float32)
               + np.array([0.05, 0.0, 0.0], np.float32)).astype(np.float32)
        vb, ib, nb = r.dev.buffers[2:5]
        wscene.device_bvh_refit(r.ctx, vb, ib, nb, pos, m.indices.size, len(m.nodes))
        moved.meshes = [wscene.bvh_refit(m, pos)]
        want2 = primary_ref.trace(moved, W, H)[0]
        assert (words(want2) != words(want)).any()
        assert_same(r.trace(), want2, "mesh refitted")
        px = (W // 3, 2 * H // 3)
        assert_same(np.array([r.pick(*px)]), np.array([want2[px[1], px[0]]]), "pick after the refit")


# ---- the output's bounds ---------------------------------------------------------------------------------------------------
def test_output_bounds():
    """`dst` inside a larger buffer filled with a sentinel: the bytes before and after width * rows * 48 are unchanged."""
    pad = 4096
    nbytes = W * H * REC.itemsize
    with Run(cases.scene("cornell")) as r:
        buf = r.ctx.buffer_from(np.full(nbytes + 2 * pad, SENTINEL, np.uint8))
        r.ctx.trace_primary(r.sd(), r.dev.spheres, r.dev.draws, dst=r.ctx.buffer_address(buf) + pad, nbytes=nbytes)
        r.ctx.sync()
        out = np.frombuffer(r.ctx.buffer_download(buf, nbytes + 2 * pad), np.uint8)
        r.ctx.buffer_free(buf)
    assert (out[:pad] == SENTINEL).all() and (out[pad + nbytes:] == SENTINEL).all()
    assert_same(out[pad:pad + nbytes].view(REC).reshape(H, W), ref("cornell"), "inside")


# ---- refusals --------------------------------------------------------------------------------------------------------------
INVALID, NO_SCREEN = T.WCPT_ERROR_INVALID_ARGUMENT, T.WCPT_ERROR_NO_SCREEN


def _raw_trace(ctx, sd, spheres, draws, dst, nbytes):
    return wcpt.lib.wcpt_trace_primary(ctx.h, None if sd is None else T.ptr(sd), spheres, draws, dst, nbytes)


def _raw_pick(ctx, sd, spheres, draws, x, y, out):
    return wcpt.lib.wcpt_pick(ctx.h, None if sd is None else T.ptr(sd), spheres, draws, x, y,
                              None if out is None else T.ptr(out))


def test_refusals():
    """Every refusal returns its code with a message, writes nothing (the sentinel buffer and the pick's output stay) and
    launches nothing: the render that follows is bit-equal to one on a context that never saw a refused call."""
    s = cases.scene("cornell")
    nbytes = W * H * REC.itemsize
    with Run(s) as clean:
        clean.render(0)
        want_img = clean.image()
    with Run(s) as r:
        ctx = r.ctx
        sd = np.ascontiguousarray(r.sd(), dtype=T.SCENE_DATA_DTYPE)
        buf = ctx.buffer_from(np.full(nbytes, SENTINEL, np.uint8))
        dst = ctx.buffer_address(buf)
        out = np.full(1, 0, REC)
        out.view(np.uint8)[:] = SENTINEL
        sph, drw = r.dev.spheres, r.dev.draws
        bad_draw = np.zeros(1, T.DRAW_COMMAND_DTYPE)        # indexCount 3 with null buffers: check_draw refuses it
        bad_draw["indexCount"] = 3
        bad = ctx.buffer_address(ctx.buffer_from(bad_draw))
        sd1 = sd.copy()
        sd1["drawCommandCount"] = 1
        long_draw = np.frombuffer(ctx.buffer_download(r.dev.buffers[-1], 32), T.DRAW_COMMAND_DTYPE).copy()
        long_draw["indexCount"] = 3 * 10 ** 6               # more indices than its index buffer holds
        long_ = ctx.buffer_address(ctx.buffer_from(long_draw))
        cases_ = [
            ("null scene", _raw_trace(ctx, None, sph, drw, dst, nbytes), INVALID),
            ("null scene (pick)", _raw_pick(ctx, None, sph, drw, 1, 1, out), INVALID),
            ("null spheres", _raw_trace(ctx, sd, 0, drw, dst, nbytes), INVALID),
            ("null spheres (pick)", _raw_pick(ctx, sd, 0, drw, 1, 1, out), INVALID),
            ("null draws", _raw_trace(ctx, sd, sph, 0, dst, nbytes), INVALID),
            ("null draws (pick)", _raw_pick(ctx, sd, sph, 0, 1, 1, out), INVALID),
            ("draw with null buffers", _raw_trace(ctx, sd1, sph, bad, dst, nbytes), INVALID),
            ("draw with null buffers (pick)", _raw_pick(ctx, sd1, sph, bad, 1, 1, out), INVALID),
            ("indexCount past its buffer", _raw_trace(ctx, sd1, sph, long_, dst, nbytes), INVALID),
            ("indexCount past its buffer (pick)", _raw_pick(ctx, sd1, sph, long_, 1, 1, out), INVALID),
            ("null dst", _raw_trace(ctx, sd, sph, drw, 0, nbytes), INVALID),
            ("misaligned dst", _raw_trace(ctx, sd, sph, drw, dst + 8, nbytes - 8), INVALID),
            ("dst one byte short", _raw_trace(ctx, sd, sph, drw, dst, nbytes - 1), INVALID),
            ("null out", _raw_pick(ctx, sd, sph, drw, 1, 1, None), INVALID),
            ("x == width", _raw_pick(ctx, sd, sph, drw, W, 0, out), INVALID),
            ("y == height", _raw_pick(ctx, sd, sph, drw, 0, H, out), INVALID),
        ]
        for what, rc, code in cases_:
            assert rc == code, (what, rc)
        assert wcpt.lib.wcpt_last_error(ctx.h)
        # through the wrapper, which hands on the size the caller states for its memory
        with pytest.raises(wcpt.WcptError) as e:
            ctx.trace_primary(sd, sph, drw, dst=dst, nbytes=nbytes - 48)
        assert e.value.code == INVALID
        with pytest.raises(ValueError):
            ctx.trace_primary(sd, sph, drw, dst=dst)
        ctx.sync()
        assert (np.frombuffer(ctx.buffer_download(buf, nbytes), np.uint8) == SENTINEL).all()
        assert (out.view(np.uint8) == SENTINEL).all()
        r.render(0)
        assert np.array_equal(r.image().view(np.uint32), want_img.view(np.uint32))
        # and the calls work on this context afterwards
        assert_same(r.trace(), ref("cornell"), "after the refusals")
    # no screen
    ctx = wcpt.Context(0)
    try:
        dev = wcpt.DeviceScene(ctx, s)
        buf = ctx.buffer_from(np.full(nbytes, SENTINEL, np.uint8))
        sd = np.ascontiguousarray(s.scene_data(W, H), dtype=T.SCENE_DATA_DTYPE)
        out = np.zeros(1, REC)
        assert _raw_trace(ctx, sd, dev.spheres, dev.draws, ctx.buffer_address(buf), nbytes) == NO_SCREEN
        assert _raw_pick(ctx, sd, dev.spheres, dev.draws, 0, 0, out) == NO_SCREEN
        assert (np.frombuffer(ctx.buffer_download(buf, nbytes), np.uint8) == SENTINEL).all()
    finally:
        ctx.close()


def test_region_timing_counts_launched_passes_only():
    """WCPT_OPTION_PROFILE_REGION 1: a pass counts like a render, a pick does not, and a pass that the frame preparation
    refuses (a draw command with null buffers) was no launch."""
    s = cases.scene("cornell")
    nbytes = W * H * REC.itemsize
    with Run(s, options=((T.OPTION_PROFILE_REGION, 1),)) as r:
        ctx = r.ctx
        buf = ctx.buffer_alloc(nbytes)
        dst = ctx.buffer_address(buf)
        bad_draw = np.zeros(1, T.DRAW_COMMAND_DTYPE)
        bad_draw["indexCount"] = 3
        bad = ctx.buffer_address(ctx.buffer_from(bad_draw))
        sd = np.ascontiguousarray(r.sd(), dtype=T.SCENE_DATA_DTYPE)
        ctx.profile_begin()
        assert _raw_trace(ctx, sd, r.dev.spheres, bad, dst, nbytes) == INVALID
        r.pick(3, 3)
        assert ctx.profile_end() == (0.0, 0)
        ctx.profile_begin()
        ctx.trace_primary(sd, r.dev.spheres, r.dev.draws, dst=dst, nbytes=nbytes)
        assert _raw_trace(ctx, sd, r.dev.spheres, bad, dst, nbytes) == INVALID
        ctx.trace_primary(sd, r.dev.spheres, r.dev.draws, dst=dst, nbytes=nbytes)
        ms, n = ctx.profile_end()
        assert n == 2 and ms > 0.0
        ctx.buffer_free(buf)


def test_refuses_a_frame_that_is_not_renderable():
    """A context whose rows cover more than 2^26 - 1 tiles (screen_layout.h layout_renderable). Its image would take 128
    GiB, so the frame is created over an external image that is only claimed, not allocated: creating a screen over an
    external image touches no memory, and every entry point that would use it refuses first. Each call here is refused
    twice over -- the null output it passes is refused by the check that follows the one under test -- so neither can
    launch; the message says which check answered."""
    ctx = wcpt.Context(0)
    try:
        small = ctx.buffer_alloc(4096)
        ctx.set_external_image(ctx.buffer_address(small), 1 << 38)
        ctx.create_screen(1 << 17, 1 << 16)                 # 2^14 x 2^13 = 2^27 tiles
        sd = np.zeros((), T.SCENE_DATA_DTYPE)
        assert _raw_trace(ctx, sd, 0, 0, 0, 0) == INVALID
        assert b"8x8 tiles" in wcpt.lib.wcpt_last_error(ctx.h)
        assert _raw_pick(ctx, sd, 0, 0, 0, 0, None) == INVALID
        assert b"8x8 tiles" in wcpt.lib.wcpt_last_error(ctx.h)
    finally:
        ctx.close()


# ---- the traversal stack ---------------------------------------------------------------------------------------------------
def test_stack_overflow_is_reported_once():
    """The chain of tests/deep_tree.py with 49 levels does not fit the 48-entry stack (tests/test_gpu_stack_overflow.py has
    the reading of the code: a refused push stores nothing and sets a flag; the subtree is not visited). The pass runs
    the same interior_step on the same LdsStack<16, 32>: it completes, the next sync returns WCPT_ERROR_STACK_OVERFLOW once,
    and the context stays usable. The pick returns it itself."""
    over = deep_chain_scene(cases.get_scene("default"), levels=49)
    fits = deep_chain_scene(cases.get_scene("default"), levels=48)
    w, h = 48, 32
    with Run(fits, w, h) as r:
        assert_same(r.trace(), primary_ref.trace(fits, w, h)[0], "48 levels fill the last entry")
    with Run(over, w, h) as r:
        nbytes = w * h * REC.itemsize
        buf = r.ctx.buffer_alloc(nbytes)
        r.ctx.trace_primary(r.sd(), r.dev.spheres, r.dev.draws, dst=r.ctx.buffer_address(buf), nbytes=nbytes)
        with pytest.raises(wcpt.WcptError) as e:
            r.ctx.sync()
        assert e.value.code == T.WCPT_ERROR_STACK_OVERFLOW
        r.ctx.sync()                                        # reported once
        got = np.frombuffer(r.ctx.buffer_download(buf, nbytes), REC).reshape(h, w)
        want = primary_ref.trace(over, w, h)[0]
        # the one leaf whose push was refused is the last level's, triangle 48: only a pixel that shows it may differ
        same = (words(got) == words(want)).all(axis=-1)
        shows_48 = ((want["kind"] & T.HIT_KIND_MASK) == T.HIT_TRIANGLE) & (want["index"] == 48)
        assert not (~same & ~shows_48).any()
        # every box of the chain is the mesh's whole box: a ray that shows one of its triangles walked to the bottom (no
        # sphere cut it short, and a hit inside the box culls no later box) and overflowed; a ray that misses the box
        # never pushes. The pick returns the code itself for the one and is clean for the other.
        sd = np.ascontiguousarray(r.sd(), dtype=T.SCENE_DATA_DTYPE)
        ys, xs = np.nonzero((want["kind"] & T.HIT_KIND_MASK) == T.HIT_TRIANGLE)
        assert len(ys) > 0
        out = np.zeros(1, REC)
        assert _raw_pick(r.ctx, sd, r.dev.spheres, r.dev.draws, int(xs[0]), int(ys[0]), out) == T.WCPT_ERROR_STACK_OVERFLOW
        assert_same(out, np.array([want[ys[0], xs[0]]]), "the record is filled all the same")
        r.ctx.sync()
        root = over.meshes[0].nodes[0]
        beside = None
        for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
            t = oracle.ray_box(sd["position"], primary_ref.directions(sd, w, h, [x], [y])[0], root["min"], root["max"])
            if t[0] > t[1] or t[1] < 0.0:
                beside = (x, y)
        assert beside is not None
        assert_same(np.array([r.pick(*beside)]), np.array([want[beside[1], beside[0]]]), "a ray beside the chain")
        r.ctx.buffer_free(buf)


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_renderer_pick_and_editor_select():
    """The mirror of the reference's Init scene (the mushroom and four spheres): PathTracingRenderer.Pick returns the
    record and the hit point, Editor.select sets selectedSphere to the sphere under the pixel and to -1 on the mesh and on
    the sky, and no frame counter moves."""
    s = cases.scene("reference_init")
    want = ref("reference_init")
    k = want["kind"] & T.HIT_KIND_MASK
    pr = wcpt.PathTracingRenderer(0)
    try:
        pr.Init(scene=s)
        pr.CreateScreen((W, H))
        ed = wcpt.Editor(pr, s.camera)
        assert ed.selectedSphere == -1
        ed.frame(moved=True)
        counted = pr.renderedFramesCount
        rng = np.random.default_rng(9)
        seen = set()
        for kind in (T.HIT_SPHERE, T.HIT_TRIANGLE, T.HIT_MISS, T.HIT_SPHERE):
            ys, xs = np.nonzero(k == kind)
            for i in rng.permutation(len(ys))[:4]:
                x, y = int(xs[i]), int(ys[i])
                rec = ed.select(x, y)
                assert_same(np.array([rec]), np.array([want[y, x]]), f"select ({x}, {y})")
                assert ed.selectedSphere == (int(want["index"][y, x]) if kind == T.HIT_SPHERE else -1)
                seen.add(ed.selectedSphere)
                rec2, position = pr.Pick(wscene.update_camera(s.camera, W / H), x, y)
                assert_same(np.array([rec2]), np.array([want[y, x]]), f"Pick ({x}, {y})")
                o = np.asarray(pr.scene_data(wscene.update_camera(s.camera, W / H))["position"], np.float32)
                with np.errstate(over="ignore"):
                    expect = o + np.float32(want["t"][y, x]) * want["direction"][y, x].astype(np.float32)
                assert position.dtype == np.float32
                assert np.array_equal(position.view(np.uint32), expect.view(np.uint32))
        assert -1 in seen and len(seen) >= 2
        # a camera away from the origin: the hit point takes its position
        cam = wscene.update_camera(wscene.make_camera(position=(-0.7, 0.3, 0.4), yaw=10.0, pitch=-5.0, fov=80.0), W / H)
        sd = pr.scene_data(cam)
        px = [(W // 2, H // 2), (5, 5), (W - 3, H - 4), (20, 30)]
        moved = primary_ref.trace(s, W, H, sd=sd, pixels=px)[0]
        assert (moved["kind"] != 0).any()
        for (x, y), m in zip(px, moved):
            rec, position = pr.Pick(cam, x, y)
            assert_same(np.array([rec]), np.array([m]), f"moved camera ({x}, {y})")
            with np.errstate(over="ignore"):
                expect = np.asarray(sd["position"], np.float32) + np.float32(m["t"]) * m["direction"].astype(np.float32)
            assert np.array_equal(position.view(np.uint32), expect.view(np.uint32))
        assert pr.renderedFramesCount == counted
        assert ed.frame() == counted + 1                    # the accumulation goes on
    finally:
        pr.Deinit()
