"""Tiny trees (WCPT_OPTION_MK_TINY_TREE) on the GPU: a draw whose BVH is a root leaf or a root over two leaves is walked
without the megakernel's traversal loop (pt_device.h tiny_walk, csrc/mk_tiny_rule.h). Same tests, same order, same
culls per lane, so every sequence here equals, bit for bit, the same sequence on a context with the option at 0, and in
exact arithmetic the CPU oracle's accumulation.

The walk is compiled into the two launches of a split render (exact arithmetic, pair records, one draw command:
pt_device.h kTinyWalk), so each scene runs with a forced cut, where the walk runs, and whole, where the loop runs; both
against the option at 0 and the oracle.

Every case asserts on the host nodes that the tree has the shape it is here for, and through wcpt_mk_tiny_tree_stats that
the render took an instance that holds the walk with the draw's flag set (or did not). The count is per render, not per
wave, so it shows the path was selected, not which waves of a frame took which order. 76x40 leaves a partial 8x8 tile column.
The oracle's images are computed once per module and shared.

The two cubes' 12 / 12 tree is written out (tiny_scenes.two_leaf_bvh): the midpoint builder halves each cube once more,
so it has no tree of two 12-triangle leaves with distinct boxes to offer."""
import copy

import numpy as np
import pytest

import wcpt
import oracle
from wcpt import scene as wscene

import tiny_scenes as ts
from test_gpu_parity import assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 76, 40
FRAMES = range(4)


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def _with_meshes(meshes, camera, spheres=False):
    s = copy.copy(get_scene("cornell"))
    if not spheres:
        s.spheres = s.spheres[:0]
    s.meshes = meshes
    s.camera = camera
    return s


_built = {}


def _scene(name):
    if name in _built:
        return _built[name]
    front = wscene.make_camera(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)
    if name == "cornell":
        s = get_scene("cornell")
    elif name.startswith("stack"):
        s = _with_meshes([wscene.bvh_build(ts.stack(int(name[5:])))], front)
    elif name.startswith("strip"):
        s = _with_meshes([wscene.bvh_build(ts.strip(int(name[5:])))], front)
    elif name == "boxes_between":   # between the cubes and in front of them, looking along -z
        s = _with_meshes([ts.two_leaf_bvh(ts.two_boxes_mesh(), 12)],
                         wscene.make_camera(position=(0.0, 0.1, 1.5), yaw=-90.0, pitch=0.0, fov=90.0))
    elif name == "boxes_in_line":   # one cube straight behind the other, looking along -x
        s = _with_meshes([ts.two_leaf_bvh(ts.two_boxes_mesh(), 12)],
                         wscene.make_camera(position=(2.5, 0.05, 0.02), yaw=180.0, pitch=0.0, fov=90.0))
    elif name == "two_tiny_draws":
        s = _with_meshes([wscene.bvh_build(ts.stack(3)), wscene.bvh_build(ts.strip(3))], front)
    else:
        raise KeyError(name)
    _built[name] = s
    return s


def _cameras(s, moved):
    """per frame: None (the scene's camera), or a camera that moves a little every frame"""
    if not moved:
        return [None for _ in FRAMES]
    p = [float(v) for v in s.camera.position]
    return [wscene.make_camera(position=(p[0] + 0.03 * f, p[1] - 0.02 * f, p[2] + 0.01 * f), yaw=s.camera.yaw + 2.0 * f,
                               pitch=s.camera.pitch, fov=s.camera.fov) for f in FRAMES]


def _sequence(s, tiny, w=W, h=H, bounces=4, spp=1, cache=True, split=0, arith=0, moved=False, pairs=1):
    """The image after each frame, and the renders the context counted on the tiny-tree walk."""
    ctx = wcpt.Context(0)
    try:
        ctx.set_option(T.OPTION_MK_TINY_TREE, tiny)
        ctx.set_option(T.OPTION_PAIR_RECORDS, pairs)   # a mesh of a few triangles takes single records by itself
        ctx.set_option(T.OPTION_PRIMARY_CACHE, 1 if cache else 0)
        ctx.set_option(T.OPTION_MK_SPLIT, split)
        ctx.set_option(T.OPTION_ARITH, arith)
        dev = wcpt.DeviceScene(ctx, s)
        ctx.create_screen(w, h)
        imgs = []
        for f, cam in zip(FRAMES, _cameras(s, moved)):
            ctx.render(s.scene_data(w, h, max_bounce=bounces, samples=spp, frame=f, camera=cam), *dev.addresses())
            ctx.sync()
            imgs.append(ctx.readback(h))
        n = ctx.mk_tiny_tree_stats()
        dev.free()
        return imgs, n
    finally:
        ctx.close()


_oracles = {}


def _oracle_acc(name, w, h, bounces, spp=1, moved=False):
    key = (name, w, h, bounces, spp, moved)
    if key not in _oracles:
        s, acc, out = _scene(name), None, []
        for f, cam in zip(FRAMES, _cameras(s, moved)):
            sd = s.scene_data(w, h, max_bounce=bounces, samples=spp, frame=f, camera=cam)
            acc, _ = oracle.render_scene(s, w, h, sd=sd, image=acc, threads=8)
            out.append(acc.copy())
        _oracles[key] = out
    return _oracles[key]


def _check(name, w=W, h=H, bounces=4, spp=1, moved=False, expect_tiny=True, **kw):
    """on against off bit for bit, the walk counted on every render (or on none), and -- exact arithmetic -- the oracle.
    expect_tiny: the draw's tree is tiny; the walk then runs iff the render splits (a forced cut, one sample) in exact
    arithmetic"""
    s = _scene(name)
    on, n_on = _sequence(s, 1, w, h, bounces, spp, moved=moved, **kw)
    off, n_off = _sequence(s, 0, w, h, bounces, spp, moved=moved, **kw)
    assert n_off == 0
    runs = expect_tiny and kw.get("split", 0) != 0 and spp == 1 and kw.get("arith", 0) == 0
    assert n_on == (len(FRAMES) if runs else 0)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"frame {i}: the walk differs from the loop"
    if kw.get("arith", 0) == 0:
        for a, ref in zip(on, _oracle_acc(name, w, h, bounces, spp, moved)):
            assert_close(a, ref)
    return on


# ---- 1. the Cornell box: a root over two 17-triangle leaves with the same box -----------------------------------------
def test_cornell_tree_shape():
    assert ts.shape(_scene("cornell").meshes[0]) == [(1, 0), (0, 51), (51, 51)]


@pytest.mark.parametrize("cache", [True, False])
def test_cornell_primary_cache(cache):
    """frame 0 plain, frame 1 writes the cache, frames 2-3 read it (every primary-cache build); without the cache every
    frame traces its primary segment on the primary-ray records"""
    _check("cornell", cache=cache, split=3)
    _check("cornell", cache=cache)


@pytest.mark.parametrize("cut", [1, 2, 3])
def test_cornell_split(cut):
    """head and tail instances at every cut"""
    _check("cornell", split=cut)


def test_cornell_two_samples():
    """samples > 1 never split (the sample-reuse builds are whole kernels): the loop"""
    _check("cornell", spp=2)
    _check("cornell", spp=2, split=3)


def test_cornell_moved_camera():
    _check("cornell", moved=True, split=2)
    _check("cornell", moved=True)


def test_cornell_fast_arithmetic():
    """the fast-arithmetic instances keep the loop (pt_device.h kTinyWalk): the option changes neither their bits nor
    their path"""
    _check("cornell", arith=1)
    _check("cornell", arith=1, split=3)


def test_automatic_is_on_and_the_option_is_checked():
    s = _scene("cornell")
    imgs, n = _sequence(s, -1, split=3)
    assert n == len(FRAMES)
    for a, ref in zip(imgs, _oracle_acc("cornell", W, H, 4)):
        assert_close(a, ref)
    ctx = wcpt.Context(0)
    try:
        for bad in (-2, 2, 100):
            with pytest.raises(wcpt.WcptError):
                ctx.set_option(T.OPTION_MK_TINY_TREE, bad)
    finally:
        ctx.close()


def test_single_records_keep_the_loop():
    """the walk lives in the pair-record instances only"""
    imgs, n = _sequence(_scene("cornell"), 1, pairs=0, split=3)
    assert n == 0
    for a, ref in zip(imgs, _oracle_acc("cornell", W, H, 4)):
        assert_close(a, ref)


def _primary_orders(s, w, h):
    """Host side, binary64: per 8x8 tile of the primary rays, how many lanes inside the root's box pop the left child
    first and how many the right (interior_step's leftDist < rightDist). Not bit-exact with the kernel, and not needed
    to be: it shows which tiles hold both orders."""
    sd = s.scene_data(w, h)
    P = np.asarray(sd["inverseProjection"], np.float64).reshape(4, 4).T   # column-major
    V = np.asarray(sd["inverseView"], np.float64).reshape(4, 4).T
    o = np.asarray(sd["position"], np.float64)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    cx = ((x + 0.5) / w) * 2.0 - 1.0
    cy = (1.0 - (y + 0.5) / h) * 2.0 - 1.0
    t = np.einsum("rc,chw->rhw", P, np.stack([cx, cy, np.ones_like(cx), np.ones_like(cx)]))
    d = t[:3] / t[3]
    d /= np.linalg.norm(d, axis=0)
    wd = np.einsum("rc,chw->rhw", V[:3, :3], d)
    wd /= np.linalg.norm(wd, axis=0)

    def box(node):
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / wd
            lo = (np.asarray(node["min"], np.float64)[:, None, None] - o[:, None, None]) * inv
            hi = (np.asarray(node["max"], np.float64)[:, None, None] - o[:, None, None]) * inv
        return np.minimum(lo, hi).max(axis=0), np.maximum(lo, hi).min(axis=0)

    nodes = s.meshes[0].nodes
    c0, c1 = box(nodes[0])
    inside = ~((c0 > c1) | (c1 < 0.0))
    left = int(nodes[0]["leftNodeOrTriangleIndex"])
    l0, l1 = box(nodes[left])
    r0, r1 = box(nodes[left + 1])
    left_first = np.where(l0 > 0.0, l0, l1) < np.where(r0 > 0.0, r0, r1)
    out = []
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            m = inside[ty:ty + 8, tx:tx + 8]
            lf = left_first[ty:ty + 8, tx:tx + 8]
            out.append((int((m & lf).sum()), int((m & ~lf).sum())))
    return out


def test_the_two_cube_camera_mixes_the_orders_in_a_wave_and_cornell_does_not():
    """wcpt_mk_tiny_tree_stats counts renders, not waves: that the camera between the cubes gives waves whose lanes
    disagree on the near child (and waves of one order alone) is shown here from the rays, on the host"""
    tiles = _primary_orders(_scene("boxes_between"), 64, 32)
    assert any(a > 0 and b > 0 for a, b in tiles), tiles
    assert any(a == 0 and b > 0 for a, b in tiles), tiles   # and waves of one order alone
    assert all(a == 0 for a, b in _primary_orders(_scene("cornell"), W, H))   # equal boxes: never left first


# ---- 2. two cubes, distinct leaf boxes: waves whose lanes disagree on the near child, and a far leaf culled by rec.t --
@pytest.mark.parametrize("name", ["boxes_between", "boxes_in_line"])
def test_two_boxes(name):
    bvh = _scene(name).meshes[0]
    assert ts.shape(bvh) == [(1, 0), (0, 36), (36, 36)]
    assert not np.array_equal(bvh.nodes[1]["min"], bvh.nodes[2]["min"])
    _check(name, 64, 32)
    _check(name, 64, 32, split=2)


# ---- 3. root leaves; an odd count leaves the last pair's second slot NaN ---------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_root_leaf(n):
    name = f"stack{n}"
    assert ts.shape(_scene(name).meshes[0]) == [(0, 3 * n)]
    imgs = _check(name, 64, 32, bounces=3, split=1)
    _check(name, 64, 32, bounces=3)
    assert not np.array_equal(_bits(imgs[0]), _bits(_sequence(_with_meshes([], _scene(name).camera), 1, 64, 32, 3)[0][0]))


# ---- 4. not tiny ------------------------------------------------------------------------------------------------------
def test_one_split_past_tiny_keeps_the_loop():
    bvh = _scene("strip5").meshes[0]
    assert len(bvh.nodes) == 5 and len(_scene("strip4").meshes[0].nodes) == 3
    _check("strip5", 64, 32, bounces=3, split=2, expect_tiny=False)
    _check("strip4", 64, 32, bounces=3, split=2)


def test_two_tiny_draws_keep_the_loop():
    s = _scene("two_tiny_draws")
    assert [len(m.nodes) for m in s.meshes] == [1, 3]
    _check("two_tiny_draws", 64, 32, bounces=3, split=2, expect_tiny=False)
