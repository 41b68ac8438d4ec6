"""The walk-only kernels of tiny-tree renders (wc-path-tracer_amd/csrc/pt_mk_tiny.hip: pt_tiny_head<none | write | read>
and pt_tiny_tail; the walk in csrc/pt_tiny.h, the selection in csrc/mk_tiny_rule.h mk_tiny_kernels) on the GPU.

A split render of one draw with a tiny tree, on pair records in exact arithmetic, runs on these four kernels; with
WCPT_OPTION_MK_TINY_TREE at 0 the same context runs the general head and tail and their traversal loop. Same tests, same
order, same culls per lane: every sequence here (76x40 -- a partial tile column --, 4 frames: plain, cache write, two cache
reads) equals the option-0 sequence bit for bit and, being exact arithmetic, the CPU oracle's accumulation
(test_gpu_tiny_tree.py's _check pattern), and wcpt_mk_tiny_tree_stats says the pair was selected on every render.

What these kernels do on their own:
  - a pair record that both leaves own a slot of is tested once per ray and segment and applied in either leaf: the two
    cubes' 24 triangles cut at 11 and 13 (a shared pair) and at 12 (none), and hand-written trees whose left range lies
    behind the right one in the index buffer, or with unused triangles between the ranges;
  - a wave whose lanes agree on the near child runs its two leaves without the four turns, any other wave keeps them:
    the camera between the cubes puts both orders into one wave (asserted on the host from the rays), the camera in
    line gives waves of one order;
  - their own store path: a row range, every gather payload format, a width that is no whole tile.
The oracle's images are computed once per case and shared."""
import numpy as np
import pytest

import wcpt
import oracle
from wcpt import scene as wscene
from wcpt._lib import NODE_DTYPE

import tiny_scenes as ts
import test_gpu_tiny_tree as tt
from test_gpu_parity import assert_close, get_scene

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = 76, 40
FRAMES = tt.FRAMES

BETWEEN = dict(position=(0.0, 0.1, 1.5), yaw=-90.0, pitch=0.0, fov=90.0)   # between the cubes, looking along -z
IN_LINE = dict(position=(2.5, 0.05, 0.02), yaw=180.0, pitch=0.0, fov=90.0)  # one cube behind the other, along -x
CLOSE = dict(position=(0.0, 0.1, 0.2), yaw=-90.0, pitch=0.0, fov=90.0)     # between the cubes, inside the root's box
FRONT = dict(position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=90.0)


def _ranges_bvh(mesh, left, right):
    """A root over two leaves of the triangle ranges left = (first, end) and right = (first, end), each with its exact
    box, in any order and at any distance in the index buffer; the root's box holds both."""
    pos, idx = mesh.positions, mesh.indices
    nodes = np.zeros(3, NODE_DTYPE)
    for node, (a, b) in ((nodes[1], left), (nodes[2], right)):
        v = pos[idx[3 * a:3 * b]]
        node["min"], node["max"] = v.min(axis=0), v.max(axis=0)
        node["leftNodeOrTriangleIndex"], node["triangleCount"] = 3 * a, 3 * (b - a)
    nodes[0]["min"] = np.minimum(nodes[1]["min"], nodes[2]["min"])
    nodes[0]["max"] = np.maximum(nodes[1]["max"], nodes[2]["max"])
    nodes[0]["leftNodeOrTriangleIndex"], nodes[0]["triangleCount"] = 1, 0
    return wscene.HostBVH(pos.copy(), idx.copy(), nodes)


_scenes = {}


def _scene(name):
    if name not in _scenes:
        if name == "cornell":
            s = get_scene("cornell")
        elif name.startswith("cut"):       # cut<k>_<camera>: the two cubes, the left leaf their first k triangles
            k, cam = name[3:].split("_", 1)
            s = tt._with_meshes([ts.two_leaf_bvh(ts.two_boxes_mesh(), int(k))],
                                wscene.make_camera(**{"between": BETWEEN, "in_line": IN_LINE, "close": CLOSE}[cam]))
        elif name == "behind":             # the left child's triangles lie behind the right child's; they share pair (10, 11)
            s = tt._with_meshes([_ranges_bvh(ts.two_boxes_mesh(), (11, 24), (0, 11))], wscene.make_camera(**BETWEEN))
        elif name == "gap":                # triangles 9 .. 14 belong to no leaf; either leaf owns one slot of its edge pair
            s = tt._with_meshes([_ranges_bvh(ts.two_boxes_mesh(), (0, 9), (15, 24))], wscene.make_camera(**BETWEEN))
        elif name.startswith("stack"):
            s = tt._with_meshes([wscene.bvh_build(ts.stack(int(name[5:])))], wscene.make_camera(**FRONT))
        else:
            raise KeyError(name)
        _scenes[name] = s
    return _scenes[name]


_oracles = {}


def _oracle_acc(name, w, h, bounces, moved):
    key = (name, w, h, bounces, moved)
    if key not in _oracles:
        s, acc, out = _scene(name), None, []
        for f, cam in zip(FRAMES, tt._cameras(s, moved)):
            sd = s.scene_data(w, h, max_bounce=bounces, samples=1, frame=f, camera=cam)
            acc, _ = oracle.render_scene(s, w, h, sd=sd, image=acc, threads=8)
            out.append(acc.copy())
        _oracles[key] = out
    return _oracles[key]


def _check(name, w=W, h=H, bounces=4, moved=False, split=2, cache=True):
    """the walk-only kernels against the general ones bit for bit, selected on every render, and the oracle"""
    s = _scene(name)
    on, n_on = tt._sequence(s, 1, w, h, bounces, 1, cache=cache, split=split, moved=moved)
    off, n_off = tt._sequence(s, 0, w, h, bounces, 1, cache=cache, split=split, moved=moved)
    print(f"{name}: {w}x{h} cut {split} cache {cache} moved {moved}: tiny renders on {n_on} off {n_off}")
    assert n_off == 0 and n_on == len(FRAMES)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and np.array_equal(tt._bits(a), tt._bits(b)), f"frame {i}: differs from the general kernels"
    for a, ref in zip(on, _oracle_acc(name, w, h, bounces, moved)):
        assert_close(a, ref)
    return on


# ---- 1. leaf boundaries: a shared pair (odd cut) or none (even), both orders in a wave or one ------------------------
@pytest.mark.parametrize("camera", ["between", "in_line", "close"])
@pytest.mark.parametrize("k", [11, 12, 13])
def test_leaf_boundary(k, camera):
    """`between` is test_gpu_tiny_tree.py's camera in front of the cubes: its primary rays put both orders into one wave
    with the cut at 12 and 13; at 11 the right leaf's box holds the left one's and every primary wave has one order, so
    `close`, the same view from inside the root's box, is there to mix them at every cut"""
    s = _scene(f"cut{k}_{camera}")
    assert ts.shape(s.meshes[0]) == [(1, 0), (0, 3 * k), (3 * k, 72 - 3 * k)]
    # triangles k - 1 and k are the two slots of one pair record iff k is odd
    assert ((k - 1) // 2 == k // 2) == (k % 2 == 1)
    tiles = tt._primary_orders(s, W, H)
    if camera == "close" or (camera == "between" and k != 11):
        assert any(a > 0 and b > 0 for a, b in tiles), tiles    # waves whose lanes disagree: the four turns
    assert any((a == 0) != (b == 0) for a, b in tiles), tiles   # waves of one order: the two-leaf form
    _check(f"cut{k}_{camera}")


# ---- 2. hand-written trees: nothing is assumed of the ranges' order or distance --------------------------------------
def test_left_range_behind_the_right_one():
    bvh = _scene("behind").meshes[0]
    assert ts.shape(bvh) == [(1, 0), (33, 39), (0, 33)]
    _check("behind")


def test_unused_triangles_between_the_ranges():
    bvh = _scene("gap").meshes[0]
    assert ts.shape(bvh) == [(1, 0), (0, 27), (45, 27)]
    on = _check("gap")
    # the gap's triangles are not in the tree: the image differs from the whole mesh's
    whole = tt._sequence(_scene("cut12_between"), 1, W, H, 4, 1, split=2)[0]
    assert not np.array_equal(tt._bits(on[0]), tt._bits(whole[0]))


# ---- 3. root leaves; an odd count leaves the last pair's second slot NaN ---------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
def test_root_leaf(n):
    assert ts.shape(_scene(f"stack{n}").meshes[0]) == [(0, 3 * n)]
    _check(f"stack{n}", bounces=3, split=1)


# ---- 4. the Cornell box: every head, the tail, at the first and the last cut -----------------------------------------
@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("cut", [1, 3])
def test_cornell(cut, cache):
    """cache on: frame 0 plain, frame 1 writes, frames 2-3 read (pt_tiny_head<none>, <write>, <read>); cache off: every
    frame traces its primary segment on the primary-ray records"""
    _check("cornell", split=cut, cache=cache)


@pytest.mark.parametrize("cut", [1, 3])
def test_cornell_moved_camera(cut):
    _check("cornell", split=cut, moved=True)


# ---- 5. the kernels' own store path ------------------------------------------------------------------------------------
def _rows_sequence(s, tiny, y0, rows, split=2):
    ctx = wcpt.Context(0)
    try:
        ctx.set_option(T.OPTION_MK_TINY_TREE, tiny)
        ctx.set_option(T.OPTION_PAIR_RECORDS, 1)
        ctx.set_option(T.OPTION_MK_SPLIT, split)
        dev = wcpt.DeviceScene(ctx, s)
        ctx.create_screen(W, H)
        ctx.set_row_range(y0, rows)
        imgs = []
        for f in FRAMES:
            ctx.render(s.scene_data(W, H, max_bounce=4, samples=1, frame=f), *dev.addresses())
            ctx.sync()
            imgs.append(ctx.readback(rows))
        n = ctx.mk_tiny_tree_stats()
        dev.free()
        return imgs, n
    finally:
        ctx.close()


def test_row_range():
    """rows 11 .. 29 of the frame (no tile boundary at either end): the block's pixels are the whole frame's"""
    s = _scene("cornell")
    y0, rows = 11, 19
    on, n_on = _rows_sequence(s, 1, y0, rows)
    off, n_off = _rows_sequence(s, 0, y0, rows)
    assert n_on == len(FRAMES) and n_off == 0
    for a, b, ref in zip(on, off, _oracle_acc("cornell", W, H, 4, False)):
        assert np.array_equal(tt._bits(a), tt._bits(b))
        assert_close(a, ref[y0:y0 + rows])


@pytest.mark.parametrize("channels", [T.PAYLOAD_RGB32F, T.PAYLOAD_RGBA32F, T.PAYLOAD_DISPLAY_RGBA8])
def test_gather_payload(channels):
    """progressive frames with a payload: RGB and RGBA are the accumulation image's bits, the display payload the
    oracle's composite of it -- from the head's pixels and the tail's alike"""
    s = _scene("cornell")
    nbytes = W * H * T.PAYLOAD_PIXEL_BYTES[channels]
    payloads = {}
    for tiny in (1, 0):
        ctx = wcpt.Context(0)
        try:
            ctx.set_option(T.OPTION_MK_TINY_TREE, tiny)
            ctx.set_option(T.OPTION_PAIR_RECORDS, 1)
            ctx.set_option(T.OPTION_MK_SPLIT, 2)
            dev = wcpt.DeviceScene(ctx, s)
            buf = ctx.buffer_from(np.full(nbytes // 4, -7.0, np.float32))
            ctx.create_screen(W, H)
            ctx.set_gather_output(ctx.buffer_address(buf), nbytes, channels)
            out = []
            for f in FRAMES:
                ctx.render(s.scene_data(W, H, max_bounce=4, samples=1, frame=f), *dev.addresses())
                ctx.sync()
                img = ctx.readback(H)
                raw = ctx.buffer_download(buf, nbytes)
                if channels == T.PAYLOAD_DISPLAY_RGBA8:
                    got = np.frombuffer(raw, np.uint8).reshape(H, W, 4)
                    assert np.array_equal(got, oracle.composite(img)[1])
                else:
                    got = np.frombuffer(raw, np.float32).reshape(H, W, channels)
                    assert np.array_equal(got.view(np.uint32), img[..., :channels].view(np.uint32))
                out.append(bytes(raw))
            assert ctx.mk_tiny_tree_stats() == (len(FRAMES) if tiny else 0)
            ctx.set_gather_output(0, 0)
            ctx.buffer_free(buf)
            dev.free()
            payloads[tiny] = out
        finally:
            ctx.close()
    assert payloads[1] == payloads[0]


def test_width_of_no_whole_tile():
    """44 = 5.5 tiles of 8 pixels, 21 rows = 2.6 tiles of 8 rows: lanes outside the frame in the last column and row"""
    _check("cornell", w=44, h=21, split=2)
