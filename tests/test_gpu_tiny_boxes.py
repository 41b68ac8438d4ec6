"""Coincident boxes in the tiny walk (wc-path-tracer_amd/csrc/pt_tiny.h tiny_walk): a child whose six bound words are the
root's bits takes the root's slab distances instead of a slab test of its own, and the right child likewise the left one's.
The comparison is bitwise and wave-uniform; the decisions that read the distances (root_survives, child_pair) are the
traversal loop's.

Every case is a 76x40 sequence of 4 progressive frames with a forced cut, so that the walk-only kernels run
(wcpt_mk_tiny_tree_stats counts every render), compared bit for bit with the same sequence under WCPT_OPTION_MK_TINY_TREE 0
-- the general kernels, which test every box -- and with the CPU oracle, which walks the same nodes:

  cornell          both children's boxes are the root's (the room's two leaves span the whole room);
  cubes            the two cubes of test_gpu_tiny_kernels.py: neither box is the root's;
  left_is_root     the cubes with the left child's bounds overwritten by the root's;
  right_is_root    the same for the right child;
  common           both children widened to one box that is not the root's (the root's is wider still);
  minus_zero       the left child's bounds are the root's except -0 for +0 in one minimum: not the same bits, so it is
                   tested on its own; the camera lies in that plane, where the sign of the zero reaches the slab products;
  cornell, moved camera (every frame traces its primary segment on the primary-ray records), and a row range."""
import numpy as np
import pytest

import wcpt
from wcpt import scene as wscene
from wcpt._lib import NODE_DTYPE

import tiny_scenes as ts
import test_gpu_tiny_tree as tt
import test_gpu_tiny_kernels as tk
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

T = wcpt._lib
W, H = tk.W, tk.H
FRAMES = tk.FRAMES


def _box_words(node):
    return np.concatenate([np.asarray(node["min"], np.float32), np.asarray(node["max"], np.float32)]).view(np.uint32)


def _same_box(a, b):
    return np.array_equal(_box_words(a), _box_words(b))


def _cubes_bvh(case):
    """the two cubes, 12 / 12, with the bounds rewritten for the case; every box still holds its triangles"""
    mesh = ts.two_boxes_mesh()
    if case == "minus_zero":   # lifted so that the root's min.y is +0
        mesh = wscene.HostMesh(mesh.positions + np.array([0.0, 0.3, 0.0], np.float32), mesh.indices)
    bvh = ts.two_leaf_bvh(mesh, 12)
    root, left, right = bvh.nodes[0], bvh.nodes[1], bvh.nodes[2]
    if case == "left_is_root":
        left["min"], left["max"] = root["min"], root["max"]
    elif case == "right_is_root":
        right["min"], right["max"] = root["min"], root["max"]
    elif case == "common":
        for n in (left, right):
            n["min"], n["max"] = root["min"], root["max"]
        root["min"] = root["min"] - np.float32(0.5)
        root["max"] = root["max"] + np.float32(0.5)
    elif case == "minus_zero":
        assert root["min"][1] == 0.0 and not np.signbit(root["min"][1])
        left["min"], left["max"] = root["min"], root["max"]
        left["min"][1] = np.float32(-0.0)
    elif case != "cubes":
        raise KeyError(case)
    return bvh


CAMERAS = {"minus_zero": dict(position=(0.0, 0.0, 1.5), yaw=-90.0, pitch=0.0, fov=90.0)}


def _install(case):
    name = "boxes_" + case
    if name not in tk._scenes:
        tk._scenes[name] = tt._with_meshes([_cubes_bvh(case)], wscene.make_camera(**CAMERAS.get(case, tk.BETWEEN)))
    return name


def _nodes(case):
    return tk._scenes[_install(case)].meshes[0].nodes


def test_cornell_boxes_are_the_roots():
    n = tk._scene("cornell").meshes[0].nodes
    assert len(n) == 3 and _same_box(n[1], n[0]) and _same_box(n[2], n[0])
    tk._check("cornell", split=2)


def test_cubes_boxes_are_their_own():
    n = _nodes("cubes")
    assert not _same_box(n[1], n[0]) and not _same_box(n[2], n[0]) and not _same_box(n[1], n[2])
    tk._check(_install("cubes"))


def test_left_child_with_the_roots_bounds():
    n = _nodes("left_is_root")
    assert _same_box(n[1], n[0]) and not _same_box(n[2], n[0]) and not _same_box(n[2], n[1])
    tk._check(_install("left_is_root"))


def test_right_child_with_the_roots_bounds():
    n = _nodes("right_is_root")
    assert _same_box(n[2], n[0]) and not _same_box(n[1], n[0])
    tk._check(_install("right_is_root"))


def test_children_share_a_box_that_is_not_the_roots():
    n = _nodes("common")
    assert _same_box(n[1], n[2]) and not _same_box(n[1], n[0])
    tk._check(_install("common"))


def test_minus_zero_is_another_box():
    n = _nodes("minus_zero")
    assert n[1]["min"][1] == n[0]["min"][1] and not _same_box(n[1], n[0])          # equal as floats, not as bits
    assert np.flatnonzero(_box_words(n[1]) != _box_words(n[0])).tolist() == [1]
    tk._check(_install("minus_zero"))


def test_cornell_moved_camera():
    """the primary-record form of the pair test on every frame"""
    tk._check("cornell", split=2, moved=True)


def _rows_sequence(s, tiny, y0, rows, moved):
    ctx = wcpt.Context(0)
    try:
        ctx.set_option(T.OPTION_MK_TINY_TREE, tiny)
        ctx.set_option(T.OPTION_PAIR_RECORDS, 1)
        ctx.set_option(T.OPTION_MK_SPLIT, 2)
        dev = wcpt.DeviceScene(ctx, s)
        ctx.create_screen(W, H)
        ctx.set_row_range(y0, rows)
        imgs = []
        for f, cam in zip(FRAMES, tt._cameras(s, moved)):
            ctx.render(s.scene_data(W, H, max_bounce=4, samples=1, frame=f, camera=cam), *dev.addresses())
            ctx.sync()
            imgs.append(ctx.readback(rows))
        n = ctx.mk_tiny_tree_stats()
        dev.free()
        return imgs, n
    finally:
        ctx.close()


def test_cornell_moved_camera_row_range():
    """rows 11 .. 29, no tile boundary at either end, under the moving camera"""
    s = tk._scene("cornell")
    y0, rows = 11, 19
    on, n_on = _rows_sequence(s, 1, y0, rows, True)
    off, n_off = _rows_sequence(s, 0, y0, rows, True)
    assert n_on == len(FRAMES) and n_off == 0
    for a, b, ref in zip(on, off, tk._oracle_acc("cornell", W, H, 4, True)):
        assert np.array_equal(tt._bits(a), tt._bits(b))
        assert_close(a, ref[y0:y0 + rows])
