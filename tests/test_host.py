"""Host-side inputs of the hot path (no GPU): OBJ loader and BVH builder against their oracles, camera, scenes.

- BVH: the product builder (wc-path-tracer_amd/host, iterative) against the oracle's restatement of the
  reference recursion (oracle/pt_oracle.c, PathTracingRenderer.jai:147-217): identical node arrays and
  identical permuted index buffers, byte for byte.
- OBJ: the product loader against the pure-Python restatement (oracle/obj_oracle.py, ModelLoader.jai:60-141)
  on an edge-case fixture, on generated meshes and on the reference's own asset OBJs (fixtures under
  tests/golden/models). SURVEY.md Appendix B's mesh statistics pin the BVH sizes of those assets.
"""
import os

import numpy as np
import pytest

import obj_oracle
import oracle
import wcpt
from wcpt import scene as wscene

HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODELS = os.path.join(HERE, "golden", "models")


def _bvh_equal(mesh):
    prod = wscene.bvh_build(mesh)
    nodes, idx = oracle.bvh_build(mesh.positions, mesh.indices, wcpt.NODE_DTYPE)
    assert prod.nodes.tobytes() == nodes.tobytes()
    assert np.array_equal(prod.indices, idx)
    return prod


def _leaf_stats(b):
    cnt = b.nodes["triangleCount"]
    leaves = cnt[cnt > 0]
    return len(b.nodes), int(leaves.size), int(leaves.max() // 3)


@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_bvh_matches_oracle_on_scenes(name):
    s = wscene.generate(name)
    m = s.meshes[0]
    b = _bvh_equal(wscene.HostMesh(m.positions, m.indices))
    assert b.depth() <= 33


def test_bvh_matches_oracle_random_soups():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 50, 1000, 5000):
        centers = rng.uniform(-10, 10, (n, 3))
        pos = (centers[:, None, :] + rng.normal(0, 0.3, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
        idx = np.arange(3 * n, dtype=np.uint32)
        rng.shuffle(idx.reshape(-1, 3))
        _bvh_equal(wscene.HostMesh(pos, idx))


def test_bvh_degenerate_inputs():
    # every triangle identical: no split can separate them -> one leaf
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    idx = np.tile(np.arange(3, dtype=np.uint32), 40)
    b = _bvh_equal(wscene.HostMesh(pos, idx))
    assert len(b.nodes) == 1 and b.nodes[0]["triangleCount"] == 120
    # the first triangle ends right with first == 0 (the reference's u32 `j -= 3` would wrap, :178,190)
    pos = np.array([[5, 0, 0], [6, 0, 0], [5, 1, 0], [0, 0, 0], [0.1, 0, 0], [0, 0.1, 0],
                    [0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], np.float32)
    idx = np.arange(9, dtype=np.uint32)
    _bvh_equal(wscene.HostMesh(pos, np.tile(idx, 3)))
    # at most 2 triangles (6 indices) never split
    b = _bvh_equal(wscene.HostMesh(pos[:6], np.arange(6, dtype=np.uint32)))
    assert len(b.nodes) == 1


def test_bvh_rejects_bad_input():
    with pytest.raises(wcpt.WcptError):
        wscene.bvh_build(wscene.HostMesh(np.zeros((3, 3), np.float32), np.zeros(0, np.uint32)))
    with pytest.raises(wcpt.WcptError):
        wscene.bvh_build(wscene.HostMesh(np.zeros((3, 3), np.float32), np.array([0, 1, 5], np.uint32)))


EDGE_OBJ = """# edge cases for parse_obj_file (ModelLoader.jai:60-141)
o thing
v 0 0 0
v 1 0 0\r
v 1 1 0
v 0 1 0
  v 0.5 0.5 1.25e-1
vt 0 0
vt 1 0
vn 0 0 1

f 1 2 3
f 1/1 2/2 3/1 4/2
f 1//1 2//1 5//1
f 1/1/1 3/2/1 4/1/1 5/2/1 2/1/1
f 2 3 99
f -1 2 3
f 4  5 1
v 2 2 2
f 6 1 2
usemtl nothing
f 1 2
"""


def test_obj_edge_cases_match_oracle():
    m = wscene.obj_parse(EDGE_OBJ)
    pos, idx = obj_oracle.parse_obj(EDGE_OBJ)
    assert np.array_equal(m.positions, pos)
    assert np.array_equal(m.indices, idx)
    assert m.indices.size % 3 == 0


def test_obj_roundtrip_generated():
    s = wscene.generate("cornell", via_obj=False)
    text = wscene.mesh_to_obj(wscene.HostMesh(s.meshes[0].positions, s.meshes[0].indices))
    m = wscene.obj_parse(text)
    pos, idx = obj_oracle.parse_obj(text.decode())
    assert np.array_equal(m.positions, pos) and np.array_equal(m.indices, idx)
    # same triangles (OBJ de-dup keeps first-seen order)
    tri_a = s.meshes[0].positions[s.meshes[0].indices.reshape(-1, 3)]
    tri_b = m.positions[m.indices.reshape(-1, 3)]
    assert np.array_equal(np.sort(tri_a.reshape(-1, 9), axis=0), np.sort(tri_b.reshape(-1, 9), axis=0))


@pytest.mark.parametrize("fname,verts,indices,nodes,leaves,max_leaf", [
    # SURVEY.md Appendix B (a float64 restatement). The reference builds in f32 (Jai `float`), as we do:
    # mushroom and suzanita agree exactly; campfire has one extra split in f32 (161 nodes / 81 leaves
    # against Appendix B's float64 159 / 80), a centroid that lands on the other side of a split plane.
    ("mushroom.obj", 780, 1098, 67, 34, 43),
    ("campfire.obj", 1064, 1548, 161, 81, 108),
    ("suzanita.obj", 1966, 2904, 827, 414, 26),
])
def test_reference_assets(fname, verts, indices, nodes, leaves, max_leaf):
    path = os.path.join(REF_MODELS, fname)
    m = wscene.obj_load(path)
    pos, idx = obj_oracle.parse_obj(open(path).read())
    assert np.array_equal(m.positions, pos) and np.array_equal(m.indices, idx)
    assert (m.positions.shape[0], m.indices.size) == (verts, indices)
    b = _bvh_equal(m)
    assert _leaf_stats(b) == (nodes, leaves, max_leaf)


def test_obj_load_missing_file():
    with pytest.raises(wcpt.WcptError) as e:
        wscene.obj_load("/nonexistent/model.obj")
    assert e.value.code == -1004


def test_camera_matrices():
    cam = wscene.update_camera(wscene.make_camera((1.0, 2.0, 3.0), yaw=-90.0, pitch=0.0, fov=90.0), 16 / 9)
    d = np.ctypeslib.as_array(cam.direction)
    assert np.allclose(d, [0, 0, -1], atol=1e-6)
    V = np.ctypeslib.as_array(cam.view).reshape(4, 4).T          # column-major -> row-major
    iV = np.ctypeslib.as_array(cam.inverseView).reshape(4, 4).T
    P = np.ctypeslib.as_array(cam.projection).reshape(4, 4).T
    iP = np.ctypeslib.as_array(cam.inverseProjection).reshape(4, 4).T
    assert np.allclose(V @ iV, np.eye(4), atol=1e-5) and np.allclose(P @ iP, np.eye(4), atol=1e-5)
    assert np.allclose(iV[:3, 3], [1, 2, 3])                      # camera origin
    # the centre pixel looks along the view direction
    t = iP @ np.array([0, 0, 1, 1.0])
    w = iV @ np.concatenate([t[:3] / t[3] / np.linalg.norm(t[:3] / t[3]), [0]])
    assert np.allclose(w[:3] / np.linalg.norm(w[:3]), d, atol=1e-5)


def test_scenes_deterministic():
    a = wscene.generate("atrium")
    b = wscene.generate("atrium")
    assert a.meshes[0].positions.tobytes() == b.meshes[0].positions.tobytes()
    assert a.meshes[0].nodes.tobytes() == b.meshes[0].nodes.tobytes()
    assert 250_000 <= a.meshes[0].triangle_count if hasattr(a.meshes[0], "triangle_count") else True
    assert a.meshes[0].indices.size // 3 >= 250_000          # "Sponza-scale", SURVEY.md §8(d) C3
    c = wscene.generate("cornell")
    assert c.meshes[0].indices.size // 3 == 34               # Cornell-class, ~30 triangles
    d = wscene.generate("default")
    assert len(d.spheres) == 4 and len(d.materials) == 4 and not d.meshes
    # reference Init quirks: glass is METAL, Left's emission strength is 0
    assert d.materials["type"].tolist() == [0, 0, 0, 0]
    assert d.materials["emissionStrength"][2] == 0.0
    assert d.materials["ior"][0] == np.float32(1.5) and d.materials["absorptionStrength"].tolist() == [1, 1, 1, 1]


# ---- optional binned-SAH builder ----------------------------------------------------
def _check_bvh(b, ntri):
    nodes = b.nodes
    seen = np.zeros(ntri, np.int32)
    depth_max = 0
    stack = [(0, 1)]
    while stack:
        i, d = stack.pop()
        depth_max = max(depth_max, d)
        n = nodes[i]
        lo, hi = n["min"], n["max"]
        if n["triangleCount"] == 0:
            left = int(n["leftNodeOrTriangleIndex"])
            assert left % 2 == 1 and left + 1 < nodes.size          # children are a consecutive (odd, even) pair
            for c in (left, left + 1):
                assert np.all(nodes[c]["min"] >= lo) and np.all(nodes[c]["max"] <= hi)
                stack.append((c, d + 1))
        else:
            first, cnt = int(n["leftNodeOrTriangleIndex"]), int(n["triangleCount"])
            assert first % 3 == 0 and cnt % 3 == 0
            v = b.positions[b.indices[first:first + cnt]]
            assert np.all(v >= lo) and np.all(v <= hi)
            assert np.array_equal(v.min(axis=0), lo) and np.array_equal(v.max(axis=0), hi)
            seen[first // 3:(first + cnt) // 3] += 1
    assert np.all(seen == 1)                                         # every triangle in exactly one leaf
    return depth_max


@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_sah_bvh_valid_and_same_triangles(name):
    s = wscene.generate(name)
    m = s.meshes[0]
    mesh = wscene.HostMesh(m.positions, m.indices)
    sah = wscene.bvh_build(mesh, "sah")
    ntri = m.indices.size // 3
    depth = _check_bvh(sah, ntri)
    assert depth <= 41
    # same multiset of triangles as the input
    assert np.array_equal(np.sort(m.indices.reshape(-1, 3).view("u4,u4,u4"), axis=0),
                          np.sort(sah.indices.reshape(-1, 3).view("u4,u4,u4"), axis=0))
    if name == "atrium":
        mid = s.meshes[0]
        leaves_sah = int((sah.nodes["triangleCount"] > 0).sum())
        assert sah.nodes["triangleCount"].max() <= 3 * 8 or leaves_sah > 0
        assert mid.nodes["triangleCount"].max() >= sah.nodes["triangleCount"].max()
