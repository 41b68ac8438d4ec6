"""tests/primary_ref.py pinned to the C oracle (no GPU): for every scene the GPU tests use, at 70x44, the oracle's frame
with maxBounceCount 0 at frame 0 must equal, bit for bit, the image synthesised from the reference's records -- a hit
shows emission * emissionStrength of its material (the materials copied with distinct emissions), a miss the sky of
direction.y -- and the oracle's node_pops, triangle_tests, sphere_tests and hits for that frame must equal the
reference's sums. A reference that traverses in another order, or takes a tie the other way, fails this."""
import numpy as np
import pytest

import oracle

import primary_cases as cases
import primary_ref

W, H = cases.W, cases.H


@pytest.mark.parametrize("name", cases.SCENES)
def test_reference_is_the_oracles_segment_0(name):
    s = cases.with_distinct_emissions(cases.scene(name))
    rec, cnt = primary_ref.reference(name, cases.scene(name), W, H)
    img, ocnt = oracle.render_scene(s, W, H, max_bounce=0, samples=1, frame=0, threads=8)
    mine = primary_ref.synthesize(rec, s.materials)
    assert np.array_equal(mine.view(np.uint32), img.view(np.uint32)), \
        f"{int((mine.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())} pixels differ"
    for k in ("node_pops", "triangle_tests", "sphere_tests", "hits", "interior_visits", "draw_fetches", "segments"):
        assert cnt[k] == ocnt[k], k
    assert ocnt["pixels"] == W * H


@pytest.mark.parametrize("name", cases.SCENES)
def test_scenes_carry_their_kinds(name):
    """What each scene is there for, asserted from the reference (primary_cases.assert_kinds)."""
    cases.assert_kinds(name, primary_ref.reference(name, cases.scene(name), W, H)[0])


@pytest.mark.parametrize("name", cases.SCENES)
def test_identity_is_the_oracles_geometry(name):
    """The identity words, which the synthesised image cannot show (every triangle has material 0): the C oracle's own
    ray-triangle test of triangle `index` of draw `draw` -- that draw's vertices and permuted indices -- gives the record's
    t bit for bit, no triangle of any draw gives a smaller one (all of them tried, for meshes of up to 100 triangles),
    and the normal is that triangle's geometric normal turned towards the ray. The same for `index` of a sphere hit. A
    reference that named the wrong draw would test another mesh's triangle here."""
    s = cases.scene(name)
    rec = primary_ref.reference(name, s, W, H)[0]
    sd = s.scene_data(W, H)
    o = np.ascontiguousarray(sd["position"], np.float32)
    kind = primary_ref.kind_of(rec)
    tri_of = oracle.lib.oracle_ray_triangle
    meshes = []
    for m in s.meshes:
        pos = np.ascontiguousarray(m.positions, np.float32).reshape(-1, 3)
        meshes.append((pos, [int(v) for v in m.indices]))
    brute = sum(len(ix) for _, ix in meshes) <= 300
    for y, x in np.argwhere(kind == primary_ref.TRIANGLE):
        r = rec[y, x]
        d = np.ascontiguousarray(r["direction"], np.float32)
        pos, ix = meshes[int(r["draw"])]
        i = 3 * int(r["index"])
        p = pos.ctypes.data
        t = np.float32(tri_of(o.ctypes.data, d.ctypes.data, p + 12 * ix[i], p + 12 * ix[i + 1], p + 12 * ix[i + 2]))
        assert t.view(np.uint32) == r["t"].view(np.uint32), (x, y)
        a, b, c = (pos[ix[i + j]].astype(np.float64) for j in range(3))
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        cos = float(np.dot(d.astype(np.float64), n))
        if abs(cos) > 1e-4:                  # a grazing ray's facing may differ between binary32 and binary64
            assert bool(primary_ref.front_of(rec)[y, x]) == (cos < 0.0), (x, y)
            assert np.abs(r["normal"].astype(np.float64) - (n if cos < 0.0 else -n)).max() < 1e-5, (x, y)
        if brute:
            for pos2, ix2 in meshes:
                p2 = pos2.ctypes.data
                for j in range(0, len(ix2) - 2, 3):
                    t2 = tri_of(o.ctypes.data, d.ctypes.data, p2 + 12 * ix2[j], p2 + 12 * ix2[j + 1], p2 + 12 * ix2[j + 2])
                    assert t2 == -1.0 or t2 >= t, (x, y, j)
    for y, x in np.argwhere(kind == primary_ref.SPHERE):
        r = rec[y, x]
        sp = s.spheres[int(r["index"])]
        t = oracle.ray_sphere(o, r["direction"], sp["position"], sp["radius"])
        assert t.view(np.uint32) == r["t"].view(np.uint32) and int(r["material"]) == int(sp["material"]), (x, y)
        assert int(r["draw"]) == 0


def test_directions_are_unit_and_rowwise():
    """The direction restatement alone: one pixel at a time equals the whole frame's (no dependence on batch shape)."""
    s = cases.scene("cornell")
    sd = s.scene_data(W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    all_ = primary_ref.directions(sd, W, H, xs.reshape(-1), ys.reshape(-1)).reshape(H, W, 3)
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (33, 17)):
        one = primary_ref.directions(sd, W, H, [x], [y])[0]
        assert np.array_equal(one.view(np.uint32), all_[y, x].view(np.uint32))
    assert np.abs(np.linalg.norm(all_.astype(np.float64), axis=-1) - 1.0).max() < 1e-6
