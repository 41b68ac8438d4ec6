"""BVH refit A/B on one GPU: what a mesh whose vertices move costs per frame, for the mushroom and the atrium (config c3's
mesh), on the midpoint and on the SAH tree. One context, interleaved rounds; per round, over new positions (a smooth
bend that alternates between two phases, so every refit has work to do):
  (v) the vertex upload on its own (wcpt_buffer_upload of the positions) -- every variant below needs it first;
  (a) refit on the device: wcpt_bvh_refit_device on the tree already in device buffers;
  (b) rebuild on the device: wcpt_bvh_build_device / wcpt_bvh_build_sah_device (the unpermuted indices are re-uploaded
      before it, outside the timed region) -- the yardstick;
  (c) refit on the host: wcpt_bvh_refit on the host's copy of the tree, then wcpt_buffer_upload of the nodes.
Each ends with everything on the device and the stream idle (the uploads block; the refit and the builds are
synchronous), timed by the host clock. Every round the device refit's node bytes are compared with the host refit's. One
untimed warm-up round first (code objects, the scratch allocation).

With --frames N (default 20; 0 skips it) the atrium is then rendered as config c3 does (1920x1080, 1 spp, 4 bounces,
wavefront kernel) over the deformed positions, once with the refitted tree and once with a tree rebuilt for those
positions: N frames each after 3 warm-up frames, ms per frame by the host clock around a synchronise. Information for
deciding when to rebuild; no threshold.

    python tools/bvh_refit_ab.py [--rounds 7] [--meshes mushroom,atrium] [--frames 20] [--out LOG]

The log is profiles/bvh_refit.log.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "wc-path-tracer_amd"), ROOT]

import wcpt  # noqa: E402
from wcpt import scene as wscene  # noqa: E402
from wcpt._lib import DRAW_COMMAND_DTYPE, NODE_DTYPE, SceneC, check, lib, ptr  # noqa: E402

NODE = NODE_DTYPE.itemsize


def load(name):
    if name == "mushroom":
        return wscene.obj_load(wscene.MUSHROOM_OBJ)
    s = SceneC()
    check(lib.wcpt_scene_generate(name.encode(), 0, C.byref(s)))
    try:
        mesh = wscene._mesh_from_c(s.mesh)
    finally:
        lib.wcpt_scene_free(C.byref(s))
    return wscene.obj_parse(wscene.mesh_to_obj(mesh))  # through the OBJ loader, as scene.generate does


def deformed(pos, seed):
    """a smooth bend, as an animation would make: every vertex displaced by up to 2 % of the mesh's largest extent, along
    each axis by a sine of the next axis' coordinate (three waves across the mesh; `seed` shifts the phase)"""
    lo, extent = pos.min(axis=0), np.float32((pos.max(axis=0) - pos.min(axis=0)).max())
    phase = 2.0 * np.pi * (3.0 * (pos - lo) / extent + 0.37 * seed)
    return (pos + np.float32(0.02) * extent * np.sin(np.roll(phase, 1, axis=1)).astype(np.float32)).astype(np.float32)


def fmt(v):
    return f"median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}"


def ab(ctx, name, mesh, builder, rounds):
    pos0 = np.ascontiguousarray(mesh.positions, np.float32)
    idx0 = np.ascontiguousarray(mesh.indices, np.uint32)
    sets = [deformed(pos0, 1), deformed(pos0, 2)]
    tree = wscene.bvh_build(mesh, builder)  # the host's copy of the tree that is refitted
    used = len(tree.nodes)
    max_nodes = max(1, 2 * (idx0.size // 3))
    vb = ctx.buffer_from(pos0)
    ib_t, nb_t = ctx.buffer_from(tree.indices), ctx.buffer_from(tree.nodes)
    nb_h = ctx.buffer_alloc(used * NODE)
    ib_r, nb_r = ctx.buffer_alloc(idx0.nbytes), ctx.buffer_alloc(max_nodes * NODE)
    ms = {"v": [], "a": [], "b": [], "c": [], "c_refit": []}
    try:
        for r in range(-1, rounds):
            pos = sets[r % 2]
            t0 = time.perf_counter()
            ctx.buffer_upload(vb, pos)
            t1 = time.perf_counter()
            ctx.bvh_refit_device(vb, pos.shape[0], ib_t, idx0.size, nb_t, used)
            t2 = time.perf_counter()
            ctx.buffer_upload(ib_r, idx0)
            ctx.sync()
            t3 = time.perf_counter()
            ctx.bvh_build_device(vb, pos.shape[0], ib_r, idx0.size, nb_r, builder=builder)
            t4 = time.perf_counter()
            nodes = tree.nodes.copy()
            t5 = time.perf_counter()
            check(lib.wcpt_bvh_refit(ptr(pos), pos.shape[0], ptr(tree.indices), tree.indices.size, ptr(nodes), used))
            t6 = time.perf_counter()
            ctx.buffer_upload(nb_h, nodes)
            t7 = time.perf_counter()
            if ctx.buffer_download(nb_t, used * NODE) != nodes.tobytes():
                raise SystemExit(f"{name} {builder} round {r}: the device refit differs from wcpt_bvh_refit")
            if r >= 0:
                for key, dt in (("v", t1 - t0), ("a", t2 - t1), ("b", t4 - t3), ("c", t7 - t5), ("c_refit", t6 - t5)):
                    ms[key].append(dt * 1e3)
    finally:
        for b in (vb, ib_t, nb_t, nb_h, ib_r, nb_r):
            ctx.buffer_free(b)
    build_name = "wcpt_bvh_build_device" if builder == "midpoint" else "wcpt_bvh_build_sah_device"
    below = max(ms["a"]) < min(ms["b"])
    return [f"{name}, {builder} tree: {idx0.size // 3} triangles, {used} nodes, {tree.depth()} levels; device refit bytes equal wcpt_bvh_refit's in every round",
            f"  (v) vertex upload alone            {fmt(ms['v'])}",
            f"  (a) wcpt_bvh_refit_device          {fmt(ms['a'])}",
            f"  (b) {build_name:<31}{fmt(ms['b'])}",
            f"  (c) wcpt_bvh_refit + node upload   {fmt(ms['c'])}   (the refit alone: {fmt(ms['c_refit'])})",
            f"  (b) / (a) by medians {statistics.median(ms['b']) / statistics.median(ms['a']):7.2f};  the refit's range lies "
            f"{'wholly below' if below else 'NOT wholly below'} the rebuild's"]


def c3_frames(ctx, mesh, builder, frames):
    """ms per c3 frame over deformed positions: the built tree refitted, against a tree built for those positions"""
    s = wscene.generate("atrium")
    W, H, bounces = 1920, 1080, 4
    pos = deformed(np.ascontiguousarray(mesh.positions, np.float32), 1)
    tree = wscene.bvh_build(mesh, builder)
    refit = wscene.bvh_refit(tree, pos)
    rebuilt = wscene.bvh_build(wscene.HostMesh(pos, mesh.indices), builder)
    ctx.set_kernel(wcpt.KERNEL_WAVEFRONT)
    ctx.create_screen(W, H)
    mat, sph = ctx.buffer_from(s.materials), ctx.buffer_from(s.spheres)
    out = {}
    for label, bvh in (("original", tree), ("refit", refit), ("rebuilt", rebuilt)):
        vb, ib, nb = ctx.buffer_from(bvh.positions), ctx.buffer_from(bvh.indices), ctx.buffer_from(bvh.nodes)
        a = ctx.buffer_address
        draws = ctx.buffer_from(np.array([(a(vb), a(ib), a(nb), bvh.indices.size, 0)], DRAW_COMMAND_DTYPE))
        t = []
        for f in range(-3, frames):
            sd = s.scene_data(W, H, max_bounce=bounces, frame=max(f, 0))
            t0 = time.perf_counter()
            ctx.render(sd, a(mat), a(sph), a(draws))
            ctx.sync()
            if f >= 0:
                t.append((time.perf_counter() - t0) * 1e3)
        out[label] = t
        for b in (vb, ib, nb, draws):
            ctx.buffer_free(b)
    for b in (mat, sph):
        ctx.buffer_free(b)
    return [f"c3 frame (atrium 1920x1080, 1 spp, 4 bounces, wavefront), {builder} tree, vertices bent by up to 2 % of the extent, {frames} frames:",
            f"  (before the bend, the built tree   {fmt(out['original'])})",
            f"  refitted tree                      {fmt(out['refit'])}",
            f"  tree rebuilt for the positions     {fmt(out['rebuilt'])}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--meshes", default="mushroom,atrium")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bvh_refit.log"))
    a = ap.parse_args()
    lines = [f"build_id {wcpt.lib.wcpt_build_id().decode()}  rounds {a.rounds} (interleaved v, a, b, c; ms by the host clock)"]
    print(lines[0], flush=True)
    with wcpt.Context(0) as ctx:
        meshes = {name: load(name) for name in a.meshes.split(",")}
        for name, mesh in meshes.items():
            for builder in ("midpoint", "sah"):
                got = ab(ctx, name, mesh, builder, a.rounds)
                print("\n".join(got), flush=True)
                lines += got
        if a.frames > 0 and "atrium" in meshes:
            for builder in ("midpoint", "sah"):
                got = c3_frames(ctx, meshes["atrium"], builder, a.frames)
                print("\n".join(got), flush=True)
                lines += got
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
