"""BVH build A/B on one GPU: for the mushroom and the atrium (config c3's mesh), interleaved rounds of
  (a) host: wcpt_bvh_build (--builder sah: wcpt_bvh_build_sah) on the host, then wcpt_buffer_upload of the permuted
      indices and the nodes;
  (b) device: wcpt_bvh_build_device (wcpt_bvh_build_sah_device) on positions and unpermuted indices that are already in
      device buffers (the indices are re-uploaded before every round, outside the timed region).
Both end with everything on the device and the stream idle (the uploads block; the device build is synchronous), timed
by the host clock. Every round the device's bytes -- nodes [0, used), the node count, the index buffer -- are compared
with the host builder's. One untimed warm-up round of each first (code objects, the build's scratch allocation).

    python tools/bvh_build_ab.py [--builder midpoint|sah] [--rounds 7] [--meshes mushroom,atrium] [--out LOG]

The log is profiles/bvh_device_build.log, or profiles/bvh_sah_device_build.log with --builder sah.
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
from wcpt._lib import NODE_DTYPE, SceneC, check, lib, ptr  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--meshes", default="mushroom,atrium")
    ap.add_argument("--builder", choices=("midpoint", "sah"), default="midpoint")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sah = a.builder == "sah"
    out = a.out or os.path.join(ROOT, "profiles", "bvh_sah_device_build.log" if sah else "bvh_device_build.log")
    host_fn = lib.wcpt_bvh_build_sah if sah else lib.wcpt_bvh_build
    host_name = "wcpt_bvh_build_sah" if sah else "wcpt_bvh_build"
    dev_name = "wcpt_bvh_build_sah_device" if sah else "wcpt_bvh_build_device"
    lines = [f"build_id {wcpt.lib.wcpt_build_id().decode()}  builder {a.builder}  rounds {a.rounds} "
             "(interleaved host, device; ms by the host clock)"]
    print(lines[0], flush=True)
    with wcpt.Context(0) as ctx:
        for name in a.meshes.split(","):
            mesh = load(name)
            pos = np.ascontiguousarray(mesh.positions, np.float32)
            idx0 = np.ascontiguousarray(mesh.indices, np.uint32)
            max_nodes = max(1, 2 * (idx0.size // 3))
            vb = ctx.buffer_from(pos)
            ib_h, nb_h = ctx.buffer_alloc(idx0.nbytes), ctx.buffer_alloc(max_nodes * NODE_DTYPE.itemsize)
            ib_d, nb_d = ctx.buffer_alloc(idx0.nbytes), ctx.buffer_alloc(max_nodes * NODE_DTYPE.itemsize)
            host_ms, dev_ms, build_ms = [], [], []
            used_h = 0
            for r in range(-1, a.rounds):
                idx = idx0.copy()
                nodes = np.zeros(max_nodes, dtype=NODE_DTYPE)
                used = C.c_uint32()
                t0 = time.perf_counter()
                check(host_fn(ptr(pos), pos.shape[0], ptr(idx), idx.size, ptr(nodes), max_nodes, C.byref(used)))
                t1 = time.perf_counter()
                ctx.buffer_upload(ib_h, idx)
                ctx.buffer_upload(nb_h, nodes[: used.value])
                t2 = time.perf_counter()
                used_h = used.value
                ctx.buffer_upload(ib_d, idx0)
                ctx.sync()
                t3 = time.perf_counter()
                used_d = ctx.bvh_build_device(vb, pos.shape[0], ib_d, idx0.size, nb_d, builder=a.builder)
                t4 = time.perf_counter()
                same = (used_d == used_h and ctx.buffer_download(ib_d, idx0.nbytes) == idx.tobytes() and
                        ctx.buffer_download(nb_d, used_d * NODE_DTYPE.itemsize) == nodes[:used_h].tobytes())
                if not same:
                    raise SystemExit(f"{name} round {r}: the device build differs from {host_name}")
                if r >= 0:
                    host_ms.append((t2 - t0) * 1e3)
                    build_ms.append((t1 - t0) * 1e3)
                    dev_ms.append((t4 - t3) * 1e3)
            for b in (vb, ib_h, nb_h, ib_d, nb_d):
                ctx.buffer_free(b)

            def fmt(v):
                return f"median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}"

            lines += [f"{name}: {idx0.size // 3} triangles, {used_h} nodes; bytes equal in every round",
                      f"  (a) host build + 2 uploads   {fmt(host_ms)}   (the build alone: {fmt(build_ms)})",
                      f"  (b) {dev_name:<25}{' ' if sah else ''}{fmt(dev_ms)}",
                      f"  (a) / (b) by medians         {statistics.median(host_ms) / statistics.median(dev_ms):9.2f}"]
            print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
