"""Primary-hit pass A/B on one GPU: what wcpt_trace_primary costs against the existing path that traces the same rays.
One process, interleaved rounds, on c2 (Cornell) and c3 (atrium) at 1920x1080; per round, N calls each of
  (a) wcpt_trace_primary into a context buffer (48 B per pixel) -- the code under test;
  (b) wcpt_render with maxBounceCount 0, renderedFramesCount 0 and WCPT_OPTION_PRIMARY_CACHE 0 on the config's own kernel
      (c2 megakernel, c3 wavefront): segment 0 of every pixel and a 16 B store per pixel -- the yardstick;
  (b') for c3 also the same render on the megakernel, whose traversal the pass runs.
Each is timed with wcpt_profile_begin / wcpt_profile_end in region mode (one event before the first launch, one after the
last: ms per call = total / N). One untimed warm-up round first. Then one wcpt_pick of the centre pixel per round, host
clock around the call (it is launch- and copy-bound). Median and range over the rounds; no threshold.

    python tools/primary_ab.py [--rounds 7] [--calls 20] [--configs c2,c3] [--out LOG]

The log is profiles/primary_hits_ab.log.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "wc-path-tracer_amd"), ROOT]

import wcpt  # noqa: E402
from wcpt import scene as wscene  # noqa: E402

T = wcpt._lib
CONFIGS = {"c2": ("cornell", wcpt.KERNEL_MEGAKERNEL), "c3": ("atrium", wcpt.KERNEL_WAVEFRONT)}
KERNEL_NAMES = {wcpt.KERNEL_MEGAKERNEL: "megakernel", wcpt.KERNEL_WAVEFRONT: "wavefront"}
W, H = 1920, 1080


def fmt(v):
    return f"median {statistics.median(v):8.4f}  min {min(v):8.4f}  max {max(v):8.4f}"


def region(ctx, calls, fn):
    """ms per call of `calls` calls of fn, by the context's region timing"""
    ctx.profile_begin()
    for _ in range(calls):
        fn()
    ms, _ = ctx.profile_end()
    return ms / calls


def ab(name, rounds, calls):
    scene_name, kernel = CONFIGS[name]
    s = wscene.generate(scene_name)
    sd = s.scene_data(W, H, max_bounce=0, samples=1, frame=0)
    kernels = [kernel] + ([wcpt.KERNEL_MEGAKERNEL] if kernel != wcpt.KERNEL_MEGAKERNEL else [])
    ms = {"a": [], "pick": []}
    ms.update({k: [] for k in kernels})
    with wcpt.Context(0) as ctx:
        ctx.set_option(T.OPTION_PRIMARY_CACHE, 0)
        ctx.set_option(T.OPTION_PROFILE_REGION, 1)
        dev = wcpt.DeviceScene(ctx, s)
        ctx.create_screen(W, H)
        nbytes = W * H * T.PRIMARY_HIT_DTYPE.itemsize
        buf = ctx.buffer_alloc(nbytes)
        dst = ctx.buffer_address(buf)
        for r in range(-1, rounds):
            a = region(ctx, calls, lambda: ctx.trace_primary(sd, dev.spheres, dev.draws, dst=dst, nbytes=nbytes))
            b = {}
            for k in kernels:
                ctx.set_kernel(k)
                ctx.render(sd, *dev.addresses())   # the kernel's own preparation and buffers outside the timed region
                ctx.sync()
                b[k] = region(ctx, calls, lambda: ctx.render(sd, *dev.addresses()))
            ctx.sync()
            t0 = time.perf_counter()
            ctx.pick(sd, dev.spheres, dev.draws, W // 2, H // 2)
            p = (time.perf_counter() - t0) * 1e3
            if r >= 0:
                ms["a"].append(a)
                ms["pick"].append(p)
                for k in kernels:
                    ms[k].append(b[k])
        rec = np.frombuffer(ctx.buffer_download(buf, nbytes), T.PRIMARY_HIT_DTYPE)
        kinds = np.bincount(rec["kind"] & T.HIT_KIND_MASK, minlength=3)
        ctx.buffer_free(buf)
        dev.free()
    tris = sum(m.indices.size // 3 for m in s.meshes)
    lines = [f"{name}: {scene_name} ({tris} triangles, {len(s.spheres)} spheres), {W}x{H}; records: {kinds[0]} misses, "
             f"{kinds[1]} sphere hits, {kinds[2]} triangle hits",
             f"{'  (a) wcpt_trace_primary, 48 B/px':<54}{fmt(ms['a'])}  ms per call"]
    for i, k in enumerate(kernels):
        label = f"  (b{chr(39) * i}) wcpt_render, 0 bounces, {KERNEL_NAMES[k]}, 16 B/px"
        lines.append(f"{label:<54}{fmt(ms[k])}  ms per call")
        spread = max(ms[k]) - min(ms[k])
        diff = statistics.median(ms["a"]) - statistics.median(ms[k])
        lines.append(f"       (a) - (b{chr(39) * i}) by medians {diff:+.4f} ms; (b{chr(39) * i})'s round-to-round spread {spread:.4f} ms")
    lines.append(f"{f'  wcpt_pick of ({W // 2}, {H // 2}), host clock':<54}{fmt(ms['pick'])}  ms per call")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primary_hits_ab.log"))
    a = ap.parse_args()
    lines = [f"build_id {wcpt.lib.wcpt_build_id().decode()}  rounds {a.rounds} (interleaved a, b), {a.calls} calls per round "
             "(region timing: wcpt_profile_begin / wcpt_profile_end)"]
    print(lines[0], flush=True)
    for name in a.configs.split(","):
        got = ab(name, a.rounds, a.calls)
        print("\n".join(got), flush=True)
        lines += got
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
