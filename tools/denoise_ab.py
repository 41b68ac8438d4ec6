"""Display-step A/B on one GPU: what wcpt_composite_denoise costs beside the two existing display calls of the same
build. One process, interleaved rounds, on c2 (Cornell) and c3 (atrium) at 1920x1080, RGBA8; the image is a rendered
one-sample frame (4 bounces, frame 0) and the guide the frame's wcpt_trace_primary records. Per round, N calls each of
  (a) wcpt_composite;
  (b) wcpt_composite_bloom with the defaults;
  (d1) (d3) (d5) wcpt_composite_denoise at 1, 3 and 5 iterations, the other parameters the defaults;
  (g) wcpt_trace_primary, the guide pass, paid once per camera move.
The context runs on a torch stream of its own; each figure is the device time between two events on that stream around
N back-to-back calls, divided by N (the display calls are outside the context's own region timing, which brackets
renders). One untimed warm-up round first. Median and range over the rounds; no threshold.

    python tools/denoise_ab.py [--rounds 7] [--calls 20] [--configs c2,c3] [--out LOG]
    python tools/denoise_ab.py --once c2        one call of each on c2 and nothing else: the program of a kernel trace

The log is profiles/denoise_ab.log; the per-launch split below it is from one `rocprofv3 --kernel-trace --stats` run of
`--once`, a run of its own.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "wc-path-tracer_amd"), ROOT]

import torch  # noqa: E402

import wcpt  # noqa: E402
from wcpt import scene as wscene  # noqa: E402

T = wcpt._lib
CONFIGS = {"c2": ("cornell", wcpt.KERNEL_MEGAKERNEL), "c3": ("atrium", wcpt.KERNEL_WAVEFRONT)}
W, H = 1920, 1080
ITERATIONS = (1, 3, 5)


def fmt(v):
    return f"median {statistics.median(v):8.1f}  min {min(v):8.1f}  max {max(v):8.1f}"


def region(stream, calls, fn):
    """us per call of `calls` calls of fn: device time between two events on the context's stream"""
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record(stream)
    for _ in range(calls):
        fn()
    end.record(stream)
    end.synchronize()
    return begin.elapsed_time(end) * 1e3 / calls


class Frame:
    """A context with config `name`'s scene, a rendered one-sample frame and its guide."""

    def __init__(self, name):
        self.scene_name, kernel = CONFIGS[name]
        self.s = wscene.generate(self.scene_name)
        self.ctx = ctx = wcpt.Context(0)
        self.stream = torch.cuda.Stream()
        ctx.set_stream(self.stream.cuda_stream)
        ctx.set_kernel(kernel)
        self.dev = wcpt.DeviceScene(ctx, self.s)
        ctx.create_screen(W, H)
        self.sd = self.s.scene_data(W, H, max_bounce=4, samples=1, frame=0)
        ctx.render(self.sd, *self.dev.addresses())
        self.guide_bytes = W * H * T.PRIMARY_HIT_DTYPE.itemsize
        self.guide_buf = ctx.buffer_alloc(self.guide_bytes)
        self.guide = ctx.buffer_address(self.guide_buf)
        self.dst_buf = ctx.buffer_alloc(W * H * 4)
        self.dst = ctx.buffer_address(self.dst_buf)
        self.trace()
        ctx.sync()

    def trace(self):
        self.ctx.trace_primary(self.sd, self.dev.spheres, self.dev.draws, dst=self.guide, nbytes=self.guide_bytes)

    def calls(self):
        """label -> the call"""
        ctx, dst = self.ctx, self.dst
        out = {"a": lambda: ctx.composite(dst, rgba8=True), "b": lambda: ctx.composite(dst, rgba8=True, bloom=wcpt.BloomParams())}
        for n in ITERATIONS:
            out[f"d{n}"] = (lambda p: lambda: ctx.composite(dst, rgba8=True, denoise=p, guide=self.guide,
                                                            guide_bytes=self.guide_bytes))(wcpt.DenoiseParams(n))
        out["g"] = self.trace
        return out

    def close(self):
        self.ctx.buffer_free(self.guide_buf)
        self.ctx.buffer_free(self.dst_buf)
        self.dev.free()
        self.ctx.close()


LABELS = {"a": "(a) wcpt_composite", "b": "(b) wcpt_composite_bloom, defaults", "g": "(g) wcpt_trace_primary, the guide pass"}
LABELS.update({f"d{n}": f"(d{n}) wcpt_composite_denoise, {n} iteration{'s' if n > 1 else ''}" for n in ITERATIONS})


def ab(name, rounds, calls):
    f = Frame(name)
    try:
        fns = f.calls()
        us = {k: [] for k in fns}
        for r in range(-1, rounds):
            for k, fn in fns.items():
                v = region(f.stream, calls, fn)
                if r >= 0:
                    us[k].append(v)
        f.ctx.sync()
    finally:
        f.close()
    lines = [f"{name}: {f.scene_name}, {W}x{H}, RGBA8"]
    lines += [f"  {LABELS[k]:<50}{fmt(v)}  us per call" for k, v in us.items()]
    d1, d5 = statistics.median(us["d1"]), statistics.median(us["d5"])
    lines.append(f"       per iteration beyond the first, by medians: {(d5 - d1) / 4.0:.1f} us")
    return lines


def once(name):
    f = Frame(name)
    try:
        for fn in f.calls().values():
            fn()
        f.ctx.sync()
    finally:
        f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_ab.log"))
    a = ap.parse_args()
    if a.once:
        once(a.once)
        return
    lines = [f"build_id {wcpt.lib.wcpt_build_id().decode()}  rounds {a.rounds} (interleaved), {a.calls} calls per round "
             "(device events on the context's stream around the calls)"]
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
