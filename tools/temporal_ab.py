"""Display-step A/B on one GPU: what wcpt_composite_temporal costs beside the display calls of the same build. One process,
interleaved rounds, on c2 (Cornell) at 1920x1080, RGBA8, with an orbiting camera: the image is a rendered one-sample frame (4
bounces, frame 0) and there are two guides, wcpt_trace_primary's records of the start camera and of the camera yawed by 1.5
degrees; consecutive restart calls alternate between the two, so every one of them reprojects across a move and finds its
history. Per round, N calls each of
  (a)  wcpt_composite;
  (d1) (d3) wcpt_composite_denoise at 1 and 3 iterations, the other parameters the defaults;
  (tr) wcpt_composite_temporal, a restart call (the reproject-and-blend kernel), the defaults;
  (tn) wcpt_composite_temporal, a call that is no restart (the streaming blend kernel);
  (tr1) (tr3) a restart call followed by 1 and 3 denoise iterations in the same call.
The context runs on a torch stream of its own; each figure is the device time between two events on that stream around
N back-to-back calls, divided by N. One untimed warm-up round first. Median and range over the rounds; no threshold.

    python tools/temporal_ab.py [--rounds 7] [--calls 20] [--out LOG]
    python tools/temporal_ab.py --once        one call of each and nothing else: the program of a kernel trace

The log is profiles/temporal_ab.log.
"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "wc-path-tracer_amd"), ROOT]

import torch  # noqa: E402

import wcpt  # noqa: E402
from wcpt import scene as wscene  # noqa: E402

T = wcpt._lib
W, H = 1920, 1080
ITERATIONS = (1, 3)
YAW_STEP = 1.5
# what a restart call must move per pixel, RGBA8: the record and the accumulation texel in (48 + 16), base, the packed
# guide, hist and its length out (16 + 32 + 16 + 4), the display texel (4), and of the four taps' 4 x 52 bytes the 52 that
# no neighbour shares
RESTART_BYTES = 48 + 16 + 16 + 32 + 16 + 4 + 4 + 52
BLEND_BYTES = 16 + 16 + 16 + 4 + 4


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


class Orbit:
    """A context with c2's scene, a rendered one-sample frame and the guides of two cameras 1.5 degrees apart."""

    def __init__(self):
        self.s = wscene.generate("cornell")
        self.ctx = ctx = wcpt.Context(0)
        self.stream = torch.cuda.Stream()
        ctx.set_stream(self.stream.cuda_stream)
        ctx.set_kernel(wcpt.KERNEL_MEGAKERNEL)
        self.dev = wcpt.DeviceScene(ctx, self.s)
        ctx.create_screen(W, H)
        self.guide_bytes = W * H * T.PRIMARY_HIT_DTYPE.itemsize
        self.sd, self.guide_buf, self.guide = [], [], []
        for step in range(2):
            cam = copy.copy(self.s.camera)
            cam.yaw = self.s.camera.yaw + YAW_STEP * step
            sd = self.s.scene_data(W, H, max_bounce=4, samples=1, frame=0, camera=cam)
            buf = ctx.buffer_alloc(self.guide_bytes)
            ctx.trace_primary(sd, self.dev.spheres, self.dev.draws, dst=ctx.buffer_address(buf), nbytes=self.guide_bytes)
            self.sd.append(sd)
            self.guide_buf.append(buf)
            self.guide.append(ctx.buffer_address(buf))
        ctx.render(self.sd[0], *self.dev.addresses())
        self.dst_buf = ctx.buffer_alloc(W * H * 4)
        self.dst = ctx.buffer_address(self.dst_buf)
        self.turn = 0
        self.params = wcpt.TemporalParams()
        ctx.sync()

    def temporal(self, restart, denoise=None):
        if restart:
            self.turn ^= 1
        i = self.turn
        self.ctx.composite(self.dst, rgba8=True, temporal=self.params, scene=self.sd[i], frames=1, restart=restart,
                           denoise=denoise, guide=self.guide[i], guide_bytes=self.guide_bytes)

    def calls(self):
        """label -> the call"""
        ctx, dst = self.ctx, self.dst
        out = {"a": lambda: ctx.composite(dst, rgba8=True)}
        for n in ITERATIONS:
            out[f"d{n}"] = (lambda p: lambda: ctx.composite(dst, rgba8=True, denoise=p, guide=self.guide[0],
                                                            guide_bytes=self.guide_bytes))(wcpt.DenoiseParams(n))
        out["tr"] = lambda: self.temporal(True)
        out["tn"] = lambda: self.temporal(False)
        for n in ITERATIONS:
            out[f"tr{n}"] = (lambda p: lambda: self.temporal(True, p))(wcpt.DenoiseParams(n))
        return out

    def close(self):
        for b in self.guide_buf + [self.dst_buf]:
            self.ctx.buffer_free(b)
        self.dev.free()
        self.ctx.close()


LABELS = {"a": "(a) wcpt_composite", "tr": "(tr) wcpt_composite_temporal, restart", "tn": "(tn) wcpt_composite_temporal, no restart"}
LABELS.update({f"d{n}": f"(d{n}) wcpt_composite_denoise, {n} iteration{'s' if n > 1 else ''}" for n in ITERATIONS})
LABELS.update({f"tr{n}": f"(tr{n}) temporal restart + {n} denoise iteration{'s' if n > 1 else ''}" for n in ITERATIONS})


def ab(rounds, calls):
    f = Orbit()
    try:
        fns = f.calls()
        f.temporal(True)                           # the first call has no history: not one of the timed ones
        us = {k: [] for k in fns}
        for r in range(-1, rounds):
            for k, fn in fns.items():
                v = region(f.stream, calls, fn)
                if r >= 0:
                    us[k].append(v)
        f.ctx.sync()
    finally:
        f.close()
    lines = [f"c2: cornell, {W}x{H}, RGBA8, camera yawing {YAW_STEP} degrees between restarts"]
    lines += [f"  {LABELS[k]:<50}{fmt(v)}  us per call" for k, v in us.items()]
    pixels = W * H
    for k, nbytes, what in (("tr", RESTART_BYTES, "restart"), ("tn", BLEND_BYTES, "no restart")):
        t = statistics.median(us[k]) * 1e-6
        lines.append(f"       {what}: {nbytes} bytes per pixel to move = {nbytes * pixels / 1e6:.1f} MB per call, "
                     f"{nbytes * pixels / t / 1e12:.2f} TB/s at the median")
    for n in ITERATIONS:
        lines.append(f"       restart + {n} denoise iterations less denoise alone, by medians: "
                     f"{statistics.median(us[f'tr{n}']) - statistics.median(us[f'd{n}']):.1f} us")
    return lines


def once():
    f = Orbit()
    try:
        f.temporal(True)
        for fn in f.calls().values():
            fn()
        f.ctx.sync()
    finally:
        f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_ab.log"))
    a = ap.parse_args()
    if a.once:
        once()
        return
    lines = [f"build_id {wcpt.lib.wcpt_build_id().decode()}  rounds {a.rounds} (interleaved), {a.calls} calls per round "
             "(device events on the context's stream around the calls)"]
    print(lines[0], flush=True)
    got = ab(a.rounds, a.calls)
    print("\n".join(got), flush=True)
    lines += got
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
