"""Multi-device paths on the GPU box, through the product library:

- the C-ABI group (wcpt_group_*: one context per rank from one host thread, row blocks, a gather of each presented frame
  to the root) at n = 1, bit-identical to a plain context, in every payload format; its error paths;
- the same group at n = 2..4 on the one GPU with the COPY transport (every rank its own context, streams, double-buffered
  payloads and overlap events; only the wire differs from RCCL's), bit-identical to one context, overlapped and in line,
  across resizes, and atomic when one rank's arguments are bad;
- two ranks with libwcpt.so each rendering their row block of the frame on the one GPU, gathered over gloo (RCCL refuses
  two ranks on one device), against a one-context render.

The RCCL send/recv of an N > 1 group needs N distinct devices: the driver's scaling bench runs it (bench.py --gpus N, or
one process per GPU under torchrun); a one-GPU box cannot.
"""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import wcpt
import oracle

from test_gpu_parity import assert_close, get_scene

pytestmark = pytest.mark.gpu

PB = wcpt._lib.PAYLOAD_PIXEL_BYTES


def _context_frames(s, W, H, frames, bounces=4, kernel=wcpt.KERNEL_MEGAKERNEL, samples=1):
    with wcpt.Context(0) as ctx:
        dev = wcpt.DeviceScene(ctx, s)
        ctx.set_kernel(kernel)
        ctx.create_screen(W, H)
        for f in frames:
            ctx.render(s.scene_data(W, H, max_bounce=bounces, samples=samples, frame=f), *dev.addresses())
        ctx.sync()
        img = ctx.readback()
        dev.free()
    return img


@pytest.mark.parametrize("fmt", [wcpt._lib.PAYLOAD_RGBA32F, wcpt._lib.PAYLOAD_RGB32F,
                                 wcpt._lib.PAYLOAD_DISPLAY_RGBA8])
@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_of_one_equals_context(gpu_ctx, fmt, kernel):
    """wcpt_group_* at n = 1 on device 0: progressive frames presented into a root-context buffer equal a plain
    context's accumulation image bit for bit (RGBA / RGB floats), or its composite.comp display value (RGBA8)."""
    s = get_scene("cornell")
    W, H, frames = 72, 40, (0, 1, 2)
    ref = _context_frames(s, W, H, frames, kernel=kernel)
    with wcpt.Group([0], root=0) as g:
        ctx = g.context(0)
        dev = wcpt.DeviceScene(ctx, s)
        ctx.set_kernel(kernel)
        g.create_screen(W, H)
        nbytes = W * H * PB[fmt]
        out = ctx.buffer_from(np.full(nbytes // 4, -3.0, np.float32))
        g.set_output(fmt, ctx.buffer_address(out), nbytes)
        for f in frames:
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), [dev.materials], [dev.spheres], [dev.draws])
        g.sync()
        raw = ctx.buffer_download(out, nbytes)
        img = ctx.readback()
        ctx.buffer_free(out)
        dev.free()
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    if fmt == wcpt._lib.PAYLOAD_DISPLAY_RGBA8:
        assert np.array_equal(np.frombuffer(raw, np.uint8).reshape(H, W, 4), oracle.composite(ref)[1])
    else:
        ch = 4 if fmt == wcpt._lib.PAYLOAD_RGBA32F else 3
        got = np.frombuffer(raw, np.float32).reshape(H, W, ch)
        assert np.array_equal(got.view(np.uint32), ref[..., :ch].view(np.uint32))


def test_group_matches_oracle_and_resizes(gpu_ctx):
    """The group's frame equals the oracle's; after a resize (CreateScreen of the group) the next frame 0 is again the
    oracle's, and an output too small for the new frame is refused."""
    s = get_scene("default_dielectric")
    with wcpt.Group([0]) as g:
        ctx = g.context(0)
        dev = wcpt.DeviceScene(ctx, s)
        for (W, H) in ((48, 40), (64, 24)):
            g.create_screen(W, H)
            nbytes = W * H * 16
            out = ctx.buffer_alloc(nbytes)
            g.set_output(wcpt._lib.PAYLOAD_RGBA32F, ctx.buffer_address(out), nbytes)
            sd = s.scene_data(W, H, max_bounce=3, frame=0)
            g.render(sd, [dev.materials], [dev.spheres], [dev.draws])
            g.sync()
            got = np.frombuffer(ctx.buffer_download(out, nbytes), np.float32).reshape(H, W, 4)
            ref, _ = oracle.render_scene(s, W, H, sd=sd, threads=8)
            assert_close(got.copy(), ref)
            with pytest.raises(wcpt.WcptError):
                g.set_output(wcpt._lib.PAYLOAD_RGBA32F, ctx.buffer_address(out), nbytes - 16)
            g.set_output(wcpt._lib.PAYLOAD_RGBA32F, 0, 0)
            ctx.buffer_free(out)
        dev.free()


def test_group_errors(gpu_ctx):
    with pytest.raises(wcpt.WcptError):
        wcpt.Group([0, 0])                      # one rank per device (RCCL refuses duplicates)
    with pytest.raises(wcpt.WcptError):
        wcpt.Group([0], root=1)
    with pytest.raises(wcpt.WcptError):
        wcpt.Group([wcpt.device_count()])       # no such device
    with wcpt.Group([0]) as g:
        s = get_scene("cornell")
        dev = wcpt.DeviceScene(g.context(0), s)
        with pytest.raises(wcpt.WcptError) as e:
            g.render(s.scene_data(8, 8), [dev.materials], [dev.spheres], [dev.draws])
        assert e.value.code == -1003            # no screen yet
        with pytest.raises(wcpt.WcptError):
            g.set_output(5, 4096, 4096)         # unknown format
        dev.free()


# ---- two ranks with libwcpt.so, gathered over gloo --------------------------------------------------------------
def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    p = sk.getsockname()[1]
    sk.close()
    return p


def _rank(rank, world, port, W, H, frames, kernel, out_path):
    import sys
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "wc-path-tracer_amd")]
    import wcpt as w
    from wcpt import scene as wscene
    from wcpt.dist import gather_frame, row_block
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = wscene.generate("cornell")
    y0, rows = row_block(H, world, rank)
    with w.Context(0) as ctx:
        dev = w.DeviceScene(ctx, s)
        ctx.set_kernel(kernel)
        ctx.create_screen(W, H)
        ctx.set_row_range(y0, rows)
        for f in frames:
            ctx.render(s.scene_data(W, H, max_bounce=4, frame=f), *dev.addresses())
        ctx.sync()
        block = ctx.readback(rows)
        dev.free()
    shard = torch.zeros((-(-H // world), W, 4), dtype=torch.float32)
    shard[:rows] = torch.from_numpy(block)
    frame = gather_frame(shard, H, world, rank, rgb_only=True)
    if rank == 0:
        np.save(out_path, frame.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_two_ranks_libwcpt_gather_equals_one_device(gpu_ctx, tmp_path, kernel):
    """Two processes, each with its own libwcpt context on the GPU, render rows [0, H/2) and [H/2, H) of the same
    progressive frames; the blocks gathered on rank 0 (RGB wire format, alpha restored) equal one context's frame
    bit for bit, and that frame equals the oracle's."""
    W, H, frames = 64, 45, (0, 1)
    out = str(tmp_path / "frame.npy")
    mp.spawn(_rank, args=(2, _free_port(), W, H, frames, kernel, out), nprocs=2, join=True)
    got = np.load(out)
    s = get_scene("cornell")
    ref = _context_frames(s, W, H, frames, kernel=kernel)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    acc = None
    for f in frames:
        acc, _ = oracle.render_scene(s, W, H, max_bounce=4, frame=f, image=acc, threads=8)
    assert_close(got, acc)


def _rank_display(rank, world, port, W, H, frames, kernel, out_path):
    """One rank of the display-payload gather (bench.py --gather display): the render itself writes composite.comp's
    RGBA8 display value of the rank's row block into a device payload (WCPT_PAYLOAD_DISPLAY_RGBA8), which travels
    at 4 B/px."""
    import sys
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "wc-path-tracer_amd")]
    import wcpt as w
    from wcpt import scene as wscene
    from wcpt.dist import assemble, row_block
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = wscene.generate("cornell")
    y0, rows = row_block(H, world, rank)
    payload = torch.zeros((-(-H // world), W, 4), dtype=torch.uint8, device="cuda")
    with w.Context(0) as ctx:
        dev = w.DeviceScene(ctx, s)
        ctx.set_kernel(kernel)
        ctx.create_screen(W, H)
        ctx.set_row_range(y0, rows)
        ctx.set_gather_output(payload.data_ptr(), payload.numel(), w._lib.PAYLOAD_DISPLAY_RGBA8)
        for f in frames:
            ctx.render(s.scene_data(W, H, max_bounce=4, frame=f), *dev.addresses())
        ctx.sync()
        dev.free()
    block = payload.cpu()
    parts = [torch.empty_like(block) for _ in range(world)] if rank == 0 else None
    dist.gather(block, parts, dst=0)
    if rank == 0:
        np.save(out_path, assemble(parts, H, world).numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_two_ranks_display_payload_gather_equals_oracle_composite(gpu_ctx, tmp_path, kernel):
    """Two ranks render their row blocks with the RGBA8 display payload written by the render, gather the 4-B/px
    blocks over gloo, and rank 0's frame equals composite.comp (oracle.composite) of the oracle's accumulated frame
    byte for byte (composite.comp:36-53)."""
    W, H, frames = 64, 45, (0, 1, 2)
    out = str(tmp_path / "display.npy")
    mp.spawn(_rank_display, args=(2, _free_port(), W, H, frames, kernel, out), nprocs=2, join=True)
    got = np.load(out)
    s = get_scene("cornell")
    acc = None
    for f in frames:
        acc, _ = oracle.render_scene(s, W, H, max_bounce=4, frame=f, image=acc, threads=8)
    _, want = oracle.composite(acc)
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    assert np.array_equal(got, want)


# ---- N-rank groups on the one GPU (COPY transport) --------------------------------------------------------------------
COPY = wcpt._lib.GROUP_TRANSPORT_COPY


def _group_frames(s, W, H, frames, n, fmt, kernel, overlap=True, bounces=4, threads=-1, transport=COPY, root=0,
                  stripe=0, samples=1):
    """Progressive frames through an n-rank COPY (or DIRECT) group on device 0: (presented frame bytes, each rank's
    block). stripe > 0: interleaved row stripes (WCPT_GROUP_OPTION_ROW_STRIPE)."""
    with wcpt.Group([0] * n, root=root, transport=transport) as g:
        if stripe:
            g.set_option(wcpt._lib.GROUP_OPTION_ROW_STRIPE, stripe)
        devs = []
        for r in range(n):
            c = g.context(r)
            c.set_kernel(kernel)
            devs.append(wcpt.DeviceScene(c, s))
        g.set_option(wcpt._lib.GROUP_OPTION_OVERLAP, 1 if overlap else 0)
        g.set_option(wcpt._lib.GROUP_OPTION_THREADS, threads)
        g.create_screen(W, H)
        rc = g.context(root)
        nbytes = W * H * PB[fmt]
        out = rc.buffer_from(np.full(nbytes // 4, -5.0, np.float32))
        g.set_output(fmt, rc.buffer_address(out), nbytes)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        for f in frames:
            g.render(s.scene_data(W, H, max_bounce=bounces, samples=samples, frame=f), *addr)
        g.sync()
        info = g.info()
        raw = rc.buffer_download(out, nbytes)
        blocks = [g.context(r).readback() for r in range(n)]
        rc.buffer_free(out)
        for d in devs:
            d.free()
    assert info["frames"] == len(frames) and info["local_ranks"] == n and info["nranks"] == n
    assert info["transport"] == transport and info["distinct_devices"] == 1 and info["broken"] == 0
    assert info["issue_threads"] == (n - 1 if threads == 1 and n > 1 else 0)  # one device: threads off by default
    return raw, blocks


def _as_frame(raw, fmt, W, H):
    if fmt == wcpt._lib.PAYLOAD_DISPLAY_RGBA8:
        return np.frombuffer(raw, np.uint8).reshape(H, W, 4)
    return np.frombuffer(raw, np.float32).reshape(H, W, 4 if fmt == wcpt._lib.PAYLOAD_RGBA32F else 3)


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("fmt", [wcpt._lib.PAYLOAD_RGB32F, wcpt._lib.PAYLOAD_RGBA32F, wcpt._lib.PAYLOAD_DISPLAY_RGBA8])
@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_of_n_ranks_equals_one_device(gpu_ctx, n, fmt, kernel):
    """An n-rank group (one host thread, n contexts) presents, frame after frame, the one-device frame bit for bit:
    every rank renders its row block with the global seeds, payload buffers alternate between frames while the previous
    frame's transfer is in flight, and the blocks land at their rows of the root's output. Each rank keeps only its
    block of the accumulation, equal to those rows of the one-device image."""
    s = get_scene("cornell")
    W, H, frames = 72, 45, (0, 1, 2, 3)
    ref = _context_frames(s, W, H, frames, kernel=kernel)
    raw, blocks = _group_frames(s, W, H, frames, n, fmt, kernel)
    got = _as_frame(raw, fmt, W, H)
    if fmt == wcpt._lib.PAYLOAD_DISPLAY_RGBA8:
        assert np.array_equal(got, oracle.composite(ref)[1])
    else:
        assert np.array_equal(got.view(np.uint32), ref[..., :got.shape[2]].view(np.uint32))
    from wcpt.dist import row_block
    for r, blk in enumerate(blocks):
        y0, rows = row_block(H, n, r)
        assert np.array_equal(blk.view(np.uint32), ref[y0:y0 + rows].view(np.uint32))


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_overlapped_and_inline_gathers_agree(gpu_ctx, kernel):
    """WCPT_GROUP_OPTION_OVERLAP on (communication streams, double-buffered payloads) and off (transfers in line with
    the renders) present the same bytes over many frames, and both equal the oracle's accumulated frame."""
    s = get_scene("default_dielectric")
    W, H, frames = 40, 27, tuple(range(9))
    a, _ = _group_frames(s, W, H, frames, 3, wcpt._lib.PAYLOAD_RGBA32F, kernel, overlap=True, bounces=3)
    b, _ = _group_frames(s, W, H, frames, 3, wcpt._lib.PAYLOAD_RGBA32F, kernel, overlap=False, bounces=3)
    assert a == b
    acc = None
    for f in frames:
        acc, _ = oracle.render_scene(s, W, H, max_bounce=3, frame=f, image=acc, threads=8)
    assert_close(_as_frame(a, wcpt._lib.PAYLOAD_RGBA32F, W, H).copy(), acc)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
@pytest.mark.parametrize("overlap", [True, False])
def test_group_issue_threads_present_the_same_frames(gpu_ctx, n, kernel, overlap):
    """WCPT_GROUP_OPTION_THREADS 1: every local rank but the first issues its share of each frame from a host thread of
    its own (at 8 ranks the caller's thread alone would spend more host time per frame than a c2 block renders in).
    The presented frames and every rank's block equal the one-thread group's and one device's, bit for bit, over
    progressive frames, overlapped and in line."""
    s = get_scene("default_dielectric")
    W, H, frames = 56, 33, tuple(range(6))
    ref = _context_frames(s, W, H, frames, kernel=kernel, bounces=3)
    fmt = wcpt._lib.PAYLOAD_RGBA32F
    a, blocks = _group_frames(s, W, H, frames, n, fmt, kernel, overlap=overlap, bounces=3, threads=1)
    b, _ = _group_frames(s, W, H, frames, n, fmt, kernel, overlap=overlap, bounces=3, threads=0)
    assert a == b
    assert np.array_equal(_as_frame(a, fmt, W, H).view(np.uint32), ref.view(np.uint32))
    from wcpt.dist import row_block
    for r, blk in enumerate(blocks):
        y0, rows = row_block(H, n, r)
        assert np.array_equal(blk.view(np.uint32), ref[y0:y0 + rows].view(np.uint32))


DIRECT = wcpt._lib.GROUP_TRANSPORT_DIRECT


@pytest.mark.parametrize("n,root", [(2, 0), (3, 1), (8, 0)])
@pytest.mark.parametrize("fmt", [wcpt._lib.PAYLOAD_RGB32F, wcpt._lib.PAYLOAD_RGBA32F, wcpt._lib.PAYLOAD_DISPLAY_RGBA8])
@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_direct_transport_equals_one_device(gpu_ctx, n, root, fmt, kernel):
    """WCPT_GROUP_TRANSPORT_DIRECT: every rank's render writes its rows of the root's frame itself (over xGMI between
    GPUs; here all ranks share device 0), so a frame is one launch per rank with no transfer, event or copy. The
    presented frames equal one device's bit for bit (display bytes: composite.comp of them), with any root."""
    s = get_scene("cornell")
    W, H, frames = 64, 37, (0, 1, 2)
    ref = _context_frames(s, W, H, frames, kernel=kernel)
    raw, blocks = _group_frames(s, W, H, frames, n, fmt, kernel, transport=DIRECT, root=root)
    got = _as_frame(raw, fmt, W, H)
    if fmt == wcpt._lib.PAYLOAD_DISPLAY_RGBA8:
        assert np.array_equal(got, oracle.composite(ref)[1])
    else:
        assert np.array_equal(got.view(np.uint32), ref[..., :got.shape[2]].view(np.uint32))
    from wcpt.dist import row_block
    for r, blk in enumerate(blocks):
        y0, rows = row_block(H, n, r)
        assert np.array_equal(blk.view(np.uint32), ref[y0:y0 + rows].view(np.uint32))


def test_group_direct_transport_across_resizes_and_outputs(gpu_ctx):
    """DIRECT: a resize re-points every rank's rows at the frame of the new size; a new output re-points them at the new
    buffer; presenting off and on again; each presented frame equals one device's."""
    s = get_scene("default_dielectric")
    with wcpt.Group([0, 0, 0], transport=DIRECT) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(3)]
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        root = g.context(0)
        got = []
        for (W, H) in ((40, 21), (72, 30)):
            g.create_screen(W, H)
            nbytes = W * H * 16
            out = root.buffer_alloc(nbytes)
            g.set_output(wcpt._lib.PAYLOAD_RGBA32F, root.buffer_address(out), nbytes)
            g.render(s.scene_data(W, H, max_bounce=3, frame=0), *addr)
            g.set_output(0, 0, 0)
            g.render(s.scene_data(W, H, max_bounce=3, frame=1), *addr)   # accumulates, not presented
            g.set_output(wcpt._lib.PAYLOAD_RGBA32F, root.buffer_address(out), nbytes)
            g.render(s.scene_data(W, H, max_bounce=3, frame=2), *addr)
            g.sync()
            got.append((W, H, np.frombuffer(root.buffer_download(out, nbytes), np.float32).reshape(H, W, 4).copy()))
            g.set_output(0, 0, 0)
            root.buffer_free(out)
        for d in devs:
            d.free()
    for W, H, img in got:
        ref = _context_frames(s, W, H, (0, 1, 2), bounces=3)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (W, H)


def test_group_issue_threads_refuse_bad_arguments_atomically(gpu_ctx):
    """With issue threads on, a frame whose rank-2 arguments are invalid is still refused before any rank renders
    (validation stays on the caller's thread), and the group goes on bit-exactly."""
    s = get_scene("cornell")
    W, H = 40, 21
    with wcpt.Group([0, 0, 0], transport=COPY) as g:
        g.set_option(wcpt._lib.GROUP_OPTION_THREADS, 1)
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(3)]
        g.create_screen(W, H)
        root = g.context(0)
        out = root.buffer_alloc(W * H * 16)
        g.set_output(wcpt._lib.PAYLOAD_RGBA32F, root.buffer_address(out), W * H * 16)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        g.render(s.scene_data(W, H, max_bounce=4, frame=0), *addr)
        bad = [list(x) for x in addr]
        bad[0][2] = 0                                   # rank 2: null material buffer
        with pytest.raises(wcpt.WcptError) as e:
            g.render(s.scene_data(W, H, max_bounce=4, frame=1), *bad)
        assert e.value.code == -1000
        info = g.info()
        assert info["broken"] == 0 and info["frames"] == 1 and info["issue_threads"] == 2
        for f in (1, 2):
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.sync()
        got = np.frombuffer(root.buffer_download(out, W * H * 16), np.float32).reshape(H, W, 4)
        root.buffer_free(out)
        for d in devs:
            d.free()
    ref = _context_frames(s, W, H, (0, 1, 2))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_group_rank_with_bad_arguments_renders_nothing(gpu_ctx):
    """A frame whose rank-1 arguments are invalid (a draw command whose indexCount exceeds its index buffer) is refused
    before any rank renders: the error comes back, no accumulation advances, the group stays usable, and the frames
    that follow equal a one-device sequence without the refused frame. Destroying the group afterwards does not hang."""
    s = get_scene("cornell")
    W, H = 48, 30
    with wcpt.Group([0, 0, 0], transport=COPY) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(3)]
        g.create_screen(W, H)
        root = g.context(0)
        out = root.buffer_alloc(W * H * 16)
        g.set_output(wcpt._lib.PAYLOAD_RGBA32F, root.buffer_address(out), W * H * 16)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        g.render(s.scene_data(W, H, max_bounce=4, frame=0), *addr)
        c1 = g.context(1)
        bad_draws = np.zeros(1, dtype=wcpt.DRAW_COMMAND_DTYPE)
        m = s.meshes[0]
        vb, ib, nb = (c1.buffer_from(m.positions), c1.buffer_from(m.indices), c1.buffer_from(m.nodes))
        bad_draws[0] = (c1.buffer_address(vb), c1.buffer_address(ib), c1.buffer_address(nb), m.indices.size + 300, 0)
        bd = c1.buffer_from(bad_draws)
        bad = [list(x) for x in addr]
        bad[2][1] = c1.buffer_address(bd)
        with pytest.raises(wcpt.WcptError) as e:
            g.render(s.scene_data(W, H, max_bounce=4, frame=1), *bad)
        assert e.value.code == -1000
        assert g.info()["broken"] == 0 and g.info()["frames"] == 1
        for f in (1, 2):
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.sync()
        got = np.frombuffer(root.buffer_download(out, W * H * 16), np.float32).reshape(H, W, 4)
        for b in (vb, ib, nb, bd):
            c1.buffer_free(b)
        root.buffer_free(out)
        for d in devs:
            d.free()
    ref = _context_frames(s, W, H, (0, 1, 2))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_group_resize_regrows_payloads_without_device_sync(gpu_ctx):
    """Resizing a 2-rank overlapped group to a larger frame regrows each sender's payload buffers while earlier
    transfers may still be queued (the replaced buffers are retired and freed at the next group-wide wait, with no
    device synchronisation); an output too small for the new frame is refused and presenting stops until a new one is
    set; the next frames equal the one-device frames of the new size."""
    s = get_scene("cornell")
    with wcpt.Group([0, 0], transport=COPY) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(2)]
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        root = g.context(0)
        results = []
        prev = None
        for (W, H) in ((32, 20), (80, 50), (24, 9)):
            nbytes = W * H * 12
            out = root.buffer_alloc(nbytes)
            if prev is not None and W * H > prev[1]:
                with pytest.raises(wcpt.WcptError):
                    g.create_screen(W, H)           # the previous output is too small: presenting stops
                assert g.info()["frames"] == 2 * len(results)
            else:
                g.create_screen(W, H)
            g.set_output(wcpt._lib.PAYLOAD_RGB32F, root.buffer_address(out), nbytes)
            if prev is not None:
                root.buffer_free(prev[0])
            prev = (out, W * H)
            for f in (0, 1):
                g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
            g.sync()
            results.append((W, H, np.frombuffer(root.buffer_download(out, nbytes), np.float32).reshape(H, W, 3)))
        g.set_output(wcpt._lib.PAYLOAD_RGB32F, 0, 0)
        root.buffer_free(prev[0])
        for d in devs:
            d.free()
    for W, H, got in results:
        ref = _context_frames(s, W, H, (0, 1))
        assert np.array_equal(got.view(np.uint32), ref[..., :3].view(np.uint32)), (W, H)


def test_rank_group_of_one_and_unique_id(gpu_ctx):
    """The one-process-per-device entry points on one GPU: wcpt_group_unique_id gives RCCL's 128-byte id, and a rank
    group of one (wcpt_group_create_rank with nranks = 1, no communicator needed) renders and presents exactly as a
    plain context; its info reports one rank, the RCCL transport and no exchange."""
    uid = wcpt.group_unique_id()
    assert len(uid) == wcpt._lib.GROUP_UNIQUE_ID_BYTES and any(uid)
    s = get_scene("cornell")
    W, H, frames = 40, 30, (0, 1, 2)
    ref = _context_frames(s, W, H, frames)
    with wcpt.Group.rank(0, 1, 0, root=0, uid=uid) as g:
        assert g.context(1) is None
        ctx = g.context(0)
        dev = wcpt.DeviceScene(ctx, s)
        g.create_screen(W, H)
        nbytes = W * H * 16
        out = ctx.buffer_alloc(nbytes)
        g.set_output(wcpt._lib.PAYLOAD_RGBA32F, ctx.buffer_address(out), nbytes)
        for f in frames:
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), [dev.materials], [dev.spheres], [dev.draws])
        g.sync()
        info = g.info()
        got = np.frombuffer(ctx.buffer_download(out, nbytes), np.float32).reshape(H, W, 4)
        ctx.buffer_free(out)
        dev.free()
    assert info["nranks"] == 1 and info["local_ranks"] == 1 and info["first_local_rank"] == 0
    assert info["transport"] == wcpt._lib.GROUP_TRANSPORT_RCCL and info["frames"] == len(frames)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_group_option_and_transport_errors(gpu_ctx):
    """Unknown group options and transports are refused; the overlap switch can be flipped between frames."""
    with pytest.raises(wcpt.WcptError):
        wcpt.Group([0], transport=9)
    with wcpt.Group([0, 0], transport=COPY) as g:
        with pytest.raises(wcpt.WcptError):
            g.set_option(99, 1)
        g.set_option(wcpt._lib.GROUP_OPTION_OVERLAP, 0)
        assert g.info()["overlap"] == 0
        g.set_option(wcpt._lib.GROUP_OPTION_OVERLAP, 1)
        assert g.info()["overlap"] == 1 and g.info()["nranks"] == 2


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_overlapped_payload_reuse_waits_for_the_previous_transfer(gpu_ctx, kernel):
    """Event ordering of the overlapped gather: five frames are presented into five different outputs with no wait in
    between, so frame k+2 rewrites the payload buffer frame k's transfer reads from. Each output must hold exactly its
    own progressive frame; a payload rewritten before its transfer finished would put frame k+2's rows into output k."""
    s = get_scene("cornell")
    W, H, n, frames = 64, 48, 3, (0, 1, 2, 3, 4)
    nbytes = W * H * 16
    with wcpt.Group([0] * n, transport=COPY) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(n)]
        for r in range(n):
            g.context(r).set_kernel(kernel)
        g.set_option(wcpt._lib.GROUP_OPTION_OVERLAP, 1)
        g.create_screen(W, H)
        root = g.context(0)
        outs = [root.buffer_alloc(nbytes) for _ in frames]
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        for f, o in zip(frames, outs):
            g.set_output(wcpt._lib.PAYLOAD_RGBA32F, root.buffer_address(o), nbytes)
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.sync()
        got = [np.frombuffer(root.buffer_download(o, nbytes), np.float32).reshape(H, W, 4) for o in outs]
        for o in outs:
            root.buffer_free(o)
        for d in devs:
            d.free()
    for k, f in enumerate(frames):
        ref = _context_frames(s, W, H, frames[:k + 1], kernel=kernel)
        assert np.array_equal(got[k].view(np.uint32), ref.view(np.uint32)), k


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_with_a_middle_root_and_presenting_toggled(gpu_ctx, kernel):
    """Rank 1 of 3 as the root (its own block in the middle of the frame, the blocks of ranks 0 and 2 landing above and
    below it), 37 rows (blocks of 12, 12 and 13), and presenting switched off for two frames and on again (bench.py's
    untimed re-render): the ranks keep accumulating while nothing is gathered, and the next presented frame equals the
    one-device frame of the whole sequence."""
    s = get_scene("cornell")
    W, H, n, frames = 44, 37, 3, (0, 1, 2, 3, 4)
    fmt, px = wcpt._lib.PAYLOAD_RGB32F, 12
    nbytes = W * H * px
    with wcpt.Group([0] * n, root=1, transport=COPY) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(n)]
        for r in range(n):
            g.context(r).set_kernel(kernel)
        g.create_screen(W, H)
        root = g.context(1)
        out = root.buffer_from(np.full(nbytes // 4, -3.0, np.float32))
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        g.set_output(fmt, root.buffer_address(out), nbytes)
        g.render(s.scene_data(W, H, max_bounce=4, frame=0), *addr)
        g.set_output(0, 0, 0)                      # presenting off: frames 1 and 2 accumulate only
        for f in (1, 2):
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.set_output(fmt, root.buffer_address(out), nbytes)
        for f in (3, 4):
            g.render(s.scene_data(W, H, max_bounce=4, frame=f), *addr)
        g.sync()
        info = g.info()
        got = np.frombuffer(root.buffer_download(out, nbytes), np.float32).reshape(H, W, 3)
        root.buffer_free(out)
        for d in devs:
            d.free()
    assert info["root"] == 1 and info["frames"] == len(frames)
    ref = _context_frames(s, W, H, frames, kernel=kernel)
    assert np.array_equal(got.view(np.uint32), ref[..., :3].view(np.uint32))


def test_device_pci_bus_id_names_the_gpu(gpu_ctx):
    """wcpt_device_pci_bus_id: the identity bench.py counts GPUs by across processes ("dddd:bb:dd.f"); a device
    ordinal that does not exist is an error."""
    import re
    ident = wcpt.device_pci_bus_id(0)
    assert re.fullmatch(r"[0-9a-fA-F]{4}:[0-9a-fA-F]{2}:[0-9a-fA-F]{2}\.[0-9a-fA-F]", ident), ident
    with pytest.raises(wcpt.WcptError):
        wcpt.device_pci_bus_id(wcpt.device_count() + 7)


# ---- interleaved row stripes (SURVEY.md §8(e)'s fallback; WCPT_GROUP_OPTION_ROW_STRIPE, wcpt_set_row_stripes) ----------
@pytest.mark.parametrize("n,stripe", [(2, 8), (3, 8), (2, 16), (4, 8), (3, 1)])
@pytest.mark.parametrize("transport", [COPY, DIRECT])
@pytest.mark.parametrize("fmt", [wcpt._lib.PAYLOAD_RGB32F, wcpt._lib.PAYLOAD_DISPLAY_RGBA8])
@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_row_stripes_equal_one_device(gpu_ctx, n, stripe, transport, fmt, kernel):
    """Rank r renders the stripes r, r + n, ... (45 rows: the last stripe is short, and the ranks hold different row
    counts); the root renders its stripes straight into their frame rows, COPY senders copy theirs to their rows
    (hipMemcpy2DAsync), DIRECT senders write their rows themselves. Frame after frame the presented frame equals one
    device's bit for bit, and each rank's accumulation holds exactly its frame rows."""
    from wcpt.dist import frame_rows
    s = get_scene("cornell")
    W, H, frames = 72, 45, (0, 1, 2)
    ref = _context_frames(s, W, H, frames, kernel=kernel)
    raw, blocks = _group_frames(s, W, H, frames, n, fmt, kernel, transport=transport, root=n - 1, stripe=stripe)
    got = _as_frame(raw, fmt, W, H)
    if fmt == wcpt._lib.PAYLOAD_DISPLAY_RGBA8:
        assert np.array_equal(got, oracle.composite(ref)[1])
    else:
        assert np.array_equal(got.view(np.uint32), ref[..., :3].view(np.uint32))
    seen = []
    for r, blk in enumerate(blocks):
        rows = frame_rows(H, n, r, stripe)
        seen += rows
        assert np.array_equal(blk.view(np.uint32), ref[rows].view(np.uint32))
    assert sorted(seen) == list(range(H))


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_group_row_stripes_in_line_multi_sample_and_relayout(gpu_ctx, kernel):
    """Stripes with the gather in line (overlap off) and two samples per pixel (the wavefront shade recomputes the
    primary ray of sample 1 from the frame row), then the option switched on an existing screen (the frame is laid out
    again) -- every presented frame equals one device's."""
    s = get_scene("default_dielectric")
    W, H, frames = 48, 40, (0, 1, 2)
    fmt = wcpt._lib.PAYLOAD_RGBA32F
    ref = _context_frames(s, W, H, frames, kernel=kernel, bounces=3, samples=2)
    raw, _ = _group_frames(s, W, H, frames, 3, fmt, kernel, overlap=False, bounces=3, stripe=8, samples=2)
    assert np.array_equal(_as_frame(raw, fmt, W, H).view(np.uint32), ref.view(np.uint32))
    ref1 = _context_frames(s, W, H, (0,), kernel=kernel, bounces=3)
    with wcpt.Group([0] * 2, root=0, transport=COPY) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(2)]
        for r in range(2):
            g.context(r).set_kernel(kernel)
        g.create_screen(W, H)
        out = g.context(0).buffer_alloc(W * H * 16)
        g.set_output(fmt, g.context(0).buffer_address(out), W * H * 16)
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        g.render(s.scene_data(W, H, max_bounce=3, frame=0), *addr)
        g.set_option(wcpt._lib.GROUP_OPTION_ROW_STRIPE, 16)          # re-laid out: blocks -> stripes
        assert [c.height for c in g.contexts] == [24, 16]
        g.render(s.scene_data(W, H, max_bounce=3, frame=0), *addr)
        g.sync()
        got = np.frombuffer(g.context(0).buffer_download(out, W * H * 16), np.float32).reshape(H, W, 4)
        assert np.array_equal(got.view(np.uint32), ref1.view(np.uint32))
        g.context(0).buffer_free(out)
        for d in devs:
            d.free()


_WALK_SIZES = ((16, 17), (8, 20), (24, 33))
_WALK_REFS = {}


def _walk_reference(s, W, H, k):
    """One context's image of frames 0..k-1 at W x H (one bounce), k even; each size is rendered once and shared."""
    if not _WALK_REFS:
        for (w, h) in _WALK_SIZES:
            with wcpt.Context(0) as ctx:
                dev = wcpt.DeviceScene(ctx, s)
                ctx.create_screen(w, h)
                for f in range(8):
                    ctx.render(s.scene_data(w, h, max_bounce=1, frame=f), *dev.addresses())
                    if f % 2:
                        ctx.sync()
                        _WALK_REFS[(w, h, f + 1)] = ctx.readback().copy()
                dev.free()
    return _WALK_REFS[(W, H, k)]


@pytest.mark.parametrize("transport", [COPY, DIRECT])
def test_group_layout_follows_every_change_on_one_group(gpu_ctx, transport):
    """One group of 3 ranks (root 1) walked through sizes, stripes, formats and presenting off and on: the group keeps a
    table of where every rank's rows go (group_layout.h), laid out again after every accepted change, and a stale table
    would present rows of the previous layout. Two frames after each change; each presented frame equals one context's
    of the frames accumulated since the screen was last laid out, and nothing is written past the frame. None of the
    heights divides by 3; with 8-row stripes 17 rows leave rank 2 only the one-row short stripe, and 17 and 20 rows
    give exactly as many stripes as ranks. Two changes are refused (15 rows and 16-row stripes on 20 rows both give 2
    stripes for 3 ranks): the frames after them continue the layout in force."""
    RGB, RGBA, RGBA8 = wcpt._lib.PAYLOAD_RGB32F, wcpt._lib.PAYLOAD_RGBA32F, wcpt._lib.PAYLOAD_DISPLAY_RGBA8
    STRIPE = wcpt._lib.GROUP_OPTION_ROW_STRIPE
    s = get_scene("cornell")
    cap = 24 * 33 * 16
    sentinel = np.full((cap + 4096) // 4, -7.0, np.float32)
    with wcpt.Group([0, 0, 0], root=1, transport=transport) as g:
        devs = [wcpt.DeviceScene(g.context(r), s) for r in range(3)]
        addr = [list(a) for a in zip(*[d.addresses() for d in devs])]
        root = g.context(1)
        out = root.buffer_from(sentinel)
        state = dict(W=0, H=0, fmt=RGB, frames=0)

        def screen(W, H):
            g.create_screen(W, H)
            state.update(W=W, H=H, frames=0)                  # CreateScreen: the accumulation starts again

        def stripe(rows):
            g.set_option(STRIPE, rows)                        # lays the frame out again
            state.update(frames=0)

        def output(fmt):
            g.set_output(fmt, root.buffer_address(out), cap)
            state.update(fmt=fmt)

        def two_frames(check, step):
            W, H, fmt = state["W"], state["H"], state["fmt"]
            root.buffer_upload(out, sentinel)                 # the group is idle: every check ends in a sync
            for _ in range(2):
                g.render(s.scene_data(W, H, max_bounce=1, frame=state["frames"]), *addr)
                state["frames"] += 1
            g.sync()
            if not check:
                return
            raw = root.buffer_download(out, sentinel.nbytes)
            nbytes = W * H * PB[fmt]
            got = _as_frame(raw[:nbytes], fmt, W, H)
            ref = _walk_reference(s, W, H, state["frames"])
            if fmt == RGBA8:
                assert np.array_equal(got, oracle.composite(ref)[1]), step
            else:
                assert np.array_equal(got.view(np.uint32), ref[..., :got.shape[2]].view(np.uint32)), step
            assert raw[nbytes:] == sentinel.tobytes()[nbytes:], step

        screen(16, 17)
        output(RGB)
        two_frames(True, "16x17 blocks RGB32F")
        stripe(8)
        two_frames(True, "16x17 stripes of 8 (8, 8, 1 rows)")
        output(RGBA8)
        two_frames(True, "16x17 stripes RGBA8")
        screen(8, 20)
        two_frames(True, "8x20 stripes of 8 (8, 8, 4 rows)")
        with pytest.raises(wcpt.WcptError):
            g.set_option(STRIPE, 16)                          # 2 stripes for 3 ranks: refused, stripes of 8 stay
        two_frames(True, "8x20 after the refused stripe change")
        stripe(0)
        two_frames(True, "8x20 blocks RGBA8")
        output(RGBA)
        two_frames(True, "8x20 blocks RGBA32F")
        g.set_output(0, 0, 0)
        two_frames(False, "not presenting")
        output(RGBA)
        two_frames(True, "8x20 presenting again")
        screen(24, 33)
        two_frames(True, "24x33 blocks RGBA32F")
        stripe(8)
        two_frames(True, "24x33 stripes of 8")
        with pytest.raises(wcpt.WcptError):
            g.create_screen(24, 15)                           # 2 stripes for 3 ranks: refused, 24x33 stays
        two_frames(True, "24x33 after the refused resize")
        output(RGB)
        two_frames(True, "24x33 stripes RGB32F")
        stripe(0)
        two_frames(True, "24x33 blocks RGB32F")
        screen(16, 17)
        two_frames(True, "16x17 again")
        info = g.info()
        g.set_output(0, 0, 0)
        root.buffer_free(out)
        for d in devs:
            d.free()
    assert info["broken"] == 0 and info["frames"] == 30


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_context_row_stripes_and_frame_row_output(gpu_ctx, kernel):
    """wcpt_set_row_stripes on one context: its accumulation holds exactly the frame rows of the map, bit-identical to
    a whole-frame render, and with WCPT_OPTION_GATHER_FRAME_ROWS its gather output writes them at their frame rows of a
    shared whole-frame buffer (the other rows untouched)."""
    s = get_scene("cornell")
    W, H = 40, 52
    ref = _context_frames(s, W, H, (0, 1), kernel=kernel)
    for y_first, rows, stripe, period in ((3, 16, 4, 12), (0, 13, 8, 16), (5, 47, 1, 1), (8, 16, 8, 24)):
        with wcpt.Context(0) as ctx:
            dev = wcpt.DeviceScene(ctx, s)
            ctx.set_kernel(kernel)
            ctx.create_screen(W, H)
            ctx.set_row_stripes(y_first, rows, stripe, period)
            want = [y_first + ly + (ly // stripe) * (period - stripe) for ly in range(rows)]
            nbytes = W * H * 16
            out = ctx.buffer_from(np.full(nbytes // 4, -7.0, np.float32))
            ctx.set_option(wcpt._lib.OPTION_GATHER_FRAME_ROWS, 1)
            ctx.set_gather_output(ctx.buffer_address(out), nbytes, wcpt._lib.PAYLOAD_RGBA32F)
            for f in (0, 1):
                ctx.render(s.scene_data(W, H, max_bounce=4, frame=f), *dev.addresses())
            ctx.sync()
            blk = ctx.readback(rows)
            wire = np.frombuffer(ctx.buffer_download(out, nbytes), np.float32).reshape(H, W, 4)
            ctx.buffer_free(out)
            dev.free()
        assert np.array_equal(blk.view(np.uint32), ref[want].view(np.uint32)), (y_first, rows, stripe, period)
        assert np.array_equal(wire[want].view(np.uint32), ref[want].view(np.uint32))
        other = np.setdiff1d(np.arange(H), want)
        assert (wire[other] == -7.0).all()


@pytest.mark.parametrize("kernel", [wcpt.KERNEL_MEGAKERNEL, wcpt.KERNEL_WAVEFRONT])
def test_context_screen_transitions(gpu_ctx, kernel):
    """What a resize, a row range and row stripes do to the rows one context holds (csrc/screen_layout.h, on the device):
    after every step wcpt_readback accepts exactly width * rows * 16 bytes, and a render fills those rows with the rows
    of a whole-frame render of the same size, bit for bit (seeds are global)."""
    s = get_scene("cornell")
    W = 16
    ref = {H: _context_frames(s, W, H, (0,), kernel=kernel) for H in (12, 9, 8)}

    def holds(ctx, dev, H, want):
        """the context holds the frame rows `want` of the W x H frame"""
        ctx.render(s.scene_data(W, H, max_bounce=4, frame=0), *dev.addresses())
        ctx.sync()
        blk = ctx.readback(len(want))
        with pytest.raises(wcpt.WcptError):
            ctx.readback(len(want) + 1)
        assert np.array_equal(blk.view(np.uint32), ref[H][want].view(np.uint32)), (H, want)

    with wcpt.Context(0) as ctx:
        dev = wcpt.DeviceScene(ctx, s)
        ctx.set_kernel(kernel)
        ctx.create_screen(W, 12)
        holds(ctx, dev, 12, list(range(12)))
        ctx.set_row_range(4, 6)                  # 1: a block of rows 4..9 ...
        holds(ctx, dev, 12, list(range(4, 10)))
        ctx.resize(W, 8)                         # ... clipped to rows 4..7 by a frame of 8 rows
        holds(ctx, dev, 8, list(range(4, 8)))
        ctx.resize(W, 12)                        # (the block stays clipped)
        holds(ctx, dev, 12, list(range(4, 8)))
        ctx.set_row_stripes(0, 6, 2, 4)          # 2: stripes of 2 rows every 4 rows: rows 0,1, 4,5, 8,9 ...
        holds(ctx, dev, 12, [0, 1, 4, 5, 8, 9])
        ctx.resize(W, 9)                         # ... whose last row a frame of 9 rows cuts off: the whole frame again
        holds(ctx, dev, 9, list(range(9)))
        dev.free()
    with wcpt.Context(0) as ctx:
        dev = wcpt.DeviceScene(ctx, s)
        ctx.set_kernel(kernel)
        ctx.set_row_range(7, 3)                  # 3: a range before the first screen is honoured by it
        ctx.create_screen(W, 12)
        holds(ctx, dev, 12, [7, 8, 9])
        ctx.set_row_range(0, 0)                  # 4: rows = 0 restores the whole frame
        holds(ctx, dev, 12, list(range(12)))
        dev.free()
    del s


def test_row_stripe_errors(gpu_ctx):
    s = get_scene("cornell")
    with wcpt.Context(0) as ctx:
        ctx.create_screen(16, 20)
        for args in ((0, 4, 3, 8), (0, 4, 8, 4), (0, 0, 8, 16), (8, 9, 8, 16)):   # not a power of two; period < stripe;
            with pytest.raises(wcpt.WcptError):                               # no rows; past the frame (row 23)
                ctx.set_row_stripes(*args)
        ctx.set_row_stripes(4, 8, 4, 8)
        ctx.create_screen(16, 12)        # rows 4..7 and 12..15: the new frame cannot hold them -> the whole frame again
        assert ctx.readback().shape[0] == 12
    with wcpt.Group([0] * 3, root=0, transport=COPY) as g:
        for v in (-1, 3, 65536):
            with pytest.raises(wcpt.WcptError):
                g.set_option(wcpt._lib.GROUP_OPTION_ROW_STRIPE, v)
        g.set_option(wcpt._lib.GROUP_OPTION_ROW_STRIPE, 8)
        with pytest.raises(wcpt.WcptError):
            g.create_screen(16, 16)      # two stripes of 8 rows for three ranks
        g.create_screen(16, 17)          # three stripes: ranks hold 8, 8 and 1 rows
        assert [c.height for c in g.contexts] == [8, 8, 1]
        assert g.info()["broken"] == 0
    del s


# ---- the one-process-per-GPU RCCL path, spawned by bench.py, and its bounded sync (round 6) ------------------------------
def _run(cmd, timeout):
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable] + cmd, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                          env=env, capture_output=True, text=True, timeout=timeout)


def test_spawned_rccl_ranks_present_the_one_device_frame(gpu_ctx):
    """`python bench.py --gpus 2 --rccl-rehearsal --verify` with no launcher: bench.py spawns two rank processes, each
    runs wcpt_group_create_rank (ncclCommInitRank) and the planned ncclSend / ncclRecv of every frame over RCCL's socket
    transport (a NCCL_HOSTID per rank lets two ranks share the one GPU), with interleaved 8-row stripes (the root's
    staging buffer and 2D scatter); the presented frame equals one device's render bit for bit."""
    import json
    p = _run(["bench.py", "--gpus", "2", "--config", "c1", "--rccl-rehearsal", "--row-stripe", "8", "--verify",
              "--steps", "6", "--warmup", "2", "--settle-ms", "0", "--no-cpu-baseline", "--watchdog-s", "100"], 150)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["verified"] is True and d["ranks"] == 2 and d["group"]["rccl_ranks"] == 2
    assert d["launch"].startswith("spawned by bench.py")


def test_group_sync_returns_device_lost_when_a_peer_skips_a_frame(gpu_ctx):
    """VERDICT r05 item 2 on the GPU (tools/group_fault_probe.py): rank 1 skips one frame's wcpt_group_render, so the
    root's receive never completes; its wcpt_group_sync returns WCPT_ERROR_DEVICE_LOST at the 2-s
    WCPT_GROUP_OPTION_TIMEOUT_MS (communicator aborted, the next render refused) instead of hanging, and both processes
    destroy their groups and exit."""
    import json
    p = _run(["tools/group_fault_probe.py", "--ranks", "2", "--timeout-ms", "2000"], 150)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["ok"] and all(d["checks"].values()), d["checks"]
    assert d["per_rank"][0]["sync_frame_3"]["rc"] == "WCPT_ERROR_DEVICE_LOST"


def test_bench_dump_outputs_is_the_last_timed_frame(gpu_ctx, tmp_path):
    """`python bench.py --gpus 1 --dump-outputs DIR`, a plain run: DIR/frame.npy is the frame after the last timed step
    (c1: progressive frames 0..warmup+steps-1 of the Cornell box), bit for bit a context's render of the same frames;
    the line holds the headline figure and none of what --full adds."""
    import json
    p = _run(["bench.py", "--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "2", "--settle-ms", "50",
              "--dump-outputs", str(tmp_path / "out")], 120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["full"] is False and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"kernel_ms_avg", "roofline", "cpu_baseline"} & set(d)
    frame = np.load(tmp_path / "out" / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (256, 256, 4)
    ref = _context_frames(get_scene("cornell"), 256, 256, range(5), bounces=1)
    codes = np.load(tmp_path / "out" / "frame_nonfinite.npy")
    assert np.isfinite(frame).all() and codes.shape == (256, 256)
    assert np.array_equal(codes != 0, ~np.isfinite(ref).all(axis=2)) and d["dumped"]["nonfinite_pixels"] == (codes != 0).sum()
    assert np.array_equal(frame.view(np.uint32), np.where(np.isfinite(ref), ref, np.float32(0)).view(np.uint32))
