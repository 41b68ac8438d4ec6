"""Where every byte of a group's presented frame goes (CPU): the layout wcpt_group.hip addresses a frame by
(wc-path-tracer_amd/csrc/group_layout.h, compiled here with g++ from the product header) against an independent model
of row ownership:

- with row blocks, frame row y belongs to rank r when r*H//n <= y < (r+1)*H//n;
- with stripes of S rows, to rank (y // S) % n.

For every shape {ranks, root, transport, stripe, size, format} the ranks' writes -- a frame writer's gather window, a
sender's landing range or the destination of its stripe copy -- cover every byte of the frame exactly once, each byte
by the rank that owns its row; a sender's stripe copy reads its payload once, in order; the root's staging ranges are
the senders' blocks back to back. That agreement is what makes the union of the ranks' rows the one-device frame.
"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RCCL, COPY, DIRECT = 0, 1, 2                       # wcpt.h WCPT_GROUP_TRANSPORT_*
RGB32F, RGBA32F, DISPLAY_RGBA8 = 3, 4, 8           # wcpt.h WCPT_PAYLOAD_*
PX = {RGB32F: 12, RGBA32F: 16, DISPLAY_RGBA8: 4}
OK, FRAME_TOO_SHORT, TOO_FEW_STRIPES, OUTPUT_TOO_SMALL, MISALIGNED = range(5)
FIELDS = ("y0", "rows", "bytes", "frame_off", "writes_frame", "whole_frame", "stage_off", "dst_off", "dst_pitch",
          "src_pitch", "span", "count", "tail_dst_off", "tail_src_off", "tail_bytes")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("layout") / "libgroup_layout_shim.so"
    src = os.path.join(ROOT, "tests", "group_layout_shim.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    u32, u64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.pixel_bytes.argtypes, lib.pixel_bytes.restype = [u32], u64
    lib.format_valid.argtypes = [u32]
    lib.screen_refusal.argtypes = [i32, u32, u32, u32]
    lib.output_refusal.argtypes = [u32, u32, u32, u64, u64]
    lib.lay_out.argtypes = [i32, i32, i32, u32, u32, u32, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.lay_out.restype = None
    lib.timeout_ms.argtypes, lib.timeout_ms.restype = [i32, i32], ctypes.c_double
    lib.drain_ms.argtypes, lib.drain_ms.restype = [ctypes.c_double], ctypes.c_double
    lib.issue_threads.argtypes = [i32, i32, i32, i32]
    return lib


def lay_out(shim, n, root, transport, stripe, W, H, fmt):
    head = (ctypes.c_uint64 * 2)()
    out = (ctypes.c_uint64 * (len(FIELDS) * n))()
    shim.lay_out(n, root, transport, stripe, W, H, fmt, head, out)
    k = len(FIELDS)
    return head[0], head[1], [dict(zip(FIELDS, out[k * r:k * r + k])) for r in range(n)]


def owned_rows(H, n, stripe):
    """The model: the frame rows of each rank, ascending."""
    rows = [[] for _ in range(n)]
    for y in range(H):
        if stripe:
            rows[(y // stripe) % n].append(y)
        else:
            rows[next(r for r in range(n) if r * H // n <= y < (r + 1) * H // n)].append(y)
    return rows


def copy_chunks(e):
    """(source offset, destination offset, bytes) of a stripe copy's pieces, in source order."""
    chunks = [(k * e["src_pitch"], e["dst_off"] + k * e["dst_pitch"], e["span"]) for k in range(e["count"])]
    if e["tail_bytes"]:
        chunks.append((e["tail_src_off"], e["tail_dst_off"], e["tail_bytes"]))
    return chunks


def check_shape(shim, n, root, transport, stripe, W, H, fmt, rows):
    row = W * PX[fmt]
    frame_bytes, stage_bytes, ranks = lay_out(shim, n, root, transport, stripe, W, H, fmt)
    where = (n, root, transport, stripe, W, H, fmt)
    owner = {y: r for r in range(n) for y in rows[r]}
    assert frame_bytes == row * H, where
    writes = []                                   # (first byte, end, rank) of every write into the frame
    stage = []
    for r, e in enumerate(ranks):
        mine = rows[r]
        assert (e["y0"], e["rows"]) == (mine[0], len(mine)), where
        assert e["bytes"] == len(mine) * row and e["frame_off"] == mine[0] * row, where
        assert bool(e["writes_frame"]) == (r == root or transport == DIRECT), where
        assert bool(e["whole_frame"]) == (bool(e["writes_frame"]) and stripe != 0), where
        if e["writes_frame"]:
            if e["whole_frame"]:
                # the render addresses the whole frame by frame row: local row ly of the rank's y0 / stripe / period
                # (row_map.h) is frame row y0 + (ly // S) * n * S + ly % S
                for ly in range(e["rows"]):
                    y = e["y0"] + (ly // stripe) * n * stripe + ly % stripe
                    writes.append((y * row, (y + 1) * row, r))
            else:
                writes.append((e["frame_off"], e["frame_off"] + e["bytes"], r))
            continue
        # a sender: its payload holds its rows back to back
        if stripe:
            src_at, dst_rows = 0, []
            for src, dst, nbytes in copy_chunks(e):
                assert src == src_at and nbytes % row == 0 and dst % row == 0, where   # read once, in order
                src_at += nbytes
                writes.append((dst, dst + nbytes, r))
                dst_rows += range(dst // row, (dst + nbytes) // row)
            assert src_at == e["bytes"], where
            assert dst_rows == mine, where        # payload row j lands at the rank's j-th frame row
        else:
            writes.append((e["frame_off"], e["frame_off"] + e["bytes"], r))
        if stage_bytes:
            stage.append((e["stage_off"], e["stage_off"] + e["bytes"]))
    # frame coverage: the writes tile [0, frame_bytes), and each byte's writer owns its row
    at = 0
    for a, b, r in sorted(writes):
        assert a == at and b > a, where
        assert all(owner[y] == r for y in range(a // row, (b + row - 1) // row)), where
        at = b
    assert at == frame_bytes, where
    # staging: the senders' blocks in rank order, back to back
    assert (stage_bytes == 0) == (transport != RCCL or stripe == 0 or n == 1), where
    at = 0
    for a, b in stage:
        assert a == at, where
        at = b
    assert at == stage_bytes, where
    if stage_bytes:
        assert stage_bytes == frame_bytes - ranks[root]["bytes"], where


@pytest.mark.parametrize("stripe", [0, 1, 2, 8, 16])
def test_every_byte_of_the_frame_is_written_once_by_its_rows_owner(shim, stripe):
    W = 3
    shapes = 0
    for H in range(1, 71):
        for n in range(1, 10):
            stripes = -(-H // stripe) if stripe else n
            want = FRAME_TOO_SHORT if H < n else TOO_FEW_STRIPES if stripes < n else OK
            assert shim.screen_refusal(n, stripe, W, H) == want, (n, stripe, H)
            if want != OK:
                continue
            rows = owned_rows(H, n, stripe)
            assert all(rows)                       # an accepted shape leaves no rank without a row
            for root in range(n):
                for transport in (RCCL, COPY, DIRECT):
                    for fmt in (RGB32F, RGBA32F, DISPLAY_RGBA8):
                        check_shape(shim, n, root, transport, stripe, W, H, fmt, rows)
                        shapes += 1
    assert shapes > 3000                           # stripes of 16 rows admit the fewest shapes: 3690
    assert shim.screen_refusal(3, stripe, 0, 30) == FRAME_TOO_SHORT   # no width


def test_formats_and_output_refusals(shim):
    for fmt in range(0, 20):
        assert bool(shim.format_valid(fmt)) == (fmt in PX)
    for fmt, px in PX.items():
        assert shim.pixel_bytes(fmt) == px
        assert shim.output_refusal(7, 5, fmt, 0, 35 * px) == OK
        assert shim.output_refusal(7, 5, fmt, 0, 35 * px - 1) == OUTPUT_TOO_SMALL
        assert shim.output_refusal(7, 5, fmt, 0x1002, 35 * px) == MISALIGNED          # 4 bytes for every format
        assert shim.output_refusal(7, 5, fmt, 0x1004, 35 * px) == (MISALIGNED if fmt == RGBA32F else OK)
        assert shim.output_refusal(7, 5, fmt, 0x1010, 35 * px) == OK
        assert shim.output_refusal(0, 0, fmt, 0x1010, 0) == OK                        # no screen yet: any size holds it
    assert shim.pixel_bytes(0) == 0                                                   # not presenting: no bytes
    # too small wins over misaligned: every process sees the size, only the root's the address
    assert shim.output_refusal(7, 5, RGBA32F, 0x1004, 16) == OUTPUT_TOO_SMALL


def test_arithmetic_is_64_bit(shim):
    W = H = 65536
    assert shim.output_refusal(W, H, RGBA32F, 0, 1 << 36) == OK
    assert shim.output_refusal(W, H, RGBA32F, 0, (1 << 36) - 1) == OUTPUT_TOO_SMALL
    row = W * 16
    for stripe in (0, 16):
        for transport in (RCCL, COPY):
            frame_bytes, stage_bytes, ranks = lay_out(shim, 3, 1, transport, stripe, W, H, RGBA32F)
            assert frame_bytes == 1 << 36
            rows = owned_rows(H, 3, stripe)
            for r, e in enumerate(ranks):
                assert e["bytes"] == len(rows[r]) * row and e["frame_off"] == rows[r][0] * row
                if stripe:
                    chunks = copy_chunks(e)
                    assert sum(c[2] for c in chunks) == e["bytes"]
                    assert chunks[-1][1] == rows[r][-1] // 16 * 16 * row           # its last stripe, beyond 2^32
                    assert chunks[-1][1] > 1 << 35
            if not stripe:
                assert ranks[2]["frame_off"] == (2 * H // 3) * row > 1 << 32
            if stripe and transport == RCCL:
                assert stage_bytes == ranks[0]["bytes"] + ranks[2]["bytes"] > 1 << 35
                assert ranks[2]["stage_off"] == ranks[0]["bytes"] > 1 << 32
            else:
                assert stage_bytes == 0


def test_timeout_and_issue_thread_decisions(shim):
    # WCPT_GROUP_OPTION_TIMEOUT_MS: -1 = 60 s in a group of several ranks and none in a group of one; 0 = none
    for nranks in (1, 2, 8):
        assert shim.timeout_ms(-1, nranks) == (60000.0 if nranks > 1 else 0.0)
        for option in (0, 1, 250, 9999, 10000, 60000, 3600000):
            assert shim.timeout_ms(option, nranks) == float(option)
    # the drain after an abort: the timeout, 10 s at most, and 10 s when there is none
    for t, want in ((0.0, 10000.0), (1.0, 1.0), (250.0, 250.0), (9999.0, 9999.0), (10000.0, 10000.0),
                    (60000.0, 10000.0)):
        assert shim.drain_ms(t) == want
    # WCPT_GROUP_OPTION_THREADS: 0 off, 1 on, -1 on for COPY / DIRECT ranks on more than one device
    for local in (1, 2, 3, 8):
        for transport in (RCCL, COPY, DIRECT):
            for spans in (0, 1):
                assert shim.issue_threads(0, local, transport, spans) == 0
                assert shim.issue_threads(1, local, transport, spans) == (1 if local > 1 else 0)
                assert shim.issue_threads(-1, local, transport, spans) == \
                    (1 if local > 1 and transport != RCCL and spans else 0)
