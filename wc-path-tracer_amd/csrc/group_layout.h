/*
 * group_layout.h — where every byte of a wcpt_group's presented frame goes, as functions of plain values. Pure C++17, no
 * HIP or RCCL type: wcpt_group.hip and tests/group_layout_shim.cpp (g++) evaluate the same functions, and
 * tests/test_group_layout.py checks them against a model of row ownership: for every shape the writers cover each byte
 * of the frame exactly once. group_plan.h says in which order a frame's operations are issued; this header says what
 * each of them addresses.
 *
 * A shape is {nranks, root, transport, stripe, width, height, format}. Rank r holds a contiguous block of rows or
 * (stripe != 0) interleaved stripes (screen_layout.h split_row_block, split_row_stripes); a rank either renders straight
 * into the frame on the root's device (the root; every rank with the DIRECT transport) or renders into a payload of its
 * rows back to back and sends it. A sender's payload lands at its block's place in the frame (blocks), or (stripes) its
 * stripes are copied to their rows: from the payload itself (COPY) or from the root's staging buffer, where RCCL
 * received it. All byte arithmetic is 64-bit.
 */
#ifndef WCPT_GROUP_LAYOUT_H
#define WCPT_GROUP_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "group_plan.h"
#include "screen_layout.h"

namespace wcpt {
namespace glayout {

struct Shape {
    int nranks = 0, root = 0, transport = plan::kRccl;
    uint32_t stripe = 0;            /* rows per interleaved stripe, 0 = contiguous row blocks */
    uint32_t width = 0, height = 0;
    uint32_t format = 0;            /* WCPT_PAYLOAD_*; 0 = not presenting: every byte count below is 0 */
};

/* A rank's rows, back to back at a source, to their rows of the frame (stripe != 0): one 2D copy of its `count` whole
 * stripes (`span` bytes each; pitch nranks * stripe rows in the frame, stripe rows at the source) and one copy of its
 * short last stripe, if it holds one. dst offsets are from the frame's first byte, src offsets from the block's. */
struct StripeCopy {
    uint64_t dst_off = 0, dst_pitch = 0, src_pitch = 0, span = 0, count = 0;
    uint64_t tail_dst_off = 0, tail_src_off = 0, tail_bytes = 0;
};

struct RankLayout {
    uint32_t y0 = 0, rows = 0;     /* first row (of its first stripe) and row count */
    uint64_t bytes = 0;            /* of its rows: a sender's payload, a block writer's gather window */
    uint64_t frame_off = 0;        /* byte offset of row y0 in the frame */
    bool writes_frame = false;     /* renders into the frame; otherwise it sends a payload of `bytes` bytes */
    bool whole_frame = false;      /* a frame writer with stripes: its gather output is the whole frame, addressed by
                                    * frame row (WCPT_OPTION_GATHER_FRAME_ROWS 1); else the window [frame_off, +bytes) */
    uint64_t stage_off = 0;        /* a sender's block in the root's staging buffer (stage_bytes != 0) */
    StripeCopy copy;               /* stripe != 0 */
};

struct Layout {
    uint64_t frame_bytes = 0;
    uint64_t stage_bytes = 0;      /* the root's staging buffer: RCCL with stripes and more than one rank, else 0 */
    std::vector<RankLayout> rank;  /* all nranks, whichever process holds them */
};

inline uint64_t frame_bytes(uint32_t width, uint32_t height, uint32_t format)
{
    return (uint64_t)width * height * payload_pixel_bytes(format);
}

/* The shape's layout. The shape has passed screen_refusal (every rank holds at least one row). */
inline void lay_out(const Shape& s, Layout& out)
{
    const uint64_t row = (uint64_t)s.width * payload_pixel_bytes(s.format);
    const bool staged = s.transport == plan::kRccl && s.stripe && s.nranks > 1;
    out.frame_bytes = row * s.height;
    out.stage_bytes = 0;
    out.rank.assign((size_t)s.nranks, RankLayout());
    for (int r = 0; r < s.nranks; r++) {
        RankLayout& k = out.rank[(size_t)r];
        if (s.stripe)
            split_row_stripes(s.height, (uint32_t)s.nranks, (uint32_t)r, s.stripe, k.y0, k.rows);
        else
            split_row_block(s.height, (uint32_t)s.nranks, (uint32_t)r, k.y0, k.rows);
        k.bytes = row * k.rows;
        k.frame_off = row * k.y0;
        k.writes_frame = r == s.root || s.transport == plan::kDirect;
        k.whole_frame = k.writes_frame && s.stripe;
        if (s.stripe) {
            const uint64_t S = s.stripe, P = S * (uint64_t)s.nranks, full = k.rows / S, tail = k.rows % S;
            k.copy = {k.frame_off, P * row, S * row, S * row, full, k.frame_off + full * P * row, full * S * row, tail * row};
        }
        if (staged && !k.writes_frame) { /* the senders' blocks in rank order, back to back */
            k.stage_off = out.stage_bytes;
            out.stage_bytes += k.bytes;
        }
    }
}

/* ---- refusals that every process of a group makes alike (they read only what every process is given) --------------- */

enum Refusal {
    kOk = 0,
    kFrameTooShort,   /* no width, or fewer rows than ranks */
    kTooFewStripes,   /* fewer stripes than ranks: a rank would hold no row */
    kOutputTooSmall,  /* the output does not hold the frame in its format */
    kMisaligned,      /* destination: 4 bytes, 16 for RGBA32F (the root's process alone sees it) */
};

inline Refusal screen_refusal(int nranks, uint32_t stripe, uint32_t width, uint32_t height)
{
    if (width == 0 || height < (uint32_t)nranks) return kFrameTooShort;
    if (stripe && ((uint64_t)height + stripe - 1u) / stripe < (uint64_t)nranks) return kTooFewStripes;
    return kOk;
}

inline Refusal output_refusal(uint32_t width, uint32_t height, uint32_t format, uint64_t dst, uint64_t bytes)
{
    if (frame_bytes(width, height, format) > bytes) return kOutputTooSmall;
    if ((dst & 3u) || (format == kPayloadRgba32f && (dst & 15u))) return kMisaligned;
    return kOk;
}

/* ---- two decisions of the group's options --------------------------------------------------------------------------- */

/* The default bound on one wcpt_group_sync of a group of several ranks. An editor loop syncs every frame (main.jai:73-95);
 * bench.py syncs after at most a few hundred frames (c4 at 8 ranks: ~45 ms each). */
constexpr int kDefaultTimeoutMs = 60000;
/* After the communicators were aborted the streams get the group's timeout to drain; this at most, and with no timeout */
constexpr double kDrainMs = 10000.0;

/* WCPT_GROUP_OPTION_TIMEOUT_MS: -1 (default) = kDefaultTimeoutMs in a group of several ranks, none in a group of one;
 * 0 = none (wait forever) */
inline double timeout_ms(int option, int nranks)
{
    if (option >= 0) return (double)option;
    return nranks > 1 ? (double)kDefaultTimeoutMs : 0.0;
}

inline double drain_ms(double timeout) { return timeout > 0.0 && timeout < kDrainMs ? timeout : kDrainMs; }

/* WCPT_GROUP_OPTION_THREADS: 0 off, 1 on, -1 on when this process's ranks span more than one device with COPY or DIRECT.
 * A one-process RCCL group keeps the single-thread form (every frame's sends and receives in one
 * ncclGroupStart/End, rccl.h:700,722) unless threads are asked for: its thread-per-device form is RCCL's other
 * supported pattern, but no multi-GPU box here has run it. */
inline bool issue_threads(int option, size_t local_ranks, int transport, bool spans_devices)
{
    if (local_ranks < 2 || option == 0) return false;
    if (option == 1) return true;
    return transport != plan::kRccl && spans_devices;
}

} // namespace glayout
} // namespace wcpt

#endif
