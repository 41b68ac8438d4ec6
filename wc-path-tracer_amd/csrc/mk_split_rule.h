/* mk_split_rule.h — when a megakernel render runs as two launches (WCPT_OPTION_MK_SPLIT), where it is cut, and how the
 * queue between them is laid out. Plain C++, no HIP call (the kernels share the sub-queue arithmetic at the end):
 * tests/mk_split_rule_shim.cpp compiles it with g++.
 *
 * A wave of the megakernel keeps issuing a segment's whole traversal while one of its 64 paths is alive, and in an open
 * scene paths end segment by segment (the Cornell box at 1080p: 1.00 / 0.64 / 0.58 / 0.52 / 0.46 of the pixels reach
 * segments 0..4, while the waves that still have a path stay 21060 / 20887 / 20884 / 20882 of 32400: the lanes of a live
 * wave are 99 / 89 / 80 / 72 % filled at segments 1..4). A split render cuts the segment loop once, at a launch boundary:
 * the head launch is the kernel up to the cut and appends the surviving paths to a queue; the tail launch finishes them
 * one per lane in full waves (pt_device.h SplitQueue, pt_kernels.hip pt_mk_tail). Same arithmetic per path, so the
 * image is the unsplit render's bit for bit.
 *
 * Measured before building (c2 = Cornell 1080p, 1 spp, still camera, primary cache on; 400 frames x 3 rounds): 0.0899 /
 * 0.1542 / 0.2224 / 0.2894 ms per frame at maxBounceCount 1 / 2 / 3 / 4, so segments 3-4 cost 0.135 ms, of which the
 * share (1 - survivors / (64 x live waves)) = 0.240 is the ceiling of a cut before segment 3: 0.0325 ms, 11 % of the
 * frame (attrition inside the tail leaves about 0.0265 ms; the same sum gives 0.021 ms for a cut before 2 and 0.019 ms
 * before 4).
 *
 * Measured after (same frames, region-timed, 300 frames x 3 interleaved rounds, ms per frame; every image bit-identical
 * to the unsplit one):
 *
 *   rows of 1920 (rounds of waves)   unsplit   cut 1    cut 2    cut 3    cut 4
 *   1080 (7.9)                       0.2889    0.3064   0.2817   0.2782   0.2889
 *    540 (4.0)                       0.1466    0.1604   0.1468   0.1431   0.1731
 *    270 (2.0)                       0.0768    0.0901   0.0904   0.0822   0.0971
 *    135 (1.0)                       0.0591    0.0648   0.0649   0.0655   0.0654
 *
 * A cut before segment 3 is the best everywhere it pays: -3.7 % on the frame, -2.4 % on its half, and a loss on the
 * 4- and 8-way blocks, where a second launch per pipe costs more rounds' ends than the fuller waves save. The automatic
 * rule therefore cuts before segment 3 from 3 rounds of resident waves up (between the two measured sizes on either
 * side). Less than the 9 % estimated: VALU wave-instructions per frame fall by 6.1 % (lane utilisation 0.808 -> 0.869;
 * paths still end inside the tail, and both launches carry their own prologue), the time by 3.7-3.9 %, because each of the
 * frame's four launches now ends in a last round of its own (profiles/mk_split_sq.log).
 *
 * The reference's scene (the mushroom mesh, camera inside its box) loses at every cut and bounce count, although its
 * live waves are emptier (lane fill 0.77 / 0.67 / 0.63 at segments 2..4): 0.9147 ms unsplit against 1.0894 / 1.1926 /
 * 0.9657 at cuts 1..3 of 3 bounces, 1.4001 against 1.5222 at cut 3 of 4. A tail wave holds paths of unrelated tiles,
 * and on a mesh of many leaves the lanes of such a wave walk different nodes, where the tile's own wave walked mostly
 * the same ones; the Cornell box's 34 triangles are two or three leaves that every ray tests, whichever wave it sits in
 * (its gain grows with the bounces: -9.5 % at 6). The automatic rule therefore splits only scenes of at most
 * kMkSplitAutoMaxTriangles triangles -- four leaves of the reference's builder; nothing between 34 triangles and the
 * mushroom has been measured -- and leaves every larger mesh whole. A forced cut ignores this.
 */
#ifndef WCPT_MK_SPLIT_RULE_H
#define WCPT_MK_SPLIT_RULE_H

#include <stdint.h>

#ifdef __HIPCC__
#define WCPT_MK_SPLIT_HD __host__ __device__
#else
#define WCPT_MK_SPLIT_HD
#endif

namespace wcpt {

constexpr int kMkSplitAuto = -1;            /* WCPT_OPTION_MK_SPLIT's default */
constexpr int kMkSplitMaxCut = 15;          /* the option's largest value */
constexpr uint32_t kMkSplitAutoCut = 3;     /* the automatic rule's cut (table above) */
constexpr uint32_t kMkSplitEntryBytes = 56; /* a queue entry: 14 u32 (pt_device.h kSplitWords) */
/* the automatic rule wants at least this many rounds of resident waves in the render, in halves (6 = 3 rounds) */
constexpr uint32_t kMkSplitAutoMinHalfRounds = 6;
/* ... and at most this many triangles in all draw commands (above: the tail's waves mix unrelated tiles) */
constexpr uint64_t kMkSplitAutoMaxTriangles = 64;

/* The cut of one render: 0 = one launch (the whole kernel), k >= 1 = the head stops before segment k.
 * option: WCPT_OPTION_MK_SPLIT (-1 automatic, 0 never, k forced). splittable: a render (not a counting or diagnostics
 * run) on the LDS stack -- the builds that have a head and a tail. waves: the render's 64-lane waves (its tiles, both
 * pipes together); wave_slots: the waves the device holds at once (4 per SIMD at the kernel's registers); triangles: of
 * all draw commands.
 * Off for samples > 1 (those builds share the primary segment between the samples and stay whole) and where no segment
 * follows the cut: segments are 0..maxBounceCount, so a cut never exceeds maxBounceCount (and never splits
 * maxBounceCount 0); the automatic rule is also off for maxBounceCount < 2, for renders of under 3 rounds of waves and
 * for meshes of more than kMkSplitAutoMaxTriangles triangles, and lowers its cut to maxBounceCount. */
inline uint32_t mk_split_cut(int option, bool splittable, uint32_t samples, uint32_t maxBounceCount, uint64_t waves,
                             uint64_t wave_slots, uint64_t triangles)
{
    if (option == 0 || !splittable || samples != 1u || maxBounceCount == 0u || waves == 0u) return 0u;
    if (option > 0) return (uint32_t)option <= maxBounceCount ? (uint32_t)option : 0u;
    if (maxBounceCount < 2u || triangles > kMkSplitAutoMaxTriangles) return 0u;
    if (2u * waves < (uint64_t)kMkSplitAutoMinHalfRounds * wave_slots) return 0u;
    return kMkSplitAutoCut <= maxBounceCount ? kMkSplitAutoCut : maxBounceCount;
}

/* The queues of one render of `tiles` 8x8 tiles: an unpiped render has one launch (pipe 0) of all tiles; the frame
 * overlap's pipes take (tiles + 1) / 2 and the rest (launch_megakernel). A launch's queue holds one entry per lane of
 * its waves -- its pixels, when the frame's width and rows are whole tiles -- so an append cannot pass it, and the
 * queues of both pipes lie back to back in one allocation of 64 x tiles entries, sized for the frame. */
struct MkSplitLayout {
    uint32_t cap[2];    /* entries of pipe p's queue (0: no such launch) */
    uint64_t first[2];  /* pipe p's first entry in the allocation; its arrays follow each other from 14 x first[p] u32 */
    uint64_t entries;   /* of the allocation */
};
inline MkSplitLayout mk_split_layout(uint32_t tiles, bool piped)
{
    MkSplitLayout l;
    const uint32_t half = (tiles + 1u) / 2u;
    l.cap[0] = 64u * (piped ? half : tiles);
    l.cap[1] = piped ? 64u * (tiles - half) : 0u;
    l.first[0] = 0u;
    l.first[1] = piped ? (uint64_t)l.cap[0] : 0u;
    l.entries = 64ull * tiles;
    return l;
}

/* Inside a launch's queue. Every live wave of the head appends once, and atomics on one address serialise (about 34 ns
 * each when they arrive together: 21,000 waves of a 1080p frame would spend 0.7 ms on one counter), so a queue is
 * kMkSplitSubQueues sub-queues with a counter each, kMkSplitCounterStride u32 apart: head block b appends to sub-queue
 * b mod kMkSplitSubQueues, whose share of the queue is 64 entries per such block, the shares back to back in order of
 * j; tail block b finishes entries [64 c, 64 c + 64) of sub-queue b mod kMkSplitSubQueues, c = b / kMkSplitSubQueues.
 * Head and tail have the same grid (cap / 64 blocks), so the tail's blocks cover every sub-queue's share exactly. */
constexpr uint32_t kMkSplitSubQueues = 64;
constexpr uint32_t kMkSplitCounterStride = 64;
/* u32 of one counter set (a pipe has two: this frame's and the next's) */
constexpr uint32_t kMkSplitCounterWords = kMkSplitSubQueues * kMkSplitCounterStride;
/* sub-queue j of a queue of `blocks` x 64 entries: its first entry and its entries */
WCPT_MK_SPLIT_HD inline uint32_t mk_split_sub_first(uint32_t blocks, uint32_t j)
{
    const uint32_t q = blocks / kMkSplitSubQueues, r = blocks % kMkSplitSubQueues;
    return 64u * (j * q + (j < r ? j : r));
}
WCPT_MK_SPLIT_HD inline uint32_t mk_split_sub_cap(uint32_t blocks, uint32_t j)
{
    return 64u * (blocks / kMkSplitSubQueues + (j < blocks % kMkSplitSubQueues ? 1u : 0u));
}

} // namespace wcpt

#undef WCPT_MK_SPLIT_HD
#endif
