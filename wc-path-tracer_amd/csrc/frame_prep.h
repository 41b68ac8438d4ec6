/* frame_prep.h — the per-draw record table that frame preparation (wcpt_runtime.hip prepare_tri_records) writes and the
 * kernels read (pt_device.h, pt_wavefront.hip), declared once for both sides, and everything frame preparation decides,
 * as functions of plain values. Plain C++17, no HIP call: the runtime, the kernels and tests/frame_prep_shim.cpp (g++)
 * see the same constants and evaluate the same functions.
 *
 * Table entry of one draw command, kTriTableWords x u64:
 *   word 0  address of the single records (48 B per triangle)
 *   word 1  address of the pair records (80 B per triangle pair)
 *   word 2  triangle count; bits 32..63: the BVH's node count when kTriFlagPackedRefs is set (the buffer-resource node
 *           loads of pt_device.h load_pair_rsrc cover exactly those nodes), else 0
 *   word 3  kTriFlag* bits; bits 32..63: vertices in the draw's vertex buffer (0xFFFFFFFF: unknown)
 *   word 4  address of the primary-ray pair records (112 B per pair) or 0
 */
#ifndef WCPT_FRAME_PREP_H
#define WCPT_FRAME_PREP_H

#include <stdint.h>

#include "../../include/wcpt.h"
#include "mk_tiny_rule.h"

namespace wcpt {

/* ---- the contract ----------------------------------------------------------------------------------------------- */
constexpr uint32_t kTriTableWords = 5;
constexpr uint32_t kTriWordSingles = 0, kTriWordPairs = 1, kTriWordCount = 2, kTriWordFlags = 3, kTriWordPrimary = 4;
constexpr uint64_t kTriFlagPackedRefs = 1u; /* table word 3: stack entries may carry (left, count) */
constexpr uint64_t kTriFlagIndex24 = 2u;    /* table word 3: the draw's indexCount is < 2^24 */
constexpr uint64_t kTriFlagSmallLeaves = 4u; /* table word 3: every node's triangleCount is < kRefFetch, so every packed
                                                stack entry carries its node's (left, count) */
constexpr uint64_t kTriFlagLeafRecords = 8u; /* table word 3: every leaf starts at a triangle boundary and ends within the
                                                draw's derived records, so each leaf triangle at index position p is
                                                single record p / 3 (byte offset 16 p) */
constexpr uint64_t kTriFlagTinyTree = 16u;  /* table word 3: the BVH is a root leaf or a root over two leaves, each on
                                                derived records (mk_tiny_rule.h), and WCPT_OPTION_MK_TINY_TREE allows the
                                                walk without the traversal loop (pt_tiny.h tiny_walk) */
/* the wavefront trace's one-draw fast layout: packed stack refs, 24-bit record offsets, buffer-resource node loads */
constexpr uint64_t kTriFlagsFastLayout = kTriFlagPackedRefs | kTriFlagIndex24 | kTriFlagSmallLeaves | kTriFlagLeafRecords;

/* What the leaf scan (pt_kernels.hip scan_leaf_counts, scan_tiny_tree) reports of a draw's BVH */
constexpr uint32_t kLeafScanBigLeaf = 1u;    /* some leaf has triangleCount >= kRefFetch */
constexpr uint32_t kLeafScanOffRecords = 2u; /* some leaf starts off a triangle boundary or ends past the derived records */
constexpr uint32_t kLeafScanTinyTree = 4u;   /* the tree is tiny (mk_tiny_rule.h) */
/* before the scan has answered: no fast layout, no tiny tree */
constexpr uint32_t kLeafScanUnknown = kLeafScanBigLeaf | kLeafScanOffRecords;

/* Derived triangle records (pt_device.h): triangle k = index positions 3k..3k+2 stored as (a, b - a, c - a);
 * singles: 48 B per triangle; pairs: 80 B per triangle pair (2j, 2j+1). */
constexpr uint32_t kSingleRecordBytes = 48, kPairRecordBytes = 80;
/* primary-ray pair records (pt_device.h TriPairP), built with launch_build_primary_pairs */
constexpr uint32_t kPrimPairRecordBytes = 112;

/* Pair records (packed two-triangle tests) pay off when leaves are fat: mean triangles per leaf >= this,
 * estimated as triangles / leaves with leaves = (nodes + 1) / 2 from the BVH buffer's size. Measured: the
 * Cornell box (17 per leaf) gains, the atrium (~2 per leaf) loses. */
constexpr double kPairMinTrianglesPerLeaf = 4.0;
/* Largest triangle count of a draw whose pair records are used: 40 B per triangle must stay addressable with 32-bit
 * byte offsets (2^26 triangles = 2.5 GiB of pair records); larger draws use single records. */
constexpr uint64_t kPairMaxTriangles = 1ull << 26;

/* ---- the rules -------------------------------------------------------------------------------------------------- */

/* One allocation per draw: the single records, then (256-byte aligned) the pair records; the primary-ray records of
 * the pair records build_tri_records writes are an allocation of their own (prim_bytes: one copy of them). */
struct RecordLayout { uint64_t pair_offset, bytes, prim_pairs, prim_bytes; };
inline RecordLayout record_layout(uint32_t ntri)
{
    const uint64_t singles = ((uint64_t)ntri * kSingleRecordBytes + 255u) & ~255ull;
    const uint64_t npairs = ((uint64_t)ntri + 1u) / 2u;
    return {singles, singles + ((uint64_t)ntri / 2u + 1u) * kPairRecordBytes, npairs, npairs * kPrimPairRecordBytes};
}

/* Table word 3's high half: vertices (12 B) in the rest of the draw's vertex buffer; a buffer the context does not know
 * bounds nothing. A triangle with an index past the bound gets a NaN record, which no ray accepts. */
inline uint32_t vertex_bound(bool known, uint64_t bytes_left)
{
    if (!known) return 0xFFFFFFFFu;
    return bytes_left / 12ull < 0xFFFFFFFFull ? (uint32_t)(bytes_left / 12ull) : 0xFFFFFFFFu;
}

/* Nodes (32 B) from the draw's BVH address to the end of its buffer; unknown when the context does not know the buffer. */
constexpr uint64_t kNodesUnknown = ~0ull;
inline uint64_t bvh_node_count(bool known, uint64_t bytes_left) { return known ? bytes_left / sizeof(wcpt_node) : kNodesUnknown; }

/* The draw's share of the frame's leaf estimate (frame_plan): leaves = (nodes + 1) / 2 of a full binary tree, from the
 * size of the whole BVH buffer -- not from the bytes past the draw's offset, which bvh_node_count takes for the flags.
 * Deliberately kept: the pair rule's threshold was measured with this estimate. Unknown buffer: thin leaves. */
inline uint64_t leaf_estimate(bool known, uint64_t buffer_bytes, uint32_t ntri)
{
    return known ? (buffer_bytes / sizeof(wcpt_node) + 1u) / 2u : ntri;
}

/* Stack entries may carry the child's (left, count) when every node index and index position fits in 24 bits
 * (pt_device.h node_ref); unknown BVH size -> node-index entries.
 * kTriFlagSmallLeaves / LeafRecords / TinyTree come from a device scan, once per BVH buffer generation, which only the
 * triangle cache tracks; with the cache off the BVH may change behind the runtime on any frame, and a scan per render
 * would block the host, so the fast leaf layout is simply not used. */
inline bool draw_packed_refs(int packed_option, uint64_t nodes, uint32_t index_count)
{
    return packed_option && nodes < (1ull << 24) && index_count < (1u << 24);
}
inline bool draw_needs_scan(int packed_option, bool cache_on, uint64_t nodes, uint32_t index_count)
{
    return cache_on && draw_packed_refs(packed_option, nodes, index_count);
}

/* Table words 2 and 3 of a draw. scan_bits: the leaf scan's kLeafScan* (read only where draw_needs_scan);
 * tiny_option: WCPT_OPTION_MK_TINY_TREE; nvert: vertex_bound. */
struct DrawWords { uint64_t word2, flags; };
inline DrawWords draw_words(int packed_option, bool cache_on, uint64_t nodes, uint32_t index_count, uint32_t scan_bits,
                            int tiny_option, uint32_t nvert)
{
    const bool packed = draw_packed_refs(packed_option, nodes, index_count);
    uint64_t flags = packed ? kTriFlagPackedRefs : 0u;
    if (index_count < (1u << 24)) flags |= kTriFlagIndex24;
    if (packed && cache_on) {
        if (!(scan_bits & kLeafScanBigLeaf)) flags |= kTriFlagSmallLeaves;
        if (!(scan_bits & kLeafScanOffRecords)) flags |= kTriFlagLeafRecords;
        /* the scan's own rule (mk_tiny_rule.h), where the option allows the walk */
        if (mk_tiny_enabled(tiny_option, (scan_bits & kLeafScanTinyTree) ? 1u : 0u)) flags |= kTriFlagTinyTree;
    }
    return {(uint64_t)(index_count / 3u) | (packed ? nodes << 32 : 0ull), flags | (uint64_t)nvert << 32};
}

/* The record build reads indices [0, indexCount) of the draw: an index buffer known to the context must hold them (the
 * reference's kernel never reads indexCount, but the record build does). Vertex indices are checked against
 * vertex_bound on the device. */
enum DrawArgError { kDrawArgsOk = 0, kDrawIndexCountPastBuffer, kDrawNullBuffer };
inline DrawArgError check_draw_args(uint32_t index_count, uint64_t vertex_buffer, uint64_t index_buffer, bool ib_known,
                                    uint64_t ib_bytes_left)
{
    const uint32_t ntri = index_count / 3u;
    if (ib_known && (uint64_t)ntri * 12ull > ib_bytes_left) return kDrawIndexCountPastBuffer;
    if (ntri && (vertex_buffer == 0 || index_buffer == 0)) return kDrawNullBuffer;
    return kDrawArgsOk;
}

/* What a frame runs: the outcome of frame preparation, cached while nothing it read can have changed. */
struct FramePlan {
    bool pair_records = false; /* megakernel: leaf tests on pair records */
    bool wf_fast = false;      /* wavefront trace: draw 0 has the fast layout and a known node count */
    bool tiny_tree = false;    /* draw 0's kTriFlagTinyTree is set */
    uint64_t triangles = 0;    /* of all draws (the split rule's input, mk_split_rule.h) */
    int kernel_run = WCPT_KERNEL_MEGAKERNEL; /* WCPT_KERNEL_AUTO resolved */
    bool want_primary = false; /* primary-ray records: the megakernel with pair records */
};
/* n draws, draw 0's table words 2 and 3, the triangles of all draws and of the largest, the leaf estimates' sum,
 * WCPT_OPTION_PAIR_RECORDS (-1 auto, 0 singles, 1 pairs) and the kernel option. */
inline FramePlan frame_plan(uint32_t n, uint64_t word2_0, uint64_t flags_0, uint64_t tris_all, uint64_t leaves_all,
                            uint64_t tris_max, int pair_option, int kernel_option)
{
    FramePlan p;
    if (n != 0) {
        p.triangles = tris_all;
        p.wf_fast = n == 1 && (flags_0 & kTriFlagsFastLayout) == kTriFlagsFastLayout && (word2_0 >> 32) > 0;
        p.tiny_tree = n == 1 && (flags_0 & kTriFlagTinyTree) != 0u;
        /* pair leaves address a draw's pair records with 32-bit byte offsets (pt_device.h load_pair_at) */
        p.pair_records = tris_max <= kPairMaxTriangles &&
                         (pair_option == 1 ||
                          (pair_option < 0 && leaves_all > 0 && (double)tris_all >= kPairMinTrianglesPerLeaf * leaves_all));
    }
    /* WCPT_KERNEL_AUTO: the megakernel where leaves hold several triangles (its pair loops and scalar-cache leaves pay)
     * and where there is no draw, the wavefront kernel on thin leaves (Cornell 0.37 / mushroom 1.22 ms megakernel
     * against 2.0 ms wavefront on the mushroom; the atrium 4.8 ms wavefront against 9.8 ms megakernel); an explicit
     * choice stands */
    p.kernel_run = kernel_option != WCPT_KERNEL_AUTO ? kernel_option
                                                     : (p.pair_records || n == 0 ? WCPT_KERNEL_MEGAKERNEL : WCPT_KERNEL_WAVEFRONT);
    p.want_primary = p.pair_records && p.kernel_run == WCPT_KERNEL_MEGAKERNEL;
    return p;
}

} // namespace wcpt

#endif
