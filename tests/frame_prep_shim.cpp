// Test shim (CPU): exposes frame preparation's rules and the table contract (wc-path-tracer_amd/csrc/frame_prep.h, what
// the runtime evaluates per draw and per frame) to tests/test_frame_prep.py over ctypes. Built by the test with g++; no
// HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/frame_prep.h"

using namespace wcpt;

// the contract's constants, in the order tests/test_frame_prep.py names them
extern "C" void fp_constants(uint64_t* out)
{
    const uint64_t c[] = {kTriTableWords, kTriWordSingles, kTriWordPairs, kTriWordCount, kTriWordFlags, kTriWordPrimary,
                          kTriFlagPackedRefs, kTriFlagIndex24, kTriFlagSmallLeaves, kTriFlagLeafRecords, kTriFlagTinyTree,
                          kLeafScanBigLeaf, kLeafScanOffRecords, kLeafScanTinyTree, kSingleRecordBytes, kPairRecordBytes,
                          kPrimPairRecordBytes, kPairMaxTriangles, (uint64_t)kPairMinTrianglesPerLeaf, kNodesUnknown};
    for (uint64_t v : c) *out++ = v;
}

// out: pair_offset, bytes, prim_pairs, prim_bytes
extern "C" void fp_record_layout(uint32_t ntri, uint64_t* out)
{
    const RecordLayout l = record_layout(ntri);
    out[0] = l.pair_offset, out[1] = l.bytes, out[2] = l.prim_pairs, out[3] = l.prim_bytes;
}

extern "C" uint32_t fp_vertex_bound(int known, uint64_t bytes_left) { return vertex_bound(known != 0, bytes_left); }
extern "C" uint64_t fp_bvh_node_count(int known, uint64_t bytes_left) { return bvh_node_count(known != 0, bytes_left); }
extern "C" uint64_t fp_leaf_estimate(int known, uint64_t buffer_bytes, uint32_t ntri)
{
    return leaf_estimate(known != 0, buffer_bytes, ntri);
}
extern "C" int fp_needs_scan(int packed_option, int cache_on, uint64_t nodes, uint32_t index_count)
{
    return draw_needs_scan(packed_option, cache_on != 0, nodes, index_count) ? 1 : 0;
}

// out: word 2, word 3
extern "C" void fp_draw_words(int packed_option, int cache_on, uint64_t nodes, uint32_t index_count, uint32_t scan_bits,
                              int tiny_option, uint32_t nvert, uint64_t* out)
{
    const DrawWords w = draw_words(packed_option, cache_on != 0, nodes, index_count, scan_bits, tiny_option, nvert);
    out[0] = w.word2, out[1] = w.flags;
}

// 0 pass, 1 indexCount past the index buffer, 2 null buffer with triangles
extern "C" int fp_check_draw_args(uint32_t index_count, uint64_t vb, uint64_t ib, int ib_known, uint64_t ib_bytes_left)
{
    switch (check_draw_args(index_count, vb, ib, ib_known != 0, ib_bytes_left)) {
    case kDrawArgsOk: return 0;
    case kDrawIndexCountPastBuffer: return 1;
    case kDrawNullBuffer: return 2;
    }
    return -1;
}

// out: pair_records, wf_fast, tiny_tree, triangles, kernel_run, want_primary
extern "C" void fp_frame_plan(uint32_t n, uint64_t word2_0, uint64_t flags_0, uint64_t tris_all, uint64_t leaves_all,
                              uint64_t tris_max, int pair_option, int kernel_option, uint64_t* out)
{
    const FramePlan p = frame_plan(n, word2_0, flags_0, tris_all, leaves_all, tris_max, pair_option, kernel_option);
    out[0] = p.pair_records, out[1] = p.wf_fast, out[2] = p.tiny_tree, out[3] = p.triangles;
    out[4] = (uint64_t)p.kernel_run, out[5] = p.want_primary;
}

// the scan's third bit comes from the tiny-tree rule on the draw's nodes (mk_tiny_rule.h)
extern "C" uint32_t fp_tiny_leaves(const void* nodes, uint64_t n, uint32_t lim3)
{
    return mk_tiny_leaves(static_cast<const wcpt_node*>(nodes), n, lim3);
}
