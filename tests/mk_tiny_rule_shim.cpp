// Test shim (CPU): exposes the tiny-tree rule (wc-path-tracer_amd/csrc/mk_tiny_rule.h, what the device scan evaluates on
// a draw's BVH buffer) to tests/test_mk_tiny_rule.py over ctypes. Built by the test with g++; no HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/mk_tiny_rule.h"

// nodes: n x 32 B (wcpt_node); lim3: 3 x the draw's triangles. Returns the tree's leaves (1 or 2), 0 when not tiny.
extern "C" uint32_t mkt_leaves(const void* nodes, uint64_t n, uint32_t lim3)
{
    return wcpt::mk_tiny_leaves(static_cast<const wcpt_node*>(nodes), n, lim3);
}

extern "C" int mkt_leaf_ok(uint32_t first, uint32_t count, uint32_t lim3) { return wcpt::mk_tiny_leaf_ok(first, count, lim3) ? 1 : 0; }
extern "C" int mkt_enabled(int option, uint32_t leaves) { return wcpt::mk_tiny_enabled(option, leaves) ? 1 : 0; }
extern "C" int mkt_auto(void) { return wcpt::kMkTinyAuto; }
