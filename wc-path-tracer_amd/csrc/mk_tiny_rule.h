/* mk_tiny_rule.h — which BVHs the megakernel walks without its traversal loop (WCPT_OPTION_MK_TINY_TREE). Plain C++, no
 * HIP call: the device scan (pt_kernels.hip scan_tiny_tree) and tests/mk_tiny_rule_shim.cpp (g++) evaluate the same
 * function on a node array, and the launch (pt_kernels.hip launch_megakernel) and tests/mk_tiny_kernels_shim.cpp the same
 * condition for the walk-only kernels (mk_tiny_kernels, below).
 *
 * The reference's midpoint builder gives a mesh of a few dozen triangles or fewer -- a box, a panel, a prop, the Cornell
 * room -- a root leaf or a root over two leaves. The nodes of such a draw are the same for every lane, so a wave reads
 * them through the scalar cache and keeps the leaf ranges in SGPRs: no stack, no mode loop, no per-lane leaf cursor
 * (pt_tiny.h tiny_walk). The Cornell box's 34 triangles are a root and two 17-triangle leaves whose boxes are both the
 * whole room (each wall quad has a triangle in either leaf), so every bounce ray tests both leaves.
 *
 * A tree is tiny when
 *   - node 0 is a leaf, or
 *   - node 0 is interior, its children `left` and `left + 1` lie inside the buffer, and both are leaves,
 * and every such leaf starts on a triangle boundary and ends within the draw's derived records (what pt_device.h
 * kTriFlagLeafRecords demands of every leaf). The buffer's size is only an upper bound of the node count, so the rule
 * reads the nodes; nodes that the root does not reach do not matter.
 */
#ifndef WCPT_MK_TINY_RULE_H
#define WCPT_MK_TINY_RULE_H

#include <stdint.h>

#include "../../include/wcpt.h"
#include "mk_variant.h"

#ifdef __HIPCC__
#define WCPT_MK_TINY_HD __host__ __device__
#else
#define WCPT_MK_TINY_HD
#endif

namespace wcpt {

constexpr int kMkTinyAuto = -1; /* WCPT_OPTION_MK_TINY_TREE's default: wherever the rule allows */

/* a leaf of `count` index positions from `first` lies on derived records: first is a multiple of 3 and first + count
 * does not pass lim3 = 3 x the draw's triangles (scan_leaf_counts' test) */
WCPT_MK_TINY_HD inline bool mk_tiny_leaf_ok(uint32_t first, uint32_t count, uint32_t lim3)
{
    return count != 0u && first % 3u == 0u && first <= lim3 && count <= lim3 - first;
}

/* The leaves of a tiny tree (1 or 2), or 0 when the tree is not tiny. nodes: the BVH buffer's `n` nodes (n may exceed
 * the tree's); lim3: 3 x the triangles of the draw's derived records. */
WCPT_MK_TINY_HD inline uint32_t mk_tiny_leaves(const wcpt_node* nodes, uint64_t n, uint32_t lim3)
{
    if (n == 0u) return 0u;
    const uint32_t left = nodes[0].leftNodeOrTriangleIndex, count = nodes[0].triangleCount;
    if (count != 0u) return mk_tiny_leaf_ok(left, count, lim3) ? 1u : 0u;
    if ((uint64_t)left + 1u >= n) return 0u; /* a child outside the buffer */
    for (uint32_t c = 0; c < 2u; c++) {
        const wcpt_node& k = nodes[left + c];
        if (!mk_tiny_leaf_ok(k.leftNodeOrTriangleIndex, k.triangleCount, lim3)) return 0u; /* interior, or off the records */
    }
    return 2u;
}

/* Whether the runtime sets the draw's table flag (pt_device.h kTriFlagTinyTree): the option allows it (-1 automatic and
 * 1 alike: the path has measured a gain wherever it applies; 0 never) and the scan found a tiny tree. */
inline bool mk_tiny_enabled(int option, uint32_t leaves) { return option != 0 && leaves != 0u; }

/* Whether a megakernel launch runs on the walk-only head and tail (pt_mk_tiny.hip) instead of the general ones: a render
 * (mode: mk_variant.h kModeRender) of a draw whose table flag is set (tiny_tree: frame_prep.h FramePlan::tiny_tree, so
 * one draw command and the option not 0), which mk_variant_select splits (split), on pair records (pairs), with one
 * draw command (single), in exact arithmetic (arith: WCPT_ARITH_*). Those four kernels are all there is: everything
 * else -- a whole launch, fast arithmetic, single records, several draws, a larger tree, the option at 0 -- keeps the
 * general kernels and their traversal loop. wcpt_mk_tiny_tree_stats counts the renders for which this held. */
constexpr bool mk_tiny_kernels(int mode, bool tiny_tree, bool split, bool pairs, bool single, int arith)
{
    return mode == kModeRender && tiny_tree && split && pairs && single && arith == WCPT_ARITH_EXACT;
}

} // namespace wcpt

#undef WCPT_MK_TINY_HD
#endif
