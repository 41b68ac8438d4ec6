/* bvh_refit.h — the refit of a BVH to moved vertices (wcpt_bvh_refit, wcpt_bvh_refit_device): the tree's shape -- child
 * links, leaf ranges, index order, node numbering -- stays, and only the boxes are recomputed, bottom-up. Plain C++ that
 * also compiles as HIP device code: the kernels of pt_bvh_refit.hip call the refit_step_* functions below with i = their
 * global thread index, tests/bvh_refit_shim.cpp (g++) calls the same functions in loops over i, and wcpt_bvh_refit
 * (host/wcpt_host.cpp) uses them for its checks, its leaves and its unions. Everything the bytes of the result and the
 * refusals depend on is in this header; the .hip file adds only how the steps are spread over blocks and launches.
 *
 * The rule
 *   Leaf       triangleCount != 0 (counted in indices). Its box is the sequential fold of bvh_min / bvh_max over the
 *              vertices indices[left + 0 .. left + triangleCount) in index order from +-FLOAT32_MAX: the reference's
 *              UpdateNodeBounds (PathTracingRenderer.jai:130-145) on that range. `left` need not be a multiple of 3.
 *   Interior   min[c] = bvh_min(left.min[c], right.min[c]), max[c] = bvh_max(left.max[c], right.max[c]); the left child
 *              is the first operand. On finite input that is, in value, the fold over all the node's triangles, and
 *              the bits of a tied zero depend on the tree alone: a host loop and the device agree bit for bit.
 *   Never written: leftNodeOrTriangleIndex and triangleCount.
 *
 * Relation to the builders
 *   Both builders compute a node's box as a fold over its triangles in the order they had BEFORE the node's own
 *   partition, and resolve a +0 / -0 tie by that order: the midpoint builder keeps the last occurrence (bvh_midpoint.h),
 *   the SAH builder the first (bvh_sah.h). The finished tree no longer holds that order. So a refit of a freshly built
 *   tree over unchanged positions reproduces the builder's bounds in value, and in bits wherever the bound is not a
 *   zero; the only difference that can occur is the sign of a zero bound.
 *
 * What counts as a tree (read-only checks, all completed before a byte of `nodes` is written)
 *   1 <= nodes_used <= the node buffer's capacity (the entry points' own check, before any step runs);
 *   an interior node i has left > i and left + 1 < nodes_used, in 64-bit arithmetic (both builders number children
 *     after their parents; this also rules out cycles);                                             kRefitBadChild
 *   every node but node 0 is the child of exactly one interior node (node 0 of none: left > i >= 0); kRefitBadParents
 *   a leaf has triangleCount % 3 == 0 and left + triangleCount <= index_count;                       kRefitBadLeaf
 *   every index in [0, index_count) is < vertex_count, found by a pass that reads only the indices: no leaf reads a
 *     vertex, or an index as an address, once that pass has set its bit;                             kRefitBadIndex
 *   every coordinate a leaf references is finite.                                                    kRefitNotFinite
 *
 * The steps (each called once per i of its range, all calls of a step before any of the next; no step depends on the
 * order of its calls): check_index over the indices; node (validation, parent[], reference counts, the leaves' boxes
 * into scratch); depth (reference counts checked, depth[] by a walk up parent[], which ends because parent < child);
 * then the status is read, and for d = deepest interior depth .. 0 unite(d); then store. wcpt_bvh_refit runs the same
 * checks and, instead of the levels, one loop i = nodes_used - 1 .. 0: children come after parents.
 *
 * Scratch: 36 bytes per node (a box, a parent, a reference count, a depth) and the control words.
 */
#ifndef WCPT_BVH_REFIT_H
#define WCPT_BVH_REFIT_H

#include "bvh_midpoint.h"

#ifdef __HIPCC__
#define WCPT_REFIT_HD __host__ __device__
#else
#define WCPT_REFIT_HD
#endif

namespace wcpt {

/* status bits of a refit (BvhRefit::ctrl[kRefitCtrlStatus]); any of them refuses the call */
constexpr uint32_t kRefitBadIndex = 1u, kRefitBadChild = 2u, kRefitBadLeaf = 4u, kRefitBadParents = 8u, kRefitNotFinite = 16u;
/* control words: status, the deepest level that holds an interior node */
constexpr uint32_t kRefitCtrlStatus = 0u, kRefitCtrlDepth = 1u, kRefitCtrlWords = 4u;
constexpr uint32_t kRefitNone = 0xFFFFFFFFu; /* parent[]: no parent; depth[]: a leaf (no level unites it) */

struct RefitBox {
    float lo[3], hi[3];
};

struct BvhRefit {
    const float* vertices;   /* float[3] per vertex */
    uint32_t vertex_count;
    const uint32_t* indices;
    uint32_t index_count;
    wcpt_node* nodes;        /* read by every step; written by refit_step_store alone */
    uint32_t nodes_used;
    /* scratch, per node */
    RefitBox* box;
    uint32_t* parent;        /* kRefitNone before the node step */
    uint32_t* refs;          /* 0 before the node step: the interior nodes that name the node as a child */
    uint32_t* depth;
    uint32_t* ctrl;          /* kRefitCtrlWords, 0 before the first step */
};

/* what a refusal says (the lowest bit set: the order of the checks above) */
inline const char* refit_refusal(uint32_t status)
{
    if (status & kRefitBadIndex) return "an index is not below vertex_count";
    if (status & kRefitBadChild) return "an interior node's children do not lie after it and inside nodes_used";
    if (status & kRefitBadLeaf) return "a leaf's triangleCount is no multiple of 3 or its range exceeds index_count";
    if (status & kRefitBadParents) return "a node other than 0 is not the child of exactly one interior node";
    if (status & kRefitNotFinite) return "a referenced coordinate is not finite";
    return "";
}

WCPT_REFIT_HD inline void refit_word_max(uint32_t* word, uint32_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
    atomicMax(word, v);
#else
    if (v > *word) *word = v;
#endif
}

/* ---- the rule ------------------------------------------------------------------------------------------------ */

WCPT_REFIT_HD inline bool refit_is_leaf(const wcpt_node& n) { return n.triangleCount != 0u; }

/* the structural refusals of node i alone (no index and no vertex is read) */
WCPT_REFIT_HD inline uint32_t refit_node_status(const BvhRefit& r, uint32_t i)
{
    const wcpt_node& n = r.nodes[i];
    const uint64_t left = n.leftNodeOrTriangleIndex;
    if (refit_is_leaf(n)) return n.triangleCount % 3u != 0u || left + n.triangleCount > r.index_count ? kRefitBadLeaf : 0u;
    return left <= i || left + 1u >= r.nodes_used ? kRefitBadChild : 0u;
}

/* the box of a leaf whose range and indices have passed; false when a referenced coordinate is not finite */
WCPT_REFIT_HD inline bool refit_leaf_box(const BvhRefit& r, const wcpt_node& n, RefitBox& b)
{
    for (int c = 0; c < 3; c++) {
        b.lo[c] = kBvhFloatMax;
        b.hi[c] = -kBvhFloatMax;
    }
    bool finite = true;
    const uint64_t first = n.leftNodeOrTriangleIndex;
    for (uint32_t k = 0; k < n.triangleCount; k++) {
        const float* p = r.vertices + 3ull * r.indices[first + k];
        for (int c = 0; c < 3; c++) {
            const float x = p[c];
            finite = finite && bvh_finite(x);
            b.lo[c] = bvh_min(b.lo[c], x);
            b.hi[c] = bvh_max(b.hi[c], x);
        }
    }
    return finite;
}

/* the box of an interior node: the left child is the first operand */
WCPT_REFIT_HD inline RefitBox refit_union(const RefitBox& left, const RefitBox& right)
{
    RefitBox b;
    for (int c = 0; c < 3; c++) {
        b.lo[c] = bvh_min(left.lo[c], right.lo[c]);
        b.hi[c] = bvh_max(left.hi[c], right.hi[c]);
    }
    return b;
}

/* ---- the steps ----------------------------------------------------------------------------------------------- */

/* i < index_count. Reads the index buffer only. */
WCPT_REFIT_HD inline void refit_step_check_index(const BvhRefit& r, uint32_t i)
{
    if (r.indices[i] >= r.vertex_count) bvh_word_or(r.ctrl + kRefitCtrlStatus, kRefitBadIndex);
}

/* i < nodes_used, after every index was checked: node i's own validation; an interior node names itself its children's
 * parent and counts a reference on each; a leaf folds its triangles into box[i] -- unless an index failed: then no
 * index is used as an address. (Two interior nodes that name one child both write its parent[]: the count refuses.) */
WCPT_REFIT_HD inline void refit_step_node(const BvhRefit& r, uint32_t i)
{
    const uint32_t bad = refit_node_status(r, i);
    if (bad) {
        bvh_word_or(r.ctrl + kRefitCtrlStatus, bad);
        return;
    }
    const wcpt_node& n = r.nodes[i];
    if (!refit_is_leaf(n)) {
        const uint32_t left = n.leftNodeOrTriangleIndex;
        r.parent[left] = i;
        r.parent[left + 1u] = i;
        bvh_word_add(r.refs + left, 1u);
        bvh_word_add(r.refs + left + 1u, 1u);
        return;
    }
    if (r.ctrl[kRefitCtrlStatus] & kRefitBadIndex) return; /* written by the step before this one */
    RefitBox b;
    if (!refit_leaf_box(r, n, b)) bvh_word_or(r.ctrl + kRefitCtrlStatus, kRefitNotFinite);
    r.box[i] = b;
}

/* i < nodes_used: the reference count; depth[i] for an interior node, and the deepest such depth. parent[] holds only
 * what valid interior nodes wrote, so every step of the walk goes to a smaller node number and the walk ends. */
WCPT_REFIT_HD inline void refit_step_depth(const BvhRefit& r, uint32_t i)
{
    if (r.refs[i] != (i == 0u ? 0u : 1u)) {
        bvh_word_or(r.ctrl + kRefitCtrlStatus, kRefitBadParents);
        r.depth[i] = kRefitNone;
        return;
    }
    if (refit_is_leaf(r.nodes[i])) {
        r.depth[i] = kRefitNone;
        return;
    }
    uint32_t d = 0u;
    for (uint32_t p = r.parent[i]; p != kRefitNone; p = r.parent[p]) d++;
    r.depth[i] = d;
    refit_word_max(r.ctrl + kRefitCtrlDepth, d);
}

/* i < nodes_used, for d = the deepest interior depth .. 0, once the status was read as 0: an interior node of depth d
 * takes the union of its children's boxes, which are leaves' or of depth d + 1 */
WCPT_REFIT_HD inline void refit_step_unite(const BvhRefit& r, uint32_t i, uint32_t d)
{
    if (r.depth[i] != d) return;
    const uint32_t left = r.nodes[i].leftNodeOrTriangleIndex;
    r.box[i] = refit_union(r.box[left], r.box[left + 1u]);
}

/* i < nodes_used: the only write of the caller's nodes */
WCPT_REFIT_HD inline void refit_step_store(const BvhRefit& r, uint32_t i)
{
    const RefitBox b = r.box[i];
    for (int c = 0; c < 3; c++) {
        r.nodes[i].min[c] = b.lo[c];
        r.nodes[i].max[c] = b.hi[c];
    }
}

} // namespace wcpt

#undef WCPT_REFIT_HD
#endif
