/* bvh_midpoint.h — the midpoint BVH of wcpt_bvh_build (host/wcpt_host.cpp, PathTracingRenderer.jai:147-217), restated so
 * that it can be built level by level with one thread per triangle position. Plain C++ that also compiles as HIP device
 * code: the kernels of pt_bvh_build.hip call the bvh_step_* functions below with p = their global thread index, and
 * tests/bvh_levels_shim.cpp (g++) calls the same functions in loops over p. Everything the bytes of the result depend
 * on is in this header; the .hip file adds only how the steps are spread over waves and blocks.
 *
 * The rule
 *   Bounds     a node's min / max is the sequential fold of a < b ? a : b (a > b ? a : b) over its vertices in index
 *              order from +-FLOAT32_MAX. On finite input the operator is associative, and on a tie (only +0 against -0
 *              differ in bits) it keeps the LATER operand: the result is the smallest value, with the bits of its last
 *              occurrence. That is what a 64-bit integer minimum over (order-preserving value bits, with -0 folded onto
 *              +0) << 32 | ~position finds, in any order of evaluation (bvh_min_key); the bits are then read back from the
 *              winning position (bvh_step_finalize). Each triangle's own three vertices are folded once (bvh_step_prepare).
 *   Split      axis by the reference's two strict compares; splitPos = min[axis] + extent[axis] * 0.5f; a triangle
 *              goes left iff (a + b + c) / 3.0f < splitPos, unfused, IEEE divide (bvh_axis, bvh_split_pos, bvh_centroid).
 *   Stop       triangleCount <= 6 indices or depth budget 0 (root 32: levels 0..32) is a leaf; a partition that leaves
 *              one side empty leaves a leaf, with its indices as the partition moved them (bvh_splits).
 *   Partition  the reference's loop (i from the front; a right triangle is swapped with j from the back) has a closed
 *              form. In a segment of n triangles with L left ones, let b_1 > ... > b_m be the positions >= L that hold a
 *              left triangle and f_1 < ... < f_m the positions < L that hold a right one, b_0 = n. Then
 *                a left triangle at p < L stays; the one at b_k goes to f_k;
 *                the right triangle at f_k goes to b_(k-1) - 1; one at q > L goes to q - 1; one at q = L to b_m - 1.
 *              (bvh_partition_dest; the ranks come from one prefix count of the left flags, bvh_step_rank.)
 *   Numbering  root 0; the children of the k-th interior node in preorder sit at 1 + 2k, 2 + 2k. Preorder is order by
 *              (first triangle ascending, depth ascending), and the nodes that start at one position are a chain of left
 *              children on consecutive levels, all interior but perhaps the last. So with starts[p] = the interior nodes
 *              starting at p, E = its exclusive prefix sum and lvl0[p] = the level of the first node starting at p,
 *              k(node) = E[first] + level - lvl0[first] (bvh_interior_rank).
 *
 * Non-finite coordinates are refused (bvh_step_prepare): with a NaN the fold is not associative.
 */
#ifndef WCPT_BVH_MIDPOINT_H
#define WCPT_BVH_MIDPOINT_H

#include <stdint.h>
#include <string.h>

#include "../../include/wcpt.h"

#ifdef __HIPCC__
#define WCPT_BVH_HD __host__ __device__
#else
#define WCPT_BVH_HD
#endif

namespace wcpt {

constexpr uint32_t kBvhLeafIndices = 6u; /* Subdivide: triangleCount <= 6 is a leaf */
constexpr uint32_t kBvhRootBudget = 32u; /* the root's depth budget: a node on level 32 is a leaf */
constexpr float kBvhFloatMax = 3.40282346638528859812e+38f; /* FLOAT32_MAX, PathTracingRenderer.jai:126 */

/* status bits of a build (BvhBuild::ctrl[kBvhCtrlStatus]) */
constexpr uint32_t kBvhBadIndex = 1u, kBvhNotFinite = 2u;
/* control words: status, temporary nodes allocated, nodes split on the current level */
constexpr uint32_t kBvhCtrlStatus = 0u, kBvhCtrlNodes = 1u, kBvhCtrlSplits = 2u, kBvhCtrlWords = 4u;
/* the prefix sums are stored per block of 1 << kBvhScanShift elements: scan[] within the block, scan_off[] per block */
constexpr uint32_t kBvhScanShift = 11u;

/* ---- the arithmetic ------------------------------------------------------------------------------------------ */

WCPT_BVH_HD inline float bvh_min(float a, float b) { return a < b ? a : b; } /* Jai min */
WCPT_BVH_HD inline float bvh_max(float a, float b) { return a > b ? a : b; }

WCPT_BVH_HD inline int bvh_axis(const float mn[3], const float mx[3])
{
    float extent[3];
    for (int c = 0; c < 3; c++) extent[c] = mx[c] - mn[c];
    int axis = 0;
    if (extent[1] > extent[0]) axis = 1;
    if (extent[2] > extent[axis]) axis = 2;
    return axis;
}

WCPT_BVH_HD inline float bvh_split_pos(const float mn[3], const float mx[3], int axis)
{
    const float extent = mx[axis] - mn[axis];
    return mn[axis] + extent * 0.5f;
}

WCPT_BVH_HD inline float bvh_centroid(float a, float b, float c) { return (a + b + c) / 3.0f; }

/* whether a node of `triangles` triangles on `level` is partitioned at all */
WCPT_BVH_HD inline bool bvh_splits(uint32_t triangles, uint32_t level)
{
    return !(3ull * triangles <= kBvhLeafIndices || level >= kBvhRootBudget);
}

WCPT_BVH_HD inline uint32_t bvh_bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

WCPT_BVH_HD inline bool bvh_finite(float x) { return (bvh_bits(x) & 0x7f800000u) != 0x7f800000u; }

/* finite floats onto unsigned integers of the same order, -0 and +0 onto one value */
WCPT_BVH_HD inline uint32_t bvh_order_bits(float x)
{
    uint32_t u = bvh_bits(x);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

/* Keys whose integer minimum (maximum) over a node's triangles names the position whose value the fold ends on: the
 * smallest (largest) value, and among equal ones the last position. */
WCPT_BVH_HD inline unsigned long long bvh_min_key(float x, uint32_t pos)
{
    return ((unsigned long long)bvh_order_bits(x) << 32) | (uint32_t)~pos;
}
WCPT_BVH_HD inline unsigned long long bvh_max_key(float x, uint32_t pos)
{
    return ((unsigned long long)bvh_order_bits(x) << 32) | pos;
}
WCPT_BVH_HD inline uint32_t bvh_min_key_pos(unsigned long long k) { return ~(uint32_t)k; }
WCPT_BVH_HD inline uint32_t bvh_max_key_pos(unsigned long long k) { return (uint32_t)k; }
constexpr unsigned long long kBvhMinKeyInit = ~0ull, kBvhMaxKeyInit = 0ull; /* lose against every triangle's key */

/* The partition's closed form. r: a triangle's position in its segment of n triangles, `left` its side, e the left
 * triangles before r, L the segment's left triangles, m = L - (left triangles before L). tab[k - 1] = f_k and
 * tab[L + k - 1] = b_k for k = 1..m (positions in the segment; m <= L and m <= n - L, so both fit in n words). */
WCPT_BVH_HD inline uint32_t bvh_partition_dest(uint32_t r, bool left, uint32_t e, uint32_t n, uint32_t L, uint32_t m,
                                               const uint32_t* tab)
{
    if (left) return r < L ? r : tab[L - e - 1u];          /* the (L - e)-th left triangle from the back */
    if (r < L) {
        const uint32_t k = r + 1u - e;                     /* the k-th right triangle from the front */
        return (k == 1u ? n : tab[L + k - 2u]) - 1u;
    }
    if (r > L) return r - 1u;
    return (m == 0u ? n : tab[L + m - 1u]) - 1u;
}

/* ---- the build's state --------------------------------------------------------------------------------------- */

/* A node while the tree is built, numbered in the order of allocation (any order: the final numbering is derived). */
struct BvhTempNode {
    unsigned long long kmin[3], kmax[3]; /* bvh_min_key / bvh_max_key minima / maxima over the node's triangles */
    float bmin[3], bmax[3];              /* the bounds, once bvh_step_finalize has read them back */
    uint32_t first, count;               /* the node's triangle positions [first, first + count) */
    uint32_t level, parent;
    uint32_t left;                       /* 0: a leaf; else the children are temporary nodes left and left + 1 */
    uint32_t nleft;                      /* triangles of the left child */
};

struct BvhBuild {
    const float* vertices;   /* float[3] per vertex */
    uint32_t vertex_count;
    uint32_t* indices;       /* 3 * ntri, permuted at the end (bvh_step_permute into idx_tmp, then copied back) */
    uint32_t ntri;
    /* scratch, per original triangle: its centroid, and its own min / max folded over its vertices in order */
    float *cen, *tmin, *tmax;            /* 3 * ntri each */
    /* scratch, per triangle position */
    uint32_t *perm, *perm_next;          /* the original triangle at each position, now and after this level's scatter */
    uint32_t* owner;                     /* the temporary node of the deepest level that holds the position */
    uint32_t *flag, *scan, *scan_off;    /* ntri + 1 values and their prefix sums (bvh_scan_at) */
    uint32_t* tab;                       /* the rank tables of bvh_partition_dest, at each segment's positions */
    uint32_t *starts, *lvl0;             /* numbering: interior nodes starting at p (ntri + 1), level of the first one */
    BvhTempNode* tn;                     /* 2 * ntri */
    uint32_t* ctrl;                      /* kBvhCtrlWords */
    uint32_t* idx_tmp;                   /* 3 * ntri */
    wcpt_node* out;
};

/* words that several threads of one step write: atomics on the device, plain code in a host loop */
WCPT_BVH_HD inline void bvh_key_min(unsigned long long* slot, unsigned long long k)
{
#ifdef __HIP_DEVICE_COMPILE__
    atomicMin(slot, k);
#else
    if (k < *slot) *slot = k;
#endif
}
WCPT_BVH_HD inline void bvh_key_max(unsigned long long* slot, unsigned long long k)
{
#ifdef __HIP_DEVICE_COMPILE__
    atomicMax(slot, k);
#else
    if (k > *slot) *slot = k;
#endif
}
WCPT_BVH_HD inline void bvh_word_or(uint32_t* word, uint32_t bits)
{
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(word, bits);
#else
    *word |= bits;
#endif
}
WCPT_BVH_HD inline uint32_t bvh_word_add(uint32_t* word, uint32_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return atomicAdd(word, v);
#else
    const uint32_t old = *word;
    *word = old + v;
    return old;
#endif
}

/* the exclusive prefix sum at element p of what was scanned last (flag, or starts) */
WCPT_BVH_HD inline uint32_t bvh_scan_at(const BvhBuild& b, uint32_t p) { return b.scan[p] + b.scan_off[p >> kBvhScanShift]; }

WCPT_BVH_HD inline void bvh_node_init(BvhTempNode& n, uint32_t first, uint32_t count, uint32_t level, uint32_t parent)
{
    for (int c = 0; c < 3; c++) {
        n.kmin[c] = kBvhMinKeyInit;
        n.kmax[c] = kBvhMaxKeyInit;
        n.bmin[c] = kBvhFloatMax;
        n.bmax[c] = -kBvhFloatMax;
    }
    n.first = first;
    n.count = count;
    n.level = level;
    n.parent = parent;
    n.left = 0u;
    n.nleft = 0u;
}

/* ---- the steps: each is called once per p in [0, its range), all calls of a step before any of the next ---------- */

/* i < 3 * ntri. Reads the index buffer only: no vertex is read before every index has passed. */
WCPT_BVH_HD inline void bvh_step_check_index(const BvhBuild& b, uint32_t i)
{
    if (b.indices[i] >= b.vertex_count) bvh_word_or(b.ctrl + kBvhCtrlStatus, kBvhBadIndex);
}

/* t < ntri, after the indices have passed: triangle t's centroid and own bounds; the identity permutation; the root. */
WCPT_BVH_HD inline void bvh_step_prepare(const BvhBuild& b, uint32_t t)
{
    const float* v[3];
    for (int k = 0; k < 3; k++) v[k] = b.vertices + 3ull * b.indices[3ull * t + k];
    bool finite = true;
    for (int c = 0; c < 3; c++) {
        const float x = v[0][c], y = v[1][c], z = v[2][c];
        finite = finite && bvh_finite(x) && bvh_finite(y) && bvh_finite(z);
        b.cen[3ull * t + c] = bvh_centroid(x, y, z);
        b.tmin[3ull * t + c] = bvh_min(bvh_min(x, y), z);
        b.tmax[3ull * t + c] = bvh_max(bvh_max(x, y), z);
    }
    if (!finite) bvh_word_or(b.ctrl + kBvhCtrlStatus, kBvhNotFinite);
    b.perm[t] = t;
    b.owner[t] = 0u;
    b.starts[t] = 0u;
    b.lvl0[t] = 0u;
    if (t == 0u) {
        bvh_node_init(b.tn[0], 0u, b.ntri, 0u, 0u);
        b.ctrl[kBvhCtrlNodes] = 1u;
        b.flag[b.ntri] = 0u;
        b.starts[b.ntri] = 0u;
    }
}

/* the six keys of the triangle at position p */
WCPT_BVH_HD inline void bvh_bounds_keys(const BvhBuild& b, uint32_t p, unsigned long long keys[6])
{
    const uint64_t t = b.perm[p];
    for (int c = 0; c < 3; c++) {
        keys[c] = bvh_min_key(b.tmin[3ull * t + c], p);
        keys[3 + c] = bvh_max_key(b.tmax[3ull * t + c], p);
    }
}

WCPT_BVH_HD inline void bvh_keys_into(BvhTempNode& n, const unsigned long long keys[6])
{
    for (int c = 0; c < 3; c++) {
        bvh_key_min(&n.kmin[c], keys[c]);
        bvh_key_max(&n.kmax[c], keys[3 + c]);
    }
}

/* p < ntri: position p's triangle into the keys of its owner (the root's bounds; the children's: bvh_step_descend) */
WCPT_BVH_HD inline void bvh_step_accumulate(const BvhBuild& b, uint32_t p)
{
    unsigned long long keys[6];
    bvh_bounds_keys(b, p, keys);
    bvh_keys_into(b.tn[b.owner[p]], keys);
}

/* p < ntri: the first position of a node of `level` reads the node's bounds back from the winning positions */
WCPT_BVH_HD inline void bvh_step_finalize(const BvhBuild& b, uint32_t p, uint32_t level)
{
    BvhTempNode& n = b.tn[b.owner[p]];
    if (n.level != level || n.first != p) return;
    for (int c = 0; c < 3; c++) {
        n.bmin[c] = b.tmin[3ull * b.perm[bvh_min_key_pos(n.kmin[c])] + c];
        n.bmax[c] = b.tmax[3ull * b.perm[bvh_max_key_pos(n.kmax[c])] + c];
    }
}

/* whether position p lies in a node that is partitioned on `level` */
WCPT_BVH_HD inline bool bvh_active(const BvhTempNode& n, uint32_t level) { return n.level == level && bvh_splits(n.count, level); }

/* p < ntri: flag[p] = the triangle at p goes left in its node's partition; position 0 opens the level's split count */
WCPT_BVH_HD inline void bvh_step_classify(const BvhBuild& b, uint32_t p, uint32_t level)
{
    if (p == 0u) b.ctrl[kBvhCtrlSplits] = 0u;
    const BvhTempNode& n = b.tn[b.owner[p]];
    uint32_t left = 0u;
    if (bvh_active(n, level)) {
        const int axis = bvh_axis(n.bmin, n.bmax);
        left = b.cen[3ull * b.perm[p] + axis] < bvh_split_pos(n.bmin, n.bmax, axis) ? 1u : 0u;
    }
    b.flag[p] = left;
}

/* a position's view of its segment after the flags were scanned */
struct BvhSegView { uint32_t first, n, L, m, r, e; bool left; };

WCPT_BVH_HD inline BvhSegView bvh_seg_view(const BvhBuild& b, const BvhTempNode& n, uint32_t p)
{
    BvhSegView s;
    s.first = n.first;
    s.n = n.count;
    const uint32_t base = bvh_scan_at(b, n.first);
    s.L = bvh_scan_at(b, n.first + n.count) - base;
    s.m = s.L - (bvh_scan_at(b, n.first + s.L) - base);
    s.r = p - n.first;
    s.e = bvh_scan_at(b, p) - base;
    s.left = b.flag[p] != 0u;
    return s;
}

/* p < ntri: the left triangles behind L and the right ones before L write their positions into the rank tables */
WCPT_BVH_HD inline void bvh_step_rank(const BvhBuild& b, uint32_t p, uint32_t level)
{
    const BvhTempNode& n = b.tn[b.owner[p]];
    if (!bvh_active(n, level)) return;
    const BvhSegView s = bvh_seg_view(b, n, p);
    if (s.left && s.r >= s.L) b.tab[s.first + s.L + (s.L - s.e) - 1u] = s.r;
    if (!s.left && s.r < s.L) b.tab[s.first + (s.r + 1u - s.e) - 1u] = s.r;
}

/* p < ntri: the triangle at p moves to its place after the partition (perm -> perm_next); a node's first position
 * allocates the children of a node that splits. Other positions read only first / count / level of the node here. */
WCPT_BVH_HD inline void bvh_step_scatter(const BvhBuild& b, uint32_t p, uint32_t level)
{
    BvhTempNode& n = b.tn[b.owner[p]];
    if (!bvh_active(n, level)) {
        b.perm_next[p] = b.perm[p];
        return;
    }
    const BvhSegView s = bvh_seg_view(b, n, p);
    b.perm_next[s.first + bvh_partition_dest(s.r, s.left, s.e, s.n, s.L, s.m, b.tab + s.first)] = b.perm[p];
    if (s.r != 0u || s.L == 0u || s.L == s.n) return;
    const uint32_t self = b.owner[p];
    const uint32_t child = bvh_word_add(b.ctrl + kBvhCtrlNodes, 2u);
    bvh_node_init(b.tn[child], s.first, s.L, level + 1u, self);
    bvh_node_init(b.tn[child + 1u], s.first + s.L, s.n - s.L, level + 1u, self);
    n.left = child;
    n.nleft = s.L;
    b.starts[s.first] += 1u;
    b.lvl0[s.first + s.L] = level + 1u;
    bvh_word_add(b.ctrl + kBvhCtrlSplits, 1u);
}

/* the child that position p of a node split on `level` falls into, or 0 (perm is the scattered order by now) */
WCPT_BVH_HD inline uint32_t bvh_child_of(const BvhBuild& b, uint32_t p, uint32_t level)
{
    const BvhTempNode& n = b.tn[b.owner[p]];
    if (n.level != level || n.left == 0u) return 0u;
    return n.left + (p >= n.first + n.nleft ? 1u : 0u);
}

/* p < ntri: position p moves to its child and adds its triangle to the child's keys */
WCPT_BVH_HD inline void bvh_step_descend(const BvhBuild& b, uint32_t p, uint32_t level)
{
    const uint32_t child = bvh_child_of(b, p, level);
    if (child == 0u) return;
    b.owner[p] = child;
    bvh_step_accumulate(b, p);
}

/* the rank of an interior node among the interior nodes in preorder, after `starts` was scanned */
WCPT_BVH_HD inline uint32_t bvh_interior_rank(const BvhBuild& b, const BvhTempNode& n)
{
    return bvh_scan_at(b, n.first) + (n.level - b.lvl0[n.first]);
}

/* t < temporary nodes: node t into its final place */
WCPT_BVH_HD inline void bvh_step_emit(const BvhBuild& b, uint32_t t)
{
    const BvhTempNode& n = b.tn[t];
    uint32_t id = 0u;
    if (t != 0u) {
        const BvhTempNode& parent = b.tn[n.parent];
        id = 1u + 2u * bvh_interior_rank(b, parent) + (t - parent.left);
    }
    wcpt_node o;
    for (int c = 0; c < 3; c++) {
        o.min[c] = n.bmin[c];
        o.max[c] = n.bmax[c];
    }
    o.leftNodeOrTriangleIndex = n.left ? 1u + 2u * bvh_interior_rank(b, n) : 3u * n.first;
    o.triangleCount = n.left ? 0u : 3u * n.count;
    b.out[id] = o;
}

/* p < ntri: the index triple of the triangle that ends at position p */
WCPT_BVH_HD inline void bvh_step_permute(const BvhBuild& b, uint32_t p)
{
    const uint64_t t = b.perm[p];
    for (int k = 0; k < 3; k++) b.idx_tmp[3ull * p + k] = b.indices[3ull * t + k];
}

} // namespace wcpt

#undef WCPT_BVH_HD
#endif
