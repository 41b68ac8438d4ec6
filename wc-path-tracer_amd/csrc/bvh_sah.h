/* bvh_sah.h — the binned-SAH BVH of wcpt_bvh_build_sah (host/wcpt_host.cpp, bvh_build_sah), restated so that it can be
 * built level by level with one thread per triangle position (or per open node). Plain C++ that also compiles as HIP
 * device code: the kernels of pt_bvh_sah.hip call the sah_step_* functions below with their global thread index, and
 * tests/bvh_sah_levels_shim.cpp (g++) calls the same functions in loops. Everything the bytes of the result depend on is
 * in this header; the .hip file adds only how the steps are spread over waves and blocks. The order bits, the 64-bit
 * keys' layout, the scan layout and the preorder numbering are those of bvh_midpoint.h.
 *
 * The rule
 *   Bounds     Aabb::grow is p < lo ? p : lo (p > hi ? p : hi): on a tie it keeps the EARLIER operand, the opposite of
 *              the midpoint builder. A triangle's box folds its vertices in order from +-FLOAT32_MAX, a node's box its
 *              triangles' boxes in permutation order. A node's min is therefore the smallest value with the bits of its
 *              first occurrence (only +0 against -0 differ): the 64-bit integer minimum over
 *              (order bits << 32 | position) and maximum over (order bits << 32 | ~position), in any order of
 *              evaluation (sah_min_key, sah_max_key); the bits are read back from the winning position (sah_step_finalize).
 *   Centroids  0.5f * (lo + hi) of the triangle's box, unfused. The centroid box of a node and the 3 x 16 bin boxes are
 *              plain commutative minima / maxima of order bits (-0 folded onto +0). The sign of a zero cannot show in
 *              them: they feed only cen - lo and hi - lo, which have the same value for either zero and differ at most
 *              in the sign of a zero result, and those results feed only `ext > 0`, a product converted to an integer
 *              (0 either way), `hi < lo` and products and sums of binary64 areas that are never negative.
 *   Bin        (int)((cen - cbox.lo[a]) * scale), scale = 16.f / ext, clamped to 0..15, on every axis with ext > 0
 *              (sah_bin_index). The host's conversion is defined only for a finite product below 2^31, so the build
 *              REFUSES a centroid component that is not finite (kSahCentroidNotFinite) and an open node with an axis
 *              whose positive centroid extent is not finite or whose 16.f / ext is not finite (kSahBadScale). On
 *              everything else the product lies in [0, 16 + rounding]. (A finite centroid is at most FLOAT32_MAX / 2 in
 *              magnitude, so an extent of finite centroids is finite: that half of kSahBadScale is a guard that no
 *              input reaches. 16.f / ext is inf for ext below about 4.7e-38.)
 *   Costs      area() subtracts in binary32, widens, and computes 2.0 * (x*y + y*z + z*x) in binary64, unfused; 0 for an
 *              empty box (hi[0] < lo[0]). The right-to-left sweep stores area and count of bins b..15 for b = 15..1, the
 *              left-to-right one evaluates cost = area_L * n_L + area_R * n_R for bins 0..14 where both counts are
 *              positive; cost < best is strict from best = 1e300 over axes 0, 1, 2 and bins 0..14: the first minimum
 *              wins. split_cost = 1.0 + best / (parent_area > 0 ? parent_area : 1.0). (sah_step_evaluate)
 *   Stop       count <= 1 or level >= 40: a leaf (sah_opens). With a best split: a leaf when count <= 8 and
 *              split_cost >= count. Without one: a leaf at count <= 8; else, when no axis has a positive centroid
 *              extent, the node splits at count / 2 with the order unchanged (the host's std::stable_sort on all-equal
 *              keys is the identity). A node of more than 8 triangles with a positive extent but no cost below 1e300
 *              (every cost inf or NaN: a node box whose extent overflows binary32) would be sorted by centroid on the
 *              host; the build REFUSES it (kSahNoFiniteCost).
 *              left_n == 0 || left_n == count cannot occur after a best split was found: the partition's predicate is
 *              the binning function itself, so left_n is the winning sweep's left count, which the sweep required to be
 *              positive with a positive right count. (asserted in host loops: sah_step_scatter)
 *   Partition  stable: a left triangle goes to first + (left ones before it in the node), a right one to
 *              first + left_n + (right ones before it). One prefix sum of the left flags over the whole array serves
 *              every node of the level.
 *   Numbering  the host pops the left child first: preorder. Root 0; the children of the k-th interior node in preorder
 *              sit at 1 + 2k, 2 + 2k (bvh_midpoint.h: sah_interior_rank is its bvh_interior_rank).
 *   Nodes      a leaf holds (3 * first, 3 * count), an interior node (left child, 0) and the box of all its triangles.
 *   Indices    idx[3k + v] = old[3 * perm[k] + v], from a scratch copy (sah_step_permute).
 *
 * Differences from wcpt_bvh_build_sah: the refusals named above, a referenced coordinate that is not finite
 * (kBvhNotFinite) and an index that is not below vertex_count (kBvhBadIndex).
 *
 * Scratch: 352 bytes per triangle (SahBuild's arrays; 272 of them the 2 * ntri temporary nodes) plus 1536 bytes per open
 * node (count >= 2, level < 40) of the level that has most of them (SahBin[48]; at most ntri / 2 open nodes).
 */
#ifndef WCPT_BVH_SAH_H
#define WCPT_BVH_SAH_H

#include "bvh_midpoint.h"

#ifndef __HIP_DEVICE_COMPILE__
#include <assert.h>
#endif

#ifdef __HIPCC__
#define WCPT_SAH_HD __host__ __device__
#else
#define WCPT_SAH_HD
#endif

namespace wcpt {

constexpr int kSahBins = 16;
constexpr uint32_t kSahMaxLeaf = 8u;   /* triangles */
constexpr uint32_t kSahMaxDepth = 40u; /* a node on level 40 is a leaf */

/* further status bits of a build, beside kBvhBadIndex and kBvhNotFinite */
constexpr uint32_t kSahCentroidNotFinite = 4u, kSahBadScale = 8u, kSahNoFiniteCost = 16u;
/* control words: those of bvh_midpoint.h, and the open nodes among the children allocated on the current level */
constexpr uint32_t kSahCtrlOpen = 3u;
static_assert(kSahCtrlOpen < kBvhCtrlWords, "the control block holds the open count");
constexpr uint32_t kSahNoOpen = 0xFFFFFFFFu;
/* SahTempNode::split */
constexpr uint32_t kSahSplitNone = 0u, kSahSplitAxis0 = 1u /* 1 + axis */, kSahSplitMedian = 4u;

/* ---- the arithmetic ------------------------------------------------------------------------------------------ */

struct SahBox {
    float lo[3], hi[3];
};

WCPT_SAH_HD inline void sah_box_reset(SahBox& b)
{
    for (int c = 0; c < 3; c++) {
        b.lo[c] = kBvhFloatMax;
        b.hi[c] = -kBvhFloatMax;
    }
}
WCPT_SAH_HD inline void sah_box_grow(SahBox& b, const float* p)
{
    for (int c = 0; c < 3; c++) {
        b.lo[c] = p[c] < b.lo[c] ? p[c] : b.lo[c];
        b.hi[c] = p[c] > b.hi[c] ? p[c] : b.hi[c];
    }
}
WCPT_SAH_HD inline void sah_box_grow(SahBox& b, const SahBox& o)
{
    for (int c = 0; c < 3; c++) {
        b.lo[c] = o.lo[c] < b.lo[c] ? o.lo[c] : b.lo[c];
        b.hi[c] = o.hi[c] > b.hi[c] ? o.hi[c] : b.hi[c];
    }
}
WCPT_SAH_HD inline double sah_box_area(const SahBox& b)
{
    if (b.hi[0] < b.lo[0]) return 0.0;
    const double x = b.hi[0] - b.lo[0], y = b.hi[1] - b.lo[1], z = b.hi[2] - b.lo[2];
    return 2.0 * (x * y + y * z + z * x);
}

WCPT_SAH_HD inline float sah_centroid(float lo, float hi) { return 0.5f * (lo + hi); }

/* the inverse of bvh_order_bits (a zero comes back as +0) */
WCPT_SAH_HD inline float sah_from_order_bits(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float x;
    memcpy(&x, &u, sizeof(x));
    return x;
}

/* The bin of a centroid component. For a product in [0, 2^31) this is the host's (int) conversion and clamp; what lies
 * outside (only where the build is refused) is clamped before the conversion, which is undefined there. */
WCPT_SAH_HD inline int sah_bin_index(float cen, float lo, float scale)
{
    const float x = (cen - lo) * scale;
    if (!(x < (float)kSahBins)) return kSahBins - 1;
    if (!(x >= 0.0f)) return 0;
    return (int)x;
}

/* whether a node of `count` triangles on `level` looks for a split at all */
WCPT_SAH_HD inline bool sah_opens(uint32_t count, uint32_t level) { return !(count <= 1u || level >= kSahMaxDepth); }

/* Keys whose integer minimum (maximum) over a node's triangles names the position whose value the fold ends on: the
 * smallest (largest) value, and among equal ones the first position. */
WCPT_SAH_HD inline unsigned long long sah_min_key(float x, uint32_t pos)
{
    return ((unsigned long long)bvh_order_bits(x) << 32) | pos;
}
WCPT_SAH_HD inline unsigned long long sah_max_key(float x, uint32_t pos)
{
    return ((unsigned long long)bvh_order_bits(x) << 32) | (uint32_t)~pos;
}
WCPT_SAH_HD inline uint32_t sah_min_key_pos(unsigned long long k) { return (uint32_t)k; }
WCPT_SAH_HD inline uint32_t sah_max_key_pos(unsigned long long k) { return ~(uint32_t)k; }

/* ---- the build's state --------------------------------------------------------------------------------------- */

/* one of a node's 3 x 16 bins: its triangles' box as order bits, and their number */
struct SahBin {
    uint32_t lo[3], hi[3];
    uint32_t n, pad;
};
constexpr uint32_t kSahBinsPerNode = 3u * kSahBins;

struct SahTempNode {
    unsigned long long kmin[3], kmax[3]; /* sah_min_key / sah_max_key minima / maxima over the node's triangles */
    uint32_t cmin[3], cmax[3];           /* the centroid box, as order bits */
    float bmin[3], bmax[3];              /* the bounds, once sah_step_finalize has read them back */
    uint32_t first, count;               /* the node's triangle positions [first, first + count) */
    uint32_t level, parent;
    uint32_t left;                       /* 0: a leaf; else the children are temporary nodes left and left + 1 */
    uint32_t nleft;                      /* triangles of the left child (sah_step_evaluate) */
    uint32_t open;                       /* its number among the level's open nodes (its bins), or kSahNoOpen */
    uint32_t split;                      /* kSahSplitNone, kSahSplitAxis0 + axis, kSahSplitMedian */
    uint32_t bin;                        /* a binned split: bins 0..bin go left */
    uint32_t pad;
};

struct SahBuild {
    const float* vertices;   /* float[3] per vertex */
    uint32_t vertex_count;
    uint32_t* indices;       /* 3 * ntri, permuted at the end from idx_tmp, the copy of what they were */
    uint32_t ntri;
    /* scratch, per original triangle: its centroid and its own box */
    float *cen, *tmin, *tmax;            /* 3 * ntri each */
    /* scratch, per triangle position */
    uint32_t *perm, *perm_next;          /* the original triangle at each position, now and after this level's scatter */
    uint32_t* owner;                     /* the temporary node of the deepest level that holds the position */
    uint32_t *flag, *scan, *scan_off;    /* ntri + 1 values and their prefix sums (sah_scan_at) */
    uint32_t *starts, *lvl0;             /* numbering: interior nodes starting at p (ntri + 1), level of the first one */
    uint32_t* open_node;                 /* the temporary node of each open node of the level (ntri) */
    SahTempNode* tn;                     /* 2 * ntri */
    SahBin* bins;                        /* kSahBinsPerNode per open node of the level */
    uint32_t* ctrl;                      /* kBvhCtrlWords */
    uint32_t* idx_tmp;                   /* 3 * ntri */
    wcpt_node* out;
};

WCPT_SAH_HD inline void sah_word_min(uint32_t* slot, uint32_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
    atomicMin(slot, v);
#else
    if (v < *slot) *slot = v;
#endif
}
WCPT_SAH_HD inline void sah_word_max(uint32_t* slot, uint32_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
    atomicMax(slot, v);
#else
    if (v > *slot) *slot = v;
#endif
}

WCPT_SAH_HD inline uint32_t sah_scan_at(const SahBuild& b, uint32_t p) { return b.scan[p] + b.scan_off[p >> kBvhScanShift]; }

/* an empty box in order bits: +-FLOAT32_MAX, which no finite value loses against */
WCPT_SAH_HD inline uint32_t sah_empty_lo() { return bvh_order_bits(kBvhFloatMax); }
WCPT_SAH_HD inline uint32_t sah_empty_hi() { return bvh_order_bits(-kBvhFloatMax); }

WCPT_SAH_HD inline void sah_node_init(SahTempNode& n, uint32_t first, uint32_t count, uint32_t level, uint32_t parent)
{
    for (int c = 0; c < 3; c++) {
        n.kmin[c] = kBvhMinKeyInit;
        n.kmax[c] = kBvhMaxKeyInit;
        n.cmin[c] = sah_empty_lo();
        n.cmax[c] = sah_empty_hi();
        n.bmin[c] = kBvhFloatMax;
        n.bmax[c] = -kBvhFloatMax;
    }
    n.first = first;
    n.count = count;
    n.level = level;
    n.parent = parent;
    n.left = 0u;
    n.nleft = 0u;
    n.open = kSahNoOpen;
    n.split = kSahSplitNone;
    n.bin = 0u;
    n.pad = 0u;
}

WCPT_SAH_HD inline SahBox sah_centroid_box(const SahTempNode& n)
{
    SahBox b;
    for (int c = 0; c < 3; c++) {
        b.lo[c] = sah_from_order_bits(n.cmin[c]);
        b.hi[c] = sah_from_order_bits(n.cmax[c]);
    }
    return b;
}

/* the bin of original triangle t on `axis` of a node whose centroid box is cbox (ext > 0 on that axis) */
WCPT_SAH_HD inline int sah_bin_of(const SahBuild& b, const SahBox& cbox, uint64_t t, int axis)
{
    const float ext = cbox.hi[axis] - cbox.lo[axis];
    const float scale = (float)kSahBins / ext;
    return sah_bin_index(b.cen[3ull * t + axis], cbox.lo[axis], scale);
}

/* ---- the steps: each is called once per index in [0, its range), all calls of a step before any of the next ------ */

/* i < 3 * ntri. Reads the index buffer only: no vertex is read before every index has passed. */
WCPT_SAH_HD inline void sah_step_check_index(const SahBuild& b, uint32_t i)
{
    if (b.indices[i] >= b.vertex_count) bvh_word_or(b.ctrl + kBvhCtrlStatus, kBvhBadIndex);
}

/* t < ntri, after the indices have passed: triangle t's box and centroid; the identity permutation; the root. */
WCPT_SAH_HD inline void sah_step_prepare(const SahBuild& b, uint32_t t)
{
    SahBox box;
    sah_box_reset(box);
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        const float* v = b.vertices + 3ull * b.indices[3ull * t + k];
        for (int c = 0; c < 3; c++) finite = finite && bvh_finite(v[c]);
        sah_box_grow(box, v);
    }
    bool centroid_finite = true;
    for (int c = 0; c < 3; c++) {
        const float m = sah_centroid(box.lo[c], box.hi[c]);
        centroid_finite = centroid_finite && bvh_finite(m);
        b.cen[3ull * t + c] = m;
        b.tmin[3ull * t + c] = box.lo[c];
        b.tmax[3ull * t + c] = box.hi[c];
    }
    if (!finite) bvh_word_or(b.ctrl + kBvhCtrlStatus, kBvhNotFinite);
    else if (!centroid_finite) bvh_word_or(b.ctrl + kBvhCtrlStatus, kSahCentroidNotFinite);
    b.perm[t] = t;
    b.owner[t] = 0u;
    b.starts[t] = 0u;
    b.lvl0[t] = 0u;
    if (t == 0u) {
        sah_node_init(b.tn[0], 0u, b.ntri, 0u, 0u);
        if (sah_opens(b.ntri, 0u)) {
            b.tn[0].open = 0u;
            b.open_node[0] = 0u;
        }
        b.ctrl[kBvhCtrlNodes] = 1u;
        b.flag[b.ntri] = 0u;
        b.starts[b.ntri] = 0u;
    }
}

/* what the triangle at position p adds to its node: six keys of the box, six order words of the centroid */
struct SahContribution {
    unsigned long long keys[6];
    uint32_t cen[6];
};

WCPT_SAH_HD inline void sah_contribution_none(SahContribution& k)
{
    for (int c = 0; c < 3; c++) {
        k.keys[c] = kBvhMinKeyInit;
        k.keys[3 + c] = kBvhMaxKeyInit;
        k.cen[c] = sah_empty_lo();
        k.cen[3 + c] = sah_empty_hi();
    }
}

WCPT_SAH_HD inline void sah_contribution(const SahBuild& b, uint32_t p, SahContribution& k)
{
    const uint64_t t = b.perm[p];
    for (int c = 0; c < 3; c++) {
        k.keys[c] = sah_min_key(b.tmin[3ull * t + c], p);
        k.keys[3 + c] = sah_max_key(b.tmax[3ull * t + c], p);
        k.cen[c] = k.cen[3 + c] = bvh_order_bits(b.cen[3ull * t + c]);
    }
}

/* commutative and associative: contributions may be combined in any grouping before they reach the node */
WCPT_SAH_HD inline void sah_contribution_merge(SahContribution& k, const SahContribution& o)
{
    for (int c = 0; c < 3; c++) {
        if (o.keys[c] < k.keys[c]) k.keys[c] = o.keys[c];
        if (o.keys[3 + c] > k.keys[3 + c]) k.keys[3 + c] = o.keys[3 + c];
        if (o.cen[c] < k.cen[c]) k.cen[c] = o.cen[c];
        if (o.cen[3 + c] > k.cen[3 + c]) k.cen[3 + c] = o.cen[3 + c];
    }
}

WCPT_SAH_HD inline void sah_contribution_into(SahTempNode& n, const SahContribution& k)
{
    for (int c = 0; c < 3; c++) {
        bvh_key_min(&n.kmin[c], k.keys[c]);
        bvh_key_max(&n.kmax[c], k.keys[3 + c]);
        sah_word_min(&n.cmin[c], k.cen[c]);
        sah_word_max(&n.cmax[c], k.cen[3 + c]);
    }
}

/* p < ntri: position p's triangle into its owner (the root's boxes; the children's: sah_step_descend) */
WCPT_SAH_HD inline void sah_step_accumulate(const SahBuild& b, uint32_t p)
{
    SahContribution k;
    sah_contribution(b, p, k);
    sah_contribution_into(b.tn[b.owner[p]], k);
}

/* p < ntri: the first position of a node of `level` reads the node's bounds back from the winning positions */
WCPT_SAH_HD inline void sah_step_finalize(const SahBuild& b, uint32_t p, uint32_t level)
{
    SahTempNode& n = b.tn[b.owner[p]];
    if (n.level != level || n.first != p) return;
    for (int c = 0; c < 3; c++) {
        n.bmin[c] = b.tmin[3ull * b.perm[sah_min_key_pos(n.kmin[c])] + c];
        n.bmax[c] = b.tmax[3ull * b.perm[sah_max_key_pos(n.kmax[c])] + c];
    }
}

WCPT_SAH_HD inline void sah_bin_reset(SahBin& s)
{
    for (int c = 0; c < 3; c++) {
        s.lo[c] = sah_empty_lo();
        s.hi[c] = sah_empty_hi();
    }
    s.n = 0u;
    s.pad = 0u;
}

/* i < kSahBinsPerNode * (open nodes of the level): an empty bin */
WCPT_SAH_HD inline void sah_step_bin_init(const SahBuild& b, uint32_t i) { sah_bin_reset(b.bins[i]); }

/* the triangle at position p of node n into its bin, on every axis of positive centroid extent, of the
 * kSahBinsPerNode bins at `node_bins`: the node's own, or a private copy that sah_bin_merge adds to them later */
WCPT_SAH_HD inline void sah_bin_into(const SahBuild& b, const SahTempNode& n, uint32_t p, SahBin* node_bins)
{
    const uint64_t t = b.perm[p];
    const SahBox cbox = sah_centroid_box(n);
    for (int a = 0; a < 3; a++) {
        if (!(cbox.hi[a] - cbox.lo[a] > 0.0f)) continue;
        SahBin& s = node_bins[a * kSahBins + sah_bin_of(b, cbox, t, a)];
        for (int c = 0; c < 3; c++) {
            sah_word_min(&s.lo[c], bvh_order_bits(b.tmin[3ull * t + c]));
            sah_word_max(&s.hi[c], bvh_order_bits(b.tmax[3ull * t + c]));
        }
        bvh_word_add(&s.n, 1u);
    }
}

/* p < ntri: the triangle at p into the bins of its open node */
WCPT_SAH_HD inline void sah_step_bin(const SahBuild& b, uint32_t p, uint32_t level)
{
    const SahTempNode& n = b.tn[b.owner[p]];
    if (n.level != level || n.open == kSahNoOpen) return;
    sah_bin_into(b, n, p, b.bins + (uint64_t)n.open * kSahBinsPerNode);
}

/* The second path, for large nodes. The positions are cut into spans of kSahBinSpan; a span whose first and last
 * position have one owner lies in that node altogether (a node's positions are contiguous, and a node that has split
 * owns none), and where that node is open on `level` the span may collect its triangles in private bins
 * (sah_bin_reset, sah_bin_into) and add those to the node's once (sah_bin_merge) instead of calling sah_step_bin per
 * position. Minima, maxima and sums of integers: which spans take which path does not show in the bins. */
constexpr uint32_t kSahBinSpan = 1024u;

WCPT_SAH_HD inline bool sah_span_private(const SahBuild& b, uint32_t first, uint32_t last, uint32_t level)
{
    if (b.owner[first] != b.owner[last]) return false;
    const SahTempNode& n = b.tn[b.owner[first]];
    return n.level == level && n.open != kSahNoOpen;
}

WCPT_SAH_HD inline void sah_bin_merge(SahBin& dst, const SahBin& src)
{
    if (src.n == 0u) return;
    for (int c = 0; c < 3; c++) {
        sah_word_min(&dst.lo[c], src.lo[c]);
        sah_word_max(&dst.hi[c], src.hi[c]);
    }
    bvh_word_add(&dst.n, src.n);
}

WCPT_SAH_HD inline SahBox sah_bin_box(const SahBin& s)
{
    SahBox b;
    for (int c = 0; c < 3; c++) {
        b.lo[c] = sah_from_order_bits(s.lo[c]);
        b.hi[c] = sah_from_order_bits(s.hi[c]);
    }
    return b;
}

/* o < open nodes of the level: the two sweeps over the node's bins, and what becomes of the node */
WCPT_SAH_HD inline void sah_step_evaluate(const SahBuild& b, uint32_t o)
{
    SahTempNode& n = b.tn[b.open_node[o]];
    SahBox box;
    for (int c = 0; c < 3; c++) {
        box.lo[c] = n.bmin[c];
        box.hi[c] = n.bmax[c];
    }
    const SahBox cbox = sah_centroid_box(n);
    const double parent_area = sah_box_area(box);
    double best = 1e300;
    int best_axis = -1, best_bin = -1;
    uint32_t best_left = 0u;
    bool any_extent = false;
    for (int a = 0; a < 3; a++) {
        const float ext = cbox.hi[a] - cbox.lo[a];
        if (!(ext > 0.0f)) continue;
        any_extent = true;
        if (!bvh_finite(ext) || !bvh_finite((float)kSahBins / ext)) {
            bvh_word_or(b.ctrl + kBvhCtrlStatus, kSahBadScale);
            return;
        }
        const SahBin* bins = b.bins + ((uint64_t)o * 3u + a) * kSahBins;
        double right_area[kSahBins];
        uint32_t right_n[kSahBins];
        SahBox acc;
        sah_box_reset(acc);
        uint32_t cnt = 0u;
        for (int k = kSahBins - 1; k > 0; k--) {
            sah_box_grow(acc, sah_bin_box(bins[k]));
            cnt += bins[k].n;
            right_area[k] = sah_box_area(acc);
            right_n[k] = cnt;
        }
        sah_box_reset(acc);
        cnt = 0u;
        for (int k = 0; k < kSahBins - 1; k++) {
            sah_box_grow(acc, sah_bin_box(bins[k]));
            cnt += bins[k].n;
            if (cnt == 0u || right_n[k + 1] == 0u) continue;
            const double cost = sah_box_area(acc) * cnt + right_area[k + 1] * right_n[k + 1];
            if (cost < best) {
                best = cost;
                best_axis = a;
                best_bin = k;
                best_left = cnt;
            }
        }
    }
    if (best_axis >= 0) {
        const double split_cost = 1.0 + best / (parent_area > 0.0 ? parent_area : 1.0);
        if (split_cost >= (double)n.count && n.count <= kSahMaxLeaf) return; /* the leaf is cheaper */
        n.split = kSahSplitAxis0 + (uint32_t)best_axis;
        n.bin = (uint32_t)best_bin;
        n.nleft = best_left;
        return;
    }
    if (n.count <= kSahMaxLeaf) return;
    if (any_extent) {
        bvh_word_or(b.ctrl + kBvhCtrlStatus, kSahNoFiniteCost);
        return;
    }
    n.split = kSahSplitMedian;
    n.nleft = n.count / 2u;
}

/* p < ntri: flag[p] = the triangle at p goes left in its node's split; position 0 opens the level's counts */
WCPT_SAH_HD inline void sah_step_classify(const SahBuild& b, uint32_t p, uint32_t level)
{
    if (p == 0u) {
        b.ctrl[kBvhCtrlSplits] = 0u;
        b.ctrl[kSahCtrlOpen] = 0u;
    }
    const SahTempNode& n = b.tn[b.owner[p]];
    uint32_t left = 0u;
    if (n.level == level && n.split != kSahSplitNone) {
        if (n.split == kSahSplitMedian) {
            left = p - n.first < n.nleft ? 1u : 0u;
        } else {
            const int axis = (int)(n.split - kSahSplitAxis0);
            left = sah_bin_of(b, sah_centroid_box(n), b.perm[p], axis) <= (int)n.bin ? 1u : 0u;
        }
    }
    b.flag[p] = left;
}

/* p < ntri, after the flags were scanned: the triangle at p moves to its place in the stable partition
 * (perm -> perm_next); a splitting node's first position allocates the children and numbers the open ones. Other
 * positions read only first / count / level / split / nleft of the node here. */
WCPT_SAH_HD inline void sah_step_scatter(const SahBuild& b, uint32_t p, uint32_t level)
{
    SahTempNode& n = b.tn[b.owner[p]];
    if (n.level != level || n.split == kSahSplitNone) {
        b.perm_next[p] = b.perm[p];
        return;
    }
    const uint32_t base = sah_scan_at(b, n.first);
    const uint32_t e = sah_scan_at(b, p) - base; /* left triangles before p in the node */
    const uint32_t r = p - n.first, L = n.nleft;
#ifndef __HIP_DEVICE_COMPILE__
    assert(sah_scan_at(b, n.first + n.count) - base == L && L != 0u && L != n.count);
#endif
    b.perm_next[n.first + (b.flag[p] ? e : L + (r - e))] = b.perm[p];
    if (r != 0u) return;
    const uint32_t self = b.owner[p];
    const uint32_t child = bvh_word_add(b.ctrl + kBvhCtrlNodes, 2u);
    sah_node_init(b.tn[child], n.first, L, level + 1u, self);
    sah_node_init(b.tn[child + 1u], n.first + L, n.count - L, level + 1u, self);
    for (uint32_t k = 0; k < 2u; k++) {
        if (!sah_opens(b.tn[child + k].count, level + 1u)) continue;
        const uint32_t o = bvh_word_add(b.ctrl + kSahCtrlOpen, 1u);
        b.tn[child + k].open = o;
        b.open_node[o] = child + k;
    }
    n.left = child;
    b.starts[n.first] += 1u;
    b.lvl0[n.first + L] = level + 1u;
    bvh_word_add(b.ctrl + kBvhCtrlSplits, 1u);
}

/* the child that position p of a node split on `level` falls into, or 0 (perm is the scattered order by now) */
WCPT_SAH_HD inline uint32_t sah_child_of(const SahBuild& b, uint32_t p, uint32_t level)
{
    const SahTempNode& n = b.tn[b.owner[p]];
    if (n.level != level || n.left == 0u) return 0u;
    return n.left + (p >= n.first + n.nleft ? 1u : 0u);
}

/* p < ntri: position p moves to its child and adds its triangle to the child's boxes */
WCPT_SAH_HD inline void sah_step_descend(const SahBuild& b, uint32_t p, uint32_t level)
{
    const uint32_t child = sah_child_of(b, p, level);
    if (child == 0u) return;
    b.owner[p] = child;
    sah_step_accumulate(b, p);
}

/* the rank of an interior node among the interior nodes in preorder, after `starts` was scanned */
WCPT_SAH_HD inline uint32_t sah_interior_rank(const SahBuild& b, const SahTempNode& n)
{
    return sah_scan_at(b, n.first) + (n.level - b.lvl0[n.first]);
}

/* t < temporary nodes: node t into its final place */
WCPT_SAH_HD inline void sah_step_emit(const SahBuild& b, uint32_t t)
{
    const SahTempNode& n = b.tn[t];
    uint32_t id = 0u;
    if (t != 0u) {
        const SahTempNode& parent = b.tn[n.parent];
        id = 1u + 2u * sah_interior_rank(b, parent) + (t - parent.left);
    }
    wcpt_node o;
    for (int c = 0; c < 3; c++) {
        o.min[c] = n.bmin[c];
        o.max[c] = n.bmax[c];
    }
    o.leftNodeOrTriangleIndex = n.left ? 1u + 2u * sah_interior_rank(b, n) : 3u * n.first;
    o.triangleCount = n.left ? 0u : 3u * n.count;
    b.out[id] = o;
}

/* p < ntri: the index triple of the triangle that ends at position p, from the copy of the caller's indices */
WCPT_SAH_HD inline void sah_step_permute(const SahBuild& b, uint32_t p)
{
    const uint64_t t = b.perm[p];
    for (int k = 0; k < 3; k++) b.indices[3ull * p + k] = b.idx_tmp[3ull * t + k];
}

} // namespace wcpt

#undef WCPT_SAH_HD
#endif
