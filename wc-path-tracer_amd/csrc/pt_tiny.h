/* pt_tiny.h -- Intersect for a tiny tree (mk_tiny_rule.h: a root leaf, or a root over two leaves), as the walk-only
 * kernels of pt_mk_tiny.hip run it: no traversal loop, no stack, no mode. Exact arithmetic on pair records, one draw.
 *
 * The nodes are the same for every lane, so the wave reads them with scalar loads and the leaves' record ranges are SALU
 * values. What stays per lane is the reference's own arithmetic and its decisions -- the slab tests (one per distinct box: tiny_walk), root_step's
 * cull (root_survives), interior_step's order and its two box passes (child_pair), the pop's cull of the far child
 * against the rec.t the near leaf left -- through the same definitions as the traversal loop, NaN behaviour included. A
 * leaf is run by the whole wave under a wave-uniform branch (some lane visits it), and a lane that the reference would
 * not have brought there takes nothing (`visit`): there is no wave-uniform loop under divergent control.
 * rec.t stays in its integer form (take_bits) and the winner a record tag across both leaves, decoded once. */
#ifndef WCPT_PT_TINY_H
#define WCPT_PT_TINY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_device.h"

namespace wcpt::dev {

/* The pair record that both leaves test (two 17-triangle midpoint leaves share the pair (16, 17): one slot each), tested
 * once per ray and segment. `off` is its byte offset in the records (kNoTag: the leaves share none) and `have` whether
 * `ph` holds its test; both wave-uniform. Whichever leaf the wave runs first computes `ph` for every lane -- the same
 * test of the same ray on the same record, whoever visits -- and every later run of a leaf over that record applies the
 * kept t values and acceptance bits against its own rec.t, in index order, strict <, through pair_take_bits like any
 * other pair. */
struct SharedPair { uint32_t off; bool have; PairHit ph; };

/* The pair record two leaves of triangles [k0L, kendL) and [k0R, kendR) both reach into: where one leaf's last pair is
 * the other's first. Nothing is assumed of the ranges' order or distance; ranges that overlap in more than one pair test
 * the others once per leaf, as leaves that share no pair do. All wave-uniform. */
template <uint32_t kBytes>
__device__ __forceinline__ uint32_t tiny_shared_offset(uint32_t k0L, uint32_t kendL, uint32_t k0R, uint32_t kendR)
{
    const uint32_t firstL = k0L >> 1, lastL = (kendL - 1u) >> 1, firstR = k0R >> 1, lastR = (kendR - 1u) >> 1;
    if (lastL == firstR) return lastL * kBytes;
    if (lastR == firstL) return lastR * kBytes;
    return kNoTag;
}

/* The leaf's triangles [k0, kend), both wave-uniform, as one scalar loop over the pair records that hold them. Every
 * pair is tested the same way; a pair of which the leaf owns only one slot (it starts in slot 1, or ends in slot 0)
 * takes only that slot: whether a slot is the leaf's is a SALU condition on the takes. Only visiting lanes take.
 * Applied in index order, strict <: pair_take_bits. */
template <bool PRIM, int A>
__device__ __forceinline__ void tiny_leaf(const Ray& ray, const WCPT_GLOBAL char* pbase, uint32_t k0, uint32_t kend,
                                          bool visit, uint32_t& rb, uint32_t& tag, SharedPair& sp)
{
    constexpr uint32_t kBytes = PRIM ? kPrimPairRecordBytes : kPairRecordBytes;
    const uint32_t oEnd = ((kend + 1u) >> 1) * kBytes;
    uint32_t k = k0 & ~1u; /* the first triangle of the pair at o */
    for (uint32_t o = (k0 >> 1) * kBytes; o < oEnd; o += kBytes, k += 2u) {
        const bool own0 = k >= k0, own1 = k + 1u < kend; /* wave-uniform */
        PairHit ph;
        if (o == sp.off && sp.have) { /* wave-uniform */
            ph = sp.ph;
        } else {
            if constexpr (PRIM) {
                const TriPairP p = load_pairP_const(pbase, o);
                v2f px, py, pz;
                const v2f det = pairP_det<A>(ray, p, px, py, pz);
                /* no visiting lane can take either triangle: pair_leaf's sign pre-reject (a shared pair is then not
                 * kept: the other leaf's visitors decide for themselves) */
                if (__builtin_amdgcn_ballot_w64(visit && pairP_may_take(p, det)) == 0ull) continue;
                ph = pairP_finish<A>(ray, p, px, py, pz, det);
            } else {
                ph = rayTrianglePair<A>(ray, load_pair_const(pbase, o));
            }
            if (o == sp.off) {
                sp.ph = ph;
                sp.have = true;
            }
        }
        ph.hit0 = ph.hit0 && visit && own0;
        ph.hit1 = ph.hit1 && visit && own1;
        pair_take_bits(ph, o, rb, tag);
    }
}

/* One lane's side of a tiny tree: whether it is inside the root's box (root_survives), and under an interior root the
 * child-pair decision (child_pair; unread under a root leaf). */
struct TinyLane { bool in; ChildPair c; };
/* The record ranges of the leaves, wave-uniform: triangles [k0L, kendL) and, under an interior root, [k0R, kendR). */
struct TinyRanges { bool two; uint32_t k0L, kendL, k0R, kendR; };

/* The leaves of the walk. A root leaf is visited by the lanes inside its box. Under an interior root a lane visits a
 * leaf iff it passed the leaf's box and the box's entry distance is not beyond rec.t as it stands when the leaf's turn
 * comes (:162; for a lane's near child that is interior_step's `!(nearT0 > rt)`, for its far child the pop's cull).
 *   - A wave whose lanes inside the root all pop the same child first -- every wave where the two boxes coincide, as in
 *     the Cornell room -- runs that leaf and then the other: two ballots up front, one wave-uniform branch, and no
 *     bookkeeping of turns.
 *   - Any other wave runs the leaves in up to four turns: left then right for the lanes that pop the left child first,
 *     right then left for the others; a turn no lane takes is skipped by one ballot. The groups are disjoint, so each
 *     lane sees its two leaves in the reference's order. */
template <bool PRIM, int A>
__device__ __forceinline__ void tiny_leaves(const Ray& ray, gtri_ptr recs, const TinyRanges& g, const TinyLane& t,
                                            float& rt, uint32_t& prim)
{
    constexpr uint32_t kBytes = PRIM ? kPrimPairRecordBytes : kPairRecordBytes;
    const WCPT_GLOBAL char* pbase = reinterpret_cast<const WCPT_GLOBAL char*>(recs);
    uint32_t rb = take_bits(rt), tag = kNoTag;
    SharedPair sp;
    sp.off = kNoTag;
    sp.have = false;
    sp.ph.t = bc2(0.0f);
    sp.ph.hit0 = sp.ph.hit1 = false;
    if (!g.two) {
        if (__builtin_amdgcn_ballot_w64(t.in) != 0ull) tiny_leaf<PRIM, A>(ray, pbase, g.k0L, g.kendL, t.in, rb, tag, sp);
    } else {
        sp.off = tiny_shared_offset<kBytes>(g.k0L, g.kendL, g.k0R, g.kendR);
        const unsigned long long mIn = __builtin_amdgcn_ballot_w64(t.in);
        const unsigned long long mLeft = __builtin_amdgcn_ballot_w64(t.in && t.c.leftFirst);
        if (mLeft == mIn || mLeft == 0ull) {
            /* the lanes inside the root agree on the order (none inside: both leaves are skipped below) */
            const bool rightFirst = mLeft == 0ull; /* wave-uniform */
            const bool passA = rightFirst ? t.c.passR : t.c.passL, passB = rightFirst ? t.c.passL : t.c.passR;
            const float a0 = rightFirst ? t.c.r0 : t.c.l0, b0 = rightFirst ? t.c.l0 : t.c.r0;
            bool visit = t.in && passA && !(a0 > __uint_as_float(rb + 1u));
            if (__builtin_amdgcn_ballot_w64(visit) != 0ull)
                tiny_leaf<PRIM, A>(ray, pbase, rightFirst ? g.k0R : g.k0L, rightFirst ? g.kendR : g.kendL, visit, rb, tag, sp);
            visit = t.in && passB && !(b0 > __uint_as_float(rb + 1u));
            if (__builtin_amdgcn_ballot_w64(visit) != 0ull)
                tiny_leaf<PRIM, A>(ray, pbase, rightFirst ? g.k0L : g.k0R, rightFirst ? g.kendL : g.kendR, visit, rb, tag, sp);
        } else {
#pragma clang loop unroll(disable)
            for (uint32_t i = 0; i < 4u; i++) {
                /* turn i: group i >> 1 (0: left-first lanes), position i & 1 (0: the lane's near child); the right leaf
                 * iff group and position differ */
                const bool right = ((i >> 1) ^ (i & 1u)) != 0u;
                const bool visit = t.in && (t.c.leftFirst == (i < 2u)) && (right ? t.c.passR : t.c.passL) &&
                                   !((right ? t.c.r0 : t.c.l0) > __uint_as_float(rb + 1u));
                if (__builtin_amdgcn_ballot_w64(visit) == 0ull) continue;
                tiny_leaf<PRIM, A>(ray, pbase, right ? g.k0R : g.k0L, right ? g.kendR : g.kendL, visit, rb, tag, sp);
            }
        }
    }
    if (tag != kNoTag) prim = 3u * (2u * (tag / kBytes) + (tag & 1u));
    rt = __uint_as_float(rb + 1u);
}

/* The draw's whole traversal for a tiny tree. */
template <int A>
__device__ __forceinline__ void tiny_walk(const Ray& ray, const DrawGeom& g, bool primary, float& rt, uint32_t& prim)
{
    const NodeV root = load_node_const(g.bvh, 0);
    TinyLane t;
    float c0, c1;
    node_box(ray, root, c0, c1);
    t.in = root_survives(c0, c1, rt);
    t.c = ChildPair{false, false, false, 0.0f, 0.0f};
    uint32_t firstL = root.b.z, countL = root.b.w, firstR = 0u, countR = 0u; /* a root leaf: the "left" one */
    TinyRanges r;
    r.two = root.b.w == 0u;
    if (r.two) { /* wave-uniform: interior_step on the two leaves */
        const NodeV L = load_node_const(g.bvh, root.b.z);
        const NodeV R = load_node_const(g.bvh, root.b.z + 1u);
        /* A box whose six bound words are the bits of one already tested has that one's slab distances: node_box is a
         * function of the ray and those words alone. Midpoint leaves over a room's walls both span the whole room, which
         * is the root's box, so the Cornell walk makes one slab test per segment instead of three. The nodes are in
         * SGPRs; the compares are scalar and the branches wave-uniform. */
        float l0, l1, r0, r1;
        if (same_box_bits(L, root)) {
            l0 = c0;
            l1 = c1;
        } else {
            node_box(ray, L, l0, l1);
        }
        if (same_box_bits(R, root)) {
            r0 = c0;
            r1 = c1;
        } else if (same_box_bits(R, L)) {
            r0 = l0;
            r1 = l1;
        } else {
            node_box(ray, R, r0, r1);
        }
        t.c = child_pair(l0, l1, r0, r1);
        firstL = L.b.z;
        countL = L.b.w;
        firstR = R.b.z;
        countR = R.b.w;
    }
    /* mk_tiny_rule.h: every leaf starts on a triangle boundary, inside the records */
    r.k0L = __builtin_amdgcn_readfirstlane(firstL / 3u);
    r.kendL = r.k0L + __builtin_amdgcn_readfirstlane((countL + 2u) / 3u);
    r.k0R = __builtin_amdgcn_readfirstlane(firstR / 3u);
    r.kendR = r.k0R + __builtin_amdgcn_readfirstlane((countR + 2u) / 3u);
    if (primary && g.ptris != nullptr)
        tiny_leaves<true, A>(ray, g.ptris, r, t, rt, prim);
    else
        tiny_leaves<false, A>(ray, g.tris, r, t, rt, prim);
}

/* Intersect (pathTracer.comp:135-211) of the one draw with a tiny tree: intersect<..., SINGLE>'s sphere loop, the walk
 * in place of the traversal loop, and the same epilogue. */
template <int A>
__device__ __forceinline__ Hit tiny_intersect(const Ray& ray, const wcpt_scene_data& sd,
                                              const wcpt_sphere* __restrict__ spheres,
                                              const wcpt_draw_command* __restrict__ draws,
                                              const uint64_t* __restrict__ tri_records, bool primary)
{
    float rt = kInfinity;
    uint32_t prim = kNoPrim;
    sphere_loop<A>(ray, sd.sphereCount, spheres, rt, prim);
    const DrawGeom g = draw_geom<true>(draws, tri_records, 0);
    tiny_walk<A>(ray, g, primary, rt, prim);
    return resolve_hit<kShadeA<A>>(ray, rt, prim, 0u, spheres, draws, tri_records);
}

} // namespace wcpt::dev

#endif /* WCPT_PT_TINY_H */
