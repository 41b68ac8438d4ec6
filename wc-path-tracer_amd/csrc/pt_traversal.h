/* pt_traversal.h -- Intersect (pathTracer.comp:135-211) for the megakernel: a draw's geometry, the leaf, interior, pop
 * and root steps, the traversal loop and the hit epilogue. Part of pt_device.h. (The walk of a tiny tree: pt_tiny.h.) */
#ifndef WCPT_PT_TRAVERSAL_H
#define WCPT_PT_TRAVERSAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wcpt.h"
#include "frame_prep.h"
#include "pt_counters.h"
#include "pt_geometry.h"
#include "pt_math.h"
#include "primary_record.h"

namespace wcpt::dev {

/* Closest-hit record during traversal: (t, primitive) only; the winner's normal and material are rebuilt
 * once afterwards (resolve_hit) with the reference's expressions, which gives the values the reference
 * computes at each update (:145, :173) without paying a normalize per closer hit. */

/* Geometric normal of the triangle at index positions prim..prim+2 of draw `draw` (:173): from its single record
 * when the triangle starts on a triangle boundary inside the records (the record was derived from exactly these
 * three indices), else recomputed from the index and vertex buffers with the same expression. */
template <int A = kArithExact>
__device__ __forceinline__ f3 triangle_normal(uint32_t prim, uint32_t draw, const wcpt_draw_command* __restrict__ draws,
                                              const uint64_t* __restrict__ tri_records)
{
    const uint32_t k = prim / 3u;
    if (tri_records && k * 3u == prim && k < (uint32_t)tri_records[kTriTableWords * draw + kTriWordCount]) {
        const gtri_ptr t = (gtri_ptr)(uintptr_t)tri_records[kTriTableWords * draw + kTriWordSingles];
        const v4f r2 = t[3ull * k + 2u];
        return mk3(r2.y, r2.z, r2.w);
    }
    const TriE e = tri_from_indices(as_u32(draws[draw].indexBuffer), as_f32(draws[draw].vertexBuffer), prim,
                                    tri_records ? draw_vertex_count(tri_records, draw) : 0xFFFFFFFFu);
    return normalize_a<A>(cross_a<A>(e.e1, e.e2));
}

/* Intersect epilogue (:204-208) for winner `prim` (kNoPrim, kSpherePrim | sphere, or the index position of
 * a triangle of draw `draw`) at distance t. */
template <int A = kArithExact>
__device__ __forceinline__ Hit resolve_hit(const Ray& ray, float t, uint32_t prim, uint32_t draw,
                                           const wcpt_sphere* __restrict__ spheres,
                                           const wcpt_draw_command* __restrict__ draws,
                                           const uint64_t* __restrict__ tri_records)
{
    Hit h;
    h.t = t;
    h.hit = prim != kNoPrim;
    h.front = false;
    h.material = 0;
    h.normal = mk3(0.0f, 0.0f, 0.0f);
    if (h.hit) {
        if (prim & kSpherePrim) {
            const wcpt_sphere& s = spheres[prim & ~kSpherePrim];
            const f3 c = mk3(s.position[0], s.position[1], s.position[2]);
            const f3 ph = axpy_a<A>(ray.origin, ray.direction, t);
            h.normal = div3_a<A>(ph - c, s.radius);                /* :145 */
            h.material = s.material;
        } else {
            h.normal = triangle_normal<A>(prim, draw, draws, tri_records); /* :173, material 0 (:175) */
        }
        h.front = dot_a<A>(ray.direction, h.normal) < 0.0f;
        if (!h.front) h.normal = h.normal * -1.0f;
    }
    h.p = axpy_a<A>(ray.origin, ray.direction, t);                    /* :205 */
    return h;
}

/* One draw command's geometry (pathTracer.comp:152-156 and the derived records of its table entry). */
struct DrawGeom {
    gnode_ptr bvh;
    gu32_ptr indices;
    gf32_ptr vertices;
    gtri_ptr tris;  /* pair records (PAIRS) or single records */
    gtri_ptr ptris; /* primary-ray pair records (PAIRS, when the runtime built them; table word 4) or null */
    uint32_t ntri;
    uint32_t nvert; /* vertex count bound of the index path (draw_vertex_count) */
    bool packed; /* stack entries carry (left, count): kTriFlagPackedRefs */
};
template <bool PAIRS>
__device__ __forceinline__ DrawGeom draw_geom(const wcpt_draw_command* __restrict__ draws,
                                              const uint64_t* __restrict__ tri_records, uint32_t i)
{
    DrawGeom g;
    g.bvh = as_nodes(draws[i].bvhBuffer);
    g.indices = as_u32(draws[i].indexBuffer);
    g.vertices = as_f32(draws[i].vertexBuffer);
    g.tris = (gtri_ptr)(uintptr_t)tri_records[kTriTableWords * i + (PAIRS ? kTriWordPairs : kTriWordSingles)];
    g.ptris = PAIRS ? (gtri_ptr)(uintptr_t)tri_records[kTriTableWords * i + kTriWordPrimary] : nullptr;
    g.ntri = (uint32_t)tri_records[kTriTableWords * i + kTriWordCount];
    g.nvert = draw_vertex_count(tri_records, i);
    g.packed = (tri_records[kTriTableWords * i + kTriWordFlags] & kTriFlagPackedRefs) != 0u;
    return g;
}

/* The pair-record part of a leaf (:164-178): triangles [k0, kend) in pair records (2j, 2j+1), from `recs` (pair
 * records, or primary-ray pair records when PRIM). A leaf that starts in the second slot of a pair tests that pair
 * for its first triangle, then whole pairs, then possibly the first slot of a last pair -- no per-iteration slot
 * checks; applied in index order, strict <. UNIFORM: lanes of a coherent wave walk the whole pairs with scalar loads
 * (the record base must be wave-uniform). */
/* The pair record last tested for a peeled (odd-boundary) triangle in this segment: a leaf that ends in slot 0 of a pair
 * and the leaf that starts in its slot 1 (two 17-triangle midpoint leaves share the pair (16, 17)) both need that
 * record's test. Its byte offset with the two acceptance bits in bits 0-1, and both t: the second leaf reuses the
 * values the first computed -- the same test of the same ray on the same record -- and still applies them against
 * its own rec.t in its own order. Reset per segment and per draw (the offsets are relative to a draw's records). */
struct PeelCache { uint32_t tag; v2f t; };
constexpr uint32_t kNoPeel = 0xFFFFFFFFu;
/* Take the pair's triangles in reference order (2j, then 2j+1; each iff accepted with t < rec.t, strict):
 * the winner is tagged with the record offset (+1 for the second).
 * rb = bits(rec.t) - 1 (take_bits); hit0/hit1 are the acceptance without t > 0 */
__device__ __forceinline__ void pair_take_bits(const PairHit& ph, uint32_t off, uint32_t& rb, uint32_t& tag)
{
    const uint32_t b0 = take_bits(ph.t.x), b1 = take_bits(ph.t.y);
    if (ph.hit0 && b0 < rb) { rb = b0; tag = off; }
    if (ph.hit1 && b1 < rb) { rb = b1; tag = off + 1u; }
}
template <bool COUNT, bool DIAG, bool UNIFORM, bool PRIM, int A = kArithExact>
__device__ __forceinline__ void pair_leaf(const Ray& ray, gtri_ptr recs, uint32_t k0, uint32_t kend, float& rt,
                                          uint32_t& prim, Counters& cnt, PeelCache& pc)
{
    constexpr uint32_t kBytes = PRIM ? kPrimPairRecordBytes : kPairRecordBytes;
    const WCPT_GLOBAL char* pbase = reinterpret_cast<const WCPT_GLOBAL char*>(recs);
    auto test_at = [&](uint32_t off) {
        if constexpr (PRIM) return rayTrianglePairP<A>(ray, load_pairP_at(pbase, off));
        else return rayTrianglePair<A>(ray, load_pair_at(pbase, off));
    };
    /* the peeled pair at `off`, through the per-segment cache */
    auto peeled_at = [&](uint32_t off) {
        PairHit ph;
        if ((pc.tag & ~3u) == off) {
            ph.t = pc.t;
            ph.hit0 = (pc.tag & 1u) != 0u;
            ph.hit1 = (pc.tag & 2u) != 0u;
        } else {
            ph = test_at(off);
            pc.tag = off | (ph.hit0 ? 1u : 0u) | (ph.hit1 ? 2u : 0u);
            pc.t = ph.t;
        }
        return ph;
    };
    uint32_t rb = take_bits(rt); /* rec.t as bits - 1 through the leaf (take_bits) */
    uint32_t k = k0;
    if (k & 1u) {
        const PairHit ph = peeled_at((k >> 1) * kBytes);
        count_tri<COUNT, DIAG>(cnt);
        if (ph.hit1 && take_bits(ph.t.y) < rb) { rb = take_bits(ph.t.y); prim = 3u * k; }
        k++;
    }
    /* whole pairs: one 32-bit byte-offset induction variable from the draw's record base, and the winner recorded
     * as a tag -- the pair's offset for its first triangle, offset + 1 for its second -- decoded into the index
     * position once per leaf */
    const uint32_t kfull = kend & ~1u;
    const uint32_t offEnd = (kfull >> 1) * kBytes;
    uint32_t off = (k >> 1) * kBytes, tag = kNoTag;
    if (UNIFORM) {
        /* Lanes whose whole-pair range equals the first active lane's (in a coherent wave: all of them) read the
         * records at wave-uniform offsets with scalar loads: they go through the scalar cache (no per-lane
         * addresses, no vector-memory return of 64 copies of the record) and the packed-FP32 instructions take the
         * record straight from SGPRs (c2 -6 %). The other lanes take the per-lane loop below. */
        const uint32_t offU = __builtin_amdgcn_readfirstlane(off);
        const uint32_t endU = __builtin_amdgcn_readfirstlane(offEnd);
        /* tested through an opaque value: a plain `off == offU` lets the compiler substitute the equal per-lane
         * value back into the loads */
        uint32_t diff = (off ^ offU) | (offEnd ^ endU);
        asm volatile("" : "+v"(diff));
        if (diff == 0u) {
            /* the loop counter itself in an SGPR (offU..endU): no per-lane offset arithmetic (70 -> 68 VALU per
             * pair, c2 -1.7 %). A wave-uniform loop like this one was mis-compiled inside the old nested draw loop;
             * in the flat traversal loop it is correct (tools/stack_probe.py) */
            for (uint32_t o = offU; o < endU; o += kBytes) {
                PairHit ph;
                if constexpr (PRIM) {
                    const TriPairP p = load_pairP_const(pbase, o);
                    v2f px, py, pz;
                    const v2f det = pairP_det<A>(ray, p, px, py, pz);
                    if (__builtin_amdgcn_ballot_w64(pairP_may_take(p, det)) == 0ull) {
                        /* no lane can take either triangle (t <= 0 or NaN for all): the reference's tests still
                         * ran (and are counted), and none would change rec.t */
                        count_tri<COUNT, DIAG>(cnt);
                        count_tri<COUNT, DIAG>(cnt);
                        continue;
                    }
                    ph = pairP_finish<A>(ray, p, px, py, pz, det);
                } else {
                    ph = rayTrianglePair<A>(ray, load_pair_const(pbase, o));
                }
#if WCPT_DUP_PAIR
                {
                    Ray r2 = ray;
                    r2.direction.x = launder(r2.direction.x);
                    PairHit p2;
                    if constexpr (PRIM) p2 = rayTrianglePairP<A>(r2, load_pairP_const(pbase, o));
                    else p2 = rayTrianglePair<A>(r2, load_pair_const(pbase, o));
                    sink(p2.t.x + p2.t.y);
                    sink_u((p2.hit0 ? 1u : 0u) | (p2.hit1 ? 2u : 0u));
                }
#endif
                count_tri<COUNT, DIAG>(cnt);
                count_tri<COUNT, DIAG>(cnt);
                pair_take_bits(ph, o, rb, tag);
            }
            off = offEnd;
        }
    }
    for (; off < offEnd; off += kBytes) {
        const PairHit ph = test_at(off);
#if WCPT_DUP_PAIR
        if constexpr (!PRIM) {
            Ray r2 = ray;
            r2.origin.x = launder(r2.origin.x);
            const PairHit p2 = rayTrianglePair<A>(r2, load_pair_at(pbase, off));
            sink(p2.t.x + p2.t.y);
            sink_u((p2.hit0 ? 1u : 0u) | (p2.hit1 ? 2u : 0u));
        }
#endif
        count_tri<COUNT, DIAG>(cnt);
        count_tri<COUNT, DIAG>(cnt);
        pair_take_bits(ph, off, rb, tag);
    }
    if (tag != kNoTag) prim = 3u * (2u * (tag / kBytes) + (tag & 1u));
    if (k < kfull) k = kfull;
    if (k < kend) {
        const PairHit ph = peeled_at((k >> 1) * kBytes);
        count_tri<COUNT, DIAG>(cnt);
        if (ph.hit0 && take_bits(ph.t.x) < rb) { rb = take_bits(ph.t.x); prim = 3u * k; }
    }
    rt = __uint_as_float(rb + 1u);
}

/* Leaf (:164-178): every triangle of the leaf at index positions [curLeft, curLeft + curCount), in index order,
 * taken iff accepted with t < rec.t (strict). UNIFORM: the leaf's whole pairs may be read with scalar loads (the
 * draw's record base must then be wave-uniform). primary: the segment is a sample's first (origin = the camera,
 * wave-uniform), whose leaves are tested from the primary-ray pair records when the draw has them. */
template <bool COUNT, bool DIAG, bool PAIRS, bool UNIFORM, int A = kArithExact>
__device__ __forceinline__ void leaf_step(const Ray& ray, const DrawGeom& g, uint32_t curLeft, uint32_t curCount,
                                          float& rt, uint32_t& prim, Counters& cnt, bool primary, PeelCache& pc)
{
    const uint32_t k0 = leaf_record(curLeft, curCount, g.ntri);
    if (PAIRS && k0 != kNoRecord) {
        const uint32_t kend = k0 + (curCount + 2u) / 3u;
        if (primary && g.ptris != nullptr)
            pair_leaf<COUNT, DIAG, UNIFORM, true, A>(ray, g.ptris, k0, kend, rt, prim, cnt, pc);
        else
            pair_leaf<COUNT, DIAG, UNIFORM, false, A>(ray, g.tris, k0, kend, rt, prim, cnt, pc);
    } else {
        for (uint32_t k = 0, j = 0; k < curCount; k += 3, j++) {
            const uint32_t first = k + curLeft;
            const TriE tr = (!PAIRS && k0 != kNoRecord) ? load_tri(g.tris, k0 + j)
                                                        : tri_from_indices(g.indices, g.vertices, first, g.nvert);
            const float t = rayTriangleE<A>(ray, tr.a, tr.e1, tr.e2);
            count_tri<COUNT, DIAG>(cnt);
            if (t != -1.0f && t < rt) {
                rt = t;
                prim = first;
            }
        }
    }
    phase_mark(cnt, 3);
}

/* Interior (:179-199): fetch both children (64 contiguous bytes), test both boxes, push the farther child if it
 * passes, and return true with the cursor on the nearer child if that one passes and is not culled by rec.t. */
template <bool COUNT, bool DIAG, class Stack>
__device__ __forceinline__ bool interior_step(const Ray& ray, const DrawGeom& g, Stack& stk, uint32_t& curLeft,
                                              uint32_t& curCount, float rt, Counters& cnt, bool& overflow,
                                              RefStack& rf)
{
    const NodeV L = load_node(g.bvh, curLeft);
    const NodeV R = load_node(g.bvh, curLeft + 1);
    const ChildPair c = child_pair(ray, L, R);
#if WCPT_DUP_BOX
    {
        Ray r2 = ray;
        r2.origin.x = launder(r2.origin.x);
        r2.origin.y = launder(r2.origin.y);
        r2.origin.z = launder(r2.origin.z);
        float a0, a1, b0, b1;
        node_box(r2, L, a0, a1);
        node_box(r2, R, b0, b1);
        sink(a0 + a1 + b0 + b1);
    }
#endif
    if (COUNT) {
        cnt.interior_visits++;
        cnt.node_pops += 2;
        simd_step<DIAG>(cnt.wave_int, cnt.lane_int);
    }
    const uint32_t farIdx = c.leftFirst ? curLeft + 1 : curLeft;
    const NodeV& F = c.leftFirst ? R : L;
    if (c.passFar() && !stk.push(node_ref(g.packed, farIdx, F.b.z, F.b.w), c.farT0())) overflow = true;
    ref_interior<COUNT>(rf, c.passFar(), cnt);
    phase_mark(cnt, 2);
    if (c.passNear() && !(c.nearT0() > rt)) {
        const NodeV& N = c.leftFirst ? L : R;
        curLeft = N.b.z;
        curCount = N.b.w;
        return true;
    }
    return false;
}

/* Pop (:157-162): the next deferred node whose box entry distance is not beyond rec.t; false when none is left. */
template <bool COUNT, class Stack>
__device__ __forceinline__ bool pop_step(const DrawGeom& g, Stack& stk, uint32_t& curLeft, uint32_t& curCount, float rt,
                                         Counters& cnt, RefStack& rf)
{
    bool found = false;
    while (!stk.empty()) {
        uint32_t ni;
        float t0;
        stk.pop(ni, t0);
        ref_pop<COUNT>(rf);
        if (t0 > rt) continue;
        const uint2 lc = node_ref_lc(g.packed, g.bvh, ni);
        curLeft = lc.x;
        curCount = lc.y;
        found = true;
        break;
    }
    phase_mark(cnt, 2);
    return found;
}

/* The root of draw d (:152-162): pushed untested, popped and tested. Returns true with the cursor on the root when it
 * survives the cull. */
template <bool COUNT>
__device__ __forceinline__ bool root_step(const Ray& ray, const DrawGeom& g, float rt, uint32_t& curLeft,
                                          uint32_t& curCount, Counters& cnt, RefStack& rf)
{
    if (COUNT) { cnt.draw_fetches++; cnt.node_pops++; }
    ref_root<COUNT>(rf, cnt);
    const NodeV cur = load_node(g.bvh, 0);
    if (!root_survives(ray, cur, rt)) return false;
    curLeft = cur.b.z;
    curCount = cur.b.w;
    return true;
}

/* pathTracer.comp:135-211. PAIRS: leaf tests on pair records (else single records).
 *
 * SINGLE (drawCommandCount == 1, the reference's own case, PathTracingRenderer.jai:251): the draw's geometry is
 * kernel-uniform and its traversal runs once, without the draw loop. Otherwise the draws are walked inside the one
 * traversal loop (the next draw starts when the stack of the current one is exhausted), like wf_trace: the nested
 * form -- a loop over draws containing the divergent traversal loops, inside the divergent bounce loop -- is
 * mis-compiled by this toolchain whenever the traversal grows (a DIAG build or the scalar-load leaf loop on the
 * atrium overflowed the stack, tools/stack_probe.py), while this flat form is not. */
/* Every sample of a pixel starts with the same primary ray (pathTracer.comp:302, :309-310), so its Intersect record is
 * the same too: the megakernel keeps sample 0's and later samples resolve their primary segment from it (render
 * builds for samples > 1 only, a separate instantiation -- keeping the record costs the one-sample kernel 20 VGPRs --
 * and never the COUNT build, which traces every segment as the reference does for the exact counters). */
/* Primary cache (WCPT_OPTION_PRIMARY_CACHE): the resolved primary segment kept from one frame to the next while camera,
 * frame geometry and scene stand still (primary_cache_key.h has the rule, primary_record.h the entry: the primary ray's
 * direction and resolve_hit's result for it, eight u32 per pixel, tile-major, the same for one draw and for several).
 * Render builds only; PC is the launch's mode: kPrimCacheWrite traces as usual and stores the lane's entry after the
 * primary segment of sample 0 (TraceRay; `pcache` is the tile's first entry, wave-uniform, so a wave touches one
 * contiguous run whatever the tile order or pipe; a miss has t = kInfinity); kPrimCacheRead never calls intersect for a
 * primary segment: segment 0 of every sample is path_shade on the loaded entry (TraceRay), so neither the primary
 * direction, its reciprocal, resolve_hit nor the primary-only leaf code (primary pair records, sign pre-reject) is in
 * that kernel at all. */
constexpr int kPrimCacheNone = 0, kPrimCacheWrite = 1, kPrimCacheRead = 2;
/* the lane's entry among its tile's */
__device__ __forceinline__ uint32_t* prim_cache_lane(uint32_t* tile_records)
{
    return tile_records + primary_record_word(0u, threadIdx.x);
}
/* The entry of a resolved primary segment (direction `dir`, resolve_hit's `h`) and back; h.p is the reader's own
 * axpy_a<A>(origin, dir, t), the expression resolve_hit ends with. Two 16-byte accesses per lane. */
__device__ __forceinline__ void prim_cache_store(uint32_t* __restrict__ tile_records, f3 dir, const Hit& h)
{
    PrimaryRecord r;
    r.dir[0] = __float_as_uint(dir.x);
    r.dir[1] = __float_as_uint(dir.y);
    r.dir[2] = __float_as_uint(dir.z);
    r.normal[0] = __float_as_uint(h.normal.x);
    r.normal[1] = __float_as_uint(h.normal.y);
    r.normal[2] = __float_as_uint(h.normal.z);
    r.t = __float_as_uint(h.t);
    r.material = h.material;
    r.hit = h.hit;
    r.front = h.front;
    uint32_t w[kPrimRecWords];
    primary_record_pack(r, w);
    uint4* const pl = reinterpret_cast<uint4*>(prim_cache_lane(tile_records));
    pl[0] = make_uint4(w[0], w[1], w[2], w[3]);
    pl[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
struct PrimEntry { uint4 lo, hi; }; /* an entry as loaded: unpacked at its use, so nothing of it lives longer than it must */
__device__ __forceinline__ PrimEntry prim_cache_load(const uint32_t* __restrict__ tile_records)
{
    const uint4* const pl = reinterpret_cast<const uint4*>(prim_cache_lane(const_cast<uint32_t*>(tile_records)));
    PrimEntry e;
    e.lo = pl[0];
    e.hi = pl[1];
    return e;
}
template <int A>
__device__ __forceinline__ Hit prim_entry_hit(const PrimEntry& e, f3 origin, f3& dir)
{
    const uint32_t w[kPrimRecWords] = {e.lo.x, e.lo.y, e.lo.z, e.lo.w, e.hi.x, e.hi.y, e.hi.z, e.hi.w};
    const PrimaryRecord r = primary_record_unpack(w);
    dir = mk3(__uint_as_float(r.dir[0]), __uint_as_float(r.dir[1]), __uint_as_float(r.dir[2]));
    Hit h;
    h.t = __uint_as_float(r.t);
    h.hit = r.hit;
    h.front = r.front;
    h.material = r.material;
    h.normal = mk3(__uint_as_float(r.normal[0]), __uint_as_float(r.normal[1]), __uint_as_float(r.normal[2]));
    h.p = axpy_a<A>(origin, dir, h.t); /* :205, resolve_hit's */
    return h;
}
template <bool COUNT, bool DIAG, bool PAIRS, bool SINGLE, class Stack, int A = kArithExact>
__device__ __forceinline__ Hit intersect(const Ray& ray, const wcpt_scene_data& sd, const wcpt_sphere* __restrict__ spheres,
                                         const wcpt_draw_command* __restrict__ draws,
                                         const uint64_t* __restrict__ tri_records, Stack& stk,
                                         Counters& cnt, bool& overflow, bool primary, float4& prim_rec,
                                         bool reuse_primary)
{
    float rt = kInfinity;
    uint32_t prim = kNoPrim, primDraw = 0;
    /* a later sample's primary segment */
    if (!COUNT && reuse_primary) {
        rt = prim_rec.x;
        prim = __float_as_uint(prim_rec.y);
        primDraw = __float_as_uint(prim_rec.z);
    } else {
        if (COUNT) {
            cnt.segments++;
            simd_step<DIAG>(cnt.wave_seg, cnt.lane_seg);
        }

        sphere_loop<A>(ray, sd.sphereCount, spheres, rt, prim);
        if (COUNT) cnt.sphere_tests += sd.sphereCount;
#if WCPT_DUP_SPHERES
        {
            Ray r2 = ray;
            r2.origin.x = launder(r2.origin.x);
            r2.direction.x = launder(r2.direction.x);
            float rt2 = kInfinity;
            uint32_t p2 = 0;
            for (uint32_t i = 0; i < sd.sphereCount; i++) {
                const wcpt_sphere& s = spheres[i];
                const float tr = raySphereNear(r2, mk3(s.position[0], s.position[1], s.position[2]), s.radius);
                if (tr > 0.0f && tr < rt2) { rt2 = tr; p2 = i; }
            }
            sink(rt2);
            sink_u(p2);
        }
#endif
        phase_mark(cnt, 1);

        uint32_t curLeft = 0, curCount = 0;
        PeelCache pc;
        pc.tag = kNoPeel;
        pc.t = bc2(0.0f);
        RefStack rf;
        if constexpr (SINGLE) {
            const DrawGeom g = draw_geom<PAIRS>(draws, tri_records, 0);
            /* one traversal step per iteration as sequential ifs on the lane's mode (pop -> interior -> leaf), like
             * wf_trace: a lane that pops an interior node visits it in the same iteration, one that descends into a
             * leaf tests it in the same iteration */
            enum : uint32_t { kInterior = 0, kLeaf = 1, kPop = 2, kDone = 3 };
            uint32_t mode = kDone;
            /* (a tiny tree's render -- mk_tiny_rule.h mk_tiny_kernels -- does not come here: pt_mk_tiny.hip) */
            if (sd.drawCommandCount != 0u && root_step<COUNT>(ray, g, rt, curLeft, curCount, cnt, rf)) {
                stk.reset();
                mode = curCount > 0 ? kLeaf : kInterior;
            }
            while (mode != kDone) {
                if (mode == kPop) {
                    /* one stack entry per iteration (no inner pop loop): a culled entry (:162) keeps the lane popping */
                    if (stk.empty()) {
                        mode = kDone;
                    } else {
                        uint32_t ni;
                        float t0;
                        stk.pop(ni, t0);
                        ref_pop<COUNT>(rf);
                        if (!(t0 > rt)) {
                            const uint2 lc = node_ref_lc(g.packed, g.bvh, ni);
                            curLeft = lc.x;
                            curCount = lc.y;
                            mode = curCount > 0 ? kLeaf : kInterior;
                        }
                    }
                    phase_mark(cnt, 2);
                }
                if (mode == kInterior)
                    mode = interior_step<COUNT, DIAG>(ray, g, stk, curLeft, curCount, rt, cnt, overflow, rf)
                               ? (curCount > 0 ? kLeaf : kInterior) : kPop;
                if (mode == kLeaf) {
                    leaf_step<COUNT, DIAG, PAIRS, true, A>(ray, g, curLeft, curCount, rt, prim, cnt, primary, pc);
                    mode = kPop;
                }
            }
        } else {
            uint32_t d = 0;
            DrawGeom g;
            float rt_before = rt;
            /* first draw (from d on) whose root survives the cull */
            auto start_draw = [&]() {
                for (; d < sd.drawCommandCount; d++) {
                    g = draw_geom<PAIRS>(draws, tri_records, d);
                    rt_before = rt;
                    if (root_step<COUNT>(ray, g, rt, curLeft, curCount, cnt, rf)) {
                        stk.reset();
                        pc.tag = kNoPeel; /* offsets of another draw's records */
                        return true;
                    }
                }
                return false;
            };
            bool active = start_draw();
            while (active) {
                if (curCount > 0) {
                    leaf_step<COUNT, DIAG, PAIRS, false, A>(ray, g, curLeft, curCount, rt, prim, cnt, primary, pc);
                } else if (interior_step<COUNT, DIAG>(ray, g, stk, curLeft, curCount, rt, cnt, overflow, rf)) {
                    continue;
                }
                if (pop_step<COUNT>(g, stk, curLeft, curCount, rt, cnt, rf)) continue;
                if (rt != rt_before) primDraw = d; /* this draw lowered rt: it owns prim */
                d++;
                active = start_draw();
            }
        }
    }
    if (!COUNT && primary && sd.samples > 1u) prim_rec = make_float4(rt, __uint_as_float(prim), __uint_as_float(primDraw), 0.0f);
    if (COUNT && prim != kNoPrim) cnt.hits++;
    ref_segment_end<COUNT>(cnt);
    const Hit hit = resolve_hit<kShadeA<A>>(ray, rt, prim, primDraw, spheres, draws, tri_records);
    phase_mark(cnt, 4);
    return hit;
}

/* The closest hit of intersect without its epilogue, for a caller that needs the winner's identity (pt_primary.hip): the
 * sphere loop, then every draw in order on the multi-draw loop above -- the same steps in the same order, so rt, prim
 * (kNoPrim, kSpherePrim | sphere, or a triangle's index position) and primDraw are what intersect hands resolve_hit for
 * this ray. Exact arithmetic, no counting; `primary` as for leaf_step. `pairs` (kernel-uniform) is the frame plan's record
 * layout, a run-time switch here: every draw's table entry holds both layouts, both leaf forms give the same (rt, prim)
 * -- the same tests in the same order -- and the caller is one kernel for every plan. */
struct ClosestHit { float t; uint32_t prim, draw; };
template <class Stack>
__device__ __forceinline__ ClosestHit closest_hit(const Ray& ray, const wcpt_scene_data& sd,
                                                  const wcpt_sphere* __restrict__ spheres,
                                                  const wcpt_draw_command* __restrict__ draws,
                                                  const uint64_t* __restrict__ tri_records, Stack& stk, bool& overflow,
                                                  bool primary, bool pairs)
{
    float rt = kInfinity;
    uint32_t prim = kNoPrim, primDraw = 0;
    Counters cnt = {};
    sphere_loop<kArithExact>(ray, sd.sphereCount, spheres, rt, prim);
    uint32_t curLeft = 0, curCount = 0;
    PeelCache pc;
    pc.tag = kNoPeel;
    pc.t = bc2(0.0f);
    RefStack rf;
    uint32_t d = 0;
    DrawGeom g;
    float rt_before = rt;
    auto start_draw = [&]() {
        for (; d < sd.drawCommandCount; d++) {
            g = pairs ? draw_geom<true>(draws, tri_records, d) : draw_geom<false>(draws, tri_records, d);
            rt_before = rt;
            if (root_step<false>(ray, g, rt, curLeft, curCount, cnt, rf)) {
                stk.reset();
                pc.tag = kNoPeel;
                return true;
            }
        }
        return false;
    };
    bool active = start_draw();
    while (active) {
        if (curCount > 0) {
            if (pairs) leaf_step<false, false, true, false, kArithExact>(ray, g, curLeft, curCount, rt, prim, cnt, primary, pc);
            else leaf_step<false, false, false, false, kArithExact>(ray, g, curLeft, curCount, rt, prim, cnt, primary, pc);
        } else if (interior_step<false, false>(ray, g, stk, curLeft, curCount, rt, cnt, overflow, rf)) {
            continue;
        }
        if (pop_step<false>(g, stk, curLeft, curCount, rt, cnt, rf)) continue;
        if (rt != rt_before) primDraw = d; /* this draw lowered rt: it owns prim */
        d++;
        active = start_draw();
    }
    return {rt, prim, primDraw};
}

} // namespace wcpt::dev

#endif /* WCPT_PT_TRAVERSAL_H */
