/* pt_geometry.h -- rays and hits, BVH nodes and stack node references, the box, sphere and triangle tests, and the
 * derived triangle records with their loads. Part of pt_device.h. */
#ifndef WCPT_PT_GEOMETRY_H
#define WCPT_PT_GEOMETRY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wcpt.h"
#include "frame_prep.h"
#include "pt_math.h"

namespace wcpt::dev {

/* ---- pathTracer.comp:24-28, 50-58 ------------------------------------------------------------- */
struct Ray { f3 origin, direction, invDirection; };
struct Hit { f3 p, normal; float t; uint32_t material; bool hit, front; };

/* pathTracer.comp:97-108 — slab test; min/max are IEEE minNum/maxNum (v_min_f32 / v_max_f32). */
__device__ __forceinline__ void rayBox(const Ray& r, float mnx_, float mny_, float mnz_, float mxx_, float mxy_,
                                       float mxz_, float& t0, float& t1)
{
    const float bx = (mnx_ - r.origin.x) * r.invDirection.x;
    const float by = (mny_ - r.origin.y) * r.invDirection.y;
    const float bz = (mnz_ - r.origin.z) * r.invDirection.z;
    const float tx = (mxx_ - r.origin.x) * r.invDirection.x;
    const float ty = (mxy_ - r.origin.y) * r.invDirection.y;
    const float tz = (mxz_ - r.origin.z) * r.invDirection.z;
    const float mnx = fminf(tx, bx), mny = fminf(ty, by), mnz = fminf(tz, bz);
    const float mxx = fmaxf(tx, bx), mxy = fmaxf(ty, by), mxz = fmaxf(tz, bz);
    t0 = fmaxf(fmaxf(mnx, mny), fmaxf(mnx, mnz));
    t1 = fminf(fminf(mxx, mxy), fminf(mxx, mxz));
}

/* A BVH node (32 B) as two 16-byte loads: {min.xyz, max.x}, {max.yz, left, count}. */
struct NodeV { v4f a; v4u b; };
__device__ __forceinline__ NodeV load_node(gnode_ptr bvh, uint32_t i)
{
    const WCPT_GLOBAL v4f* p = reinterpret_cast<const WCPT_GLOBAL v4f*>(bvh + i);
    NodeV n;
    n.a = p[0];
    n.b = reinterpret_cast<const WCPT_GLOBAL v4u*>(p)[1];
    return n;
}
/* Node i at a wave-uniform index through the constant address space: scalar loads through the scalar cache, the node in
 * SGPRs (the BVH is read-only for the whole launch; load_pair_const has the same argument for the records). */
__device__ __forceinline__ NodeV load_node_const(gnode_ptr bvh, uint32_t i)
{
    typedef const __attribute__((address_space(4))) v4f* cv4f_ptr;
    typedef const __attribute__((address_space(4))) v4u* cv4u_ptr;
    const uintptr_t a = (uintptr_t)(bvh + i);
    NodeV n;
    n.a = ((cv4f_ptr)a)[0];
    n.b = ((cv4u_ptr)a)[1];
    return n;
}
/* The child pair (left, left + 1) of an interior node through a buffer resource over the BVH (draws whose BVH is a
 * known context buffer of < 2^24 nodes: table word 2's high half holds the node count): the four loads take one VGPR
 * byte offset (buffer_load_dwordx4 v_off, s[rsrc] offen offset:0/16/32/48) instead of two 64-bit lane addresses
 * (v_lshlrev_b64 + v_lshl_add_u64 each), and an index past the buffer reads a zero node instead of other memory.
 * Same bytes for every node in the buffer. */
constexpr int kBufferDword3 = 0x00020000; /* gfx9 raw buffer resource word 3 (composable_kernel's value for gfx9) */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t node_rsrc(gnode_ptr bvh, uint32_t nodes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)bvh, (short)0, (int)(nodes * 32u), kBufferDword3);
}
__device__ __forceinline__ void load_pair_rsrc(__amdgpu_buffer_rsrc_t r, uint32_t left, NodeV& L, NodeV& R)
{
    const int off = (int)(left << 5);
    L.a = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    L.b = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off + 16, 0, 0));
    R.a = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, off + 32, 0, 0));
    R.b = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off + 48, 0, 0));
}
/* (leftNodeOrTriangleIndex, triangleCount) of node i: bytes 24..31 */
__device__ __forceinline__ uint2 load_node_lc(gnode_ptr bvh, uint32_t i)
{
    const v2u v = reinterpret_cast<const WCPT_GLOBAL v2u*>(bvh + i)[3];
    return make_uint2(v.x, v.y);
}
/* Stack entry node references. Packed form (draws whose BVH has < 2^24 nodes and whose index count is < 2^24,
 * table flag kTriFlagPackedRefs): the deferred child's own (left, count) as (left << 8) | count when count < 255,
 * so that popping it needs no node fetch -- the pop path then has no dependent memory round trip; otherwise
 * (node index << 8) | 255 and the node's (left, count) is fetched at pop. Unpacked form: the node index. */
constexpr uint32_t kRefFetch = 255u;
__device__ __forceinline__ uint32_t node_ref(bool packed, uint32_t node_index, uint32_t left, uint32_t count)
{
    if (!packed) return node_index;
    return (count < kRefFetch && left < (1u << 24)) ? (left << 8) | count : (node_index << 8) | kRefFetch;
}
__device__ __forceinline__ uint2 node_ref_lc(bool packed, gnode_ptr bvh, uint32_t ref)
{
    if (!packed) return load_node_lc(bvh, ref);
    if ((ref & 255u) != kRefFetch) return make_uint2(ref >> 8, ref & 255u);
    return load_node_lc(bvh, ref >> 8);
}
/* The packed forms when every index and count fits (the wavefront fast layout: < 2^24 nodes and index positions,
 * every triangleCount < kRefFetch, kTriFlagSmallLeaves): no fetch case */
__device__ __forceinline__ uint32_t node_ref_small(uint32_t left, uint32_t count) { return (left << 8) | count; }
__device__ __forceinline__ uint2 node_ref_lc_small(uint32_t ref) { return make_uint2(ref >> 8, ref & 255u); }
__device__ __forceinline__ void node_box(const Ray& r, const NodeV& n, float& t0, float& t1)
{
    /* node = {min.xyz, max.x | max.yz, left, count} */
    rayBox(r, n.a.x, n.a.y, n.a.z, n.a.w, __uint_as_float(n.b.x), __uint_as_float(n.b.y), t0, t1);
}
/* The child-pair decision of an interior node (:179-199), the one definition of the megakernel's interior_step and tiny
 * walk (wf_trace keeps the same expressions as its own text, with the reason there): each child's box pass (the static
 * part of :162, t0 > t1 || t1 < 0, negated so that a NaN distance passes as it does in the reference) and entry distance
 * t0, and whether the reference pops the left child first (leftDist < rightDist: false on a NaN distance, where 0 * inf
 * arose on a slab plane). The images are bit-identical to the oracle only while these expressions are the oracle's;
 * selftest geometry fn 8 compares them with it word for word. */
struct ChildPair {
    bool leftFirst, passL, passR;
    float l0, r0; /* box entry distances of the left and the right child */
    __device__ __forceinline__ bool passNear() const { return leftFirst ? passL : passR; }
    __device__ __forceinline__ bool passFar() const { return leftFirst ? passR : passL; }
    __device__ __forceinline__ float nearT0() const { return leftFirst ? l0 : r0; }
    __device__ __forceinline__ float farT0() const { return leftFirst ? r0 : l0; }
};
/* The decision on the two boxes' slab distances (l0, l1) and (r0, r1): the tiny walk passes a box's distances on from
 * a node whose bound words are the same bits (pt_tiny.h tiny_walk) instead of evaluating node_box on them again. */
__device__ __forceinline__ ChildPair child_pair(float l0, float l1, float r0, float r1)
{
    const float leftDist = (l0 > 0.0f) ? l0 : l1;
    const float rightDist = (r0 > 0.0f) ? r0 : r1;
    ChildPair c;
    c.passL = !(l0 > l1 || l1 < 0.0f);
    c.passR = !(r0 > r1 || r1 < 0.0f);
    /* reference order: left popped first iff leftDist < rightDist */
    c.leftFirst = leftDist < rightDist;
    c.l0 = l0;
    c.r0 = r0;
    return c;
}
__device__ __forceinline__ ChildPair child_pair(const Ray& ray, const NodeV& L, const NodeV& R)
{
    float l0, l1, r0, r1;
    node_box(ray, L, l0, l1);
    node_box(ray, R, r0, r1);
    return child_pair(l0, l1, r0, r1);
}
/* The root's cull (:152-162): pushed untested, popped and tested against rec.t; whether it survives. On the root box's
 * slab distances (c0, c1), and on the node. */
__device__ __forceinline__ bool root_survives(float c0, float c1, float rt)
{
    return !(c0 > c1 || c1 < 0.0f || c0 > rt);
}
__device__ __forceinline__ bool root_survives(const Ray& ray, const NodeV& root, float rt)
{
    float c0, c1;
    node_box(ray, root, c0, c1);
    return root_survives(c0, c1, rt);
}
/* Whether two nodes' six bound words are the same bits, for nodes held in SGPRs (load_node_const): an integer compare on
 * the scalar unit, wave-uniform. Bitwise, so -0 against +0 and a NaN against anything are "different" and the caller
 * evaluates the box itself. */
__device__ __forceinline__ bool same_box_bits(const NodeV& a, const NodeV& b)
{
    auto u = [](float f) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(f)); };
    auto w = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    return ((u(a.a.x) ^ u(b.a.x)) | (u(a.a.y) ^ u(b.a.y)) | (u(a.a.z) ^ u(b.a.z)) | (u(a.a.w) ^ u(b.a.w)) |
            (w(a.b.x) ^ w(b.b.x)) | (w(a.b.y) ^ w(b.b.y))) == 0u;
}

/* pathTracer.comp:110-119, near root only (:141) */
template <int A = kArithExact>
__device__ __forceinline__ float raySphereNear(const Ray& r, f3 position, float radius)
{
    constexpr int S = kSphereA<A>;
    const f3 oc = r.origin - position;
    const float b = dot_a<S>(oc, r.direction);
    const float c = nmad_a<S>(dot_a<S>(oc, oc), radius, radius); /* dot(oc, oc) - radius * radius */
    const float t = madn_a<S>(b, b, c);                          /* b * b - c */
    if (t < 0.0f) return -1.0f;
    return -b - sqrt_a<S>(t);
}

/* The sphere loop of Intersect (pathTracer.comp:140-149) over spheres [0, count): the near root of each, accepted
 * iff 0 < t < rec.t, in sphere order. Two spheres are evaluated per step with packed
 * FP32 (v_pk_mul_f32 / v_pk_add_f32: per half exactly raySphereNear's binary32 operations), the square roots and
 * the ordered takes per sphere. */
constexpr uint32_t kNoPrim = 0xFFFFFFFFu, kSpherePrim = 0x80000000u;
template <int A = kArithExact>
__device__ __forceinline__ void sphere_loop(const Ray& r, uint32_t count, const wcpt_sphere* __restrict__ spheres,
                                            float& rt, uint32_t& prim)
{
    constexpr int S = kSphereA<A>;
    uint32_t i = 0;
    const v2f ox = {r.origin.x, r.origin.x}, oy = {r.origin.y, r.origin.y}, oz = {r.origin.z, r.origin.z};
    const v2f dx = {r.direction.x, r.direction.x}, dy = {r.direction.y, r.direction.y},
                dz = {r.direction.z, r.direction.z};
    for (; i + 1u < count; i += 2u) {
        const wcpt_sphere& s0 = spheres[i];
        const wcpt_sphere& s1 = spheres[i + 1u];
        const v2f cx = {s0.position[0], s1.position[0]}, cy = {s0.position[1], s1.position[1]},
                    cz = {s0.position[2], s1.position[2]}, rad = {s0.radius, s1.radius};
        const v2f ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;     /* oc = origin - position */
        const v2f b = dot2_a<S>(ocx, ocy, ocz, dx, dy, dz);        /* dot(oc, d) */
        const v2f c = nmad2_a<S>(dot2_a<S>(ocx, ocy, ocz, ocx, ocy, ocz), rad, rad); /* dot(oc, oc) - rad * rad */
        const v2f t = madn2_a<S>(b, b, c);                         /* b * b - c */
        /* b >= 0 (the centre is not ahead of the origin) gives -b - sqrt(t) <= 0 exactly, so RN of it is <= 0 and the
         * `t0 > 0` test below fails either way: the square root is skipped (NaN b still takes the full path) */
        const float t0 = (t.x < 0.0f || b.x >= 0.0f) ? -1.0f : -b.x - sqrt_a<S>(t.x);
        const float t1 = (t.y < 0.0f || b.y >= 0.0f) ? -1.0f : -b.y - sqrt_a<S>(t.y);
        if (t0 > 0.0f && t0 < rt) { rt = t0; prim = kSpherePrim | i; }
        if (t1 > 0.0f && t1 < rt) { rt = t1; prim = kSpherePrim | (i + 1u); }
    }
    for (; i < count; i++) {
        const wcpt_sphere& s = spheres[i];
        const float tempRec = raySphereNear<A>(r, mk3(s.position[0], s.position[1], s.position[2]), s.radius);
        if (tempRec > 0.0f && tempRec < rt) {
            rt = tempRec;
            prim = kSpherePrim | i;
        }
    }
}

/* The acceptance test of :132 without its `u <= 1` term, which the other terms imply: with v >= 0, u + v >= u
 * exactly, so the rounded sum RN(u + v) >= RN(u) = u (rounding is monotonic), and u + v <= 1 then gives u <= 1.
 * A NaN u or v fails `u >= 0` / `v >= 0` either way, and u = +inf fails `u + v <= 1`. Same decision, one
 * compare less per triangle. */
__device__ __forceinline__ bool accept_tri(float t, float u, float v, float uv)
{
    return t > 0.0f && u >= 0.0f && v >= 0.0f && uv <= 1.0f;
}

/* The same decision with one compare for u, v and u + v: t > 0 && minimum3(u, v, 1 - (u + v)) >= 0, where minimum3
 * is v_minimum3_f32 (IEEE 754-2019 minimum: NaN-propagating, -0 < +0). Equivalence: a NaN u or v makes u + v and
 * 1 - (u + v) NaN, so the minimum is NaN and the test fails, as `u >= 0` / `v >= 0` does; u = +inf with v = -inf
 * fails both ways (v < 0, and the NaN sum). For non-NaN values minimum3 >= 0 is u >= 0 && v >= 0 && w >= 0 (-0 counts
 * as >= 0 in both), and w = RN(1 - uv) >= 0 exactly when uv <= 1: uv <= 1 makes 1 - uv >= 0, whose rounding stays
 * >= 0; uv > 1 means uv >= 1 + 2^-23, so 1 - uv <= -2^-23 rounds to a negative number; uv = -inf gives +inf and
 * passes as `uv <= 1` does. The device self-test fn 14 compares both forms on special and random operands. The
 * pair test forms w for both triangles with one packed subtraction: 4.5 VALU per triangle instead of 5. */
__device__ __forceinline__ float minimum3(float a, float b, float c)
{
    return __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), c);
}
__device__ __forceinline__ bool accept_tri_w(float t, float u, float v, float w)
{
    return t > 0.0f && minimum3(u, v, w) >= 0.0f;
}

/* Integer form of the take (take_bits). The reference takes an accepted triangle iff t > 0 (:132) and t < rec.t
 * (:171). For rec.t a positive float (kInfinity at most, or an earlier accepted t > 0; never NaN), the two compares
 * are one unsigned compare of bit patterns minus one: bits(t) - 1 < bits(rec.t) - 1. Positive floats (denormals
 * included: IEEE compares them as nonzero) order like their bit patterns; t = +0 gives 0 - 1 = 0xFFFFFFFF, which is
 * never below; a negative t or -0 has the sign bit, so bits - 1 >= 0x7FFFFFFF > bits(rec.t) - 1 <= 0x7F7FFFFF;
 * a NaN t (positive 0x7F800001.. or negative) lies above every finite or infinite rec.t the same way. So the pair loop
 * carries rec.t as rb = bits(rec.t) - 1, takes with one v_add_u32 and one v_cmp_u32 per triangle instead of two float
 * compares and their mask AND, and converts back at the end of the leaf. The acceptance keeps its minimum3 >= 0 test
 * (which must pass -0 and reject NaN). Device check: selftest fn 17 compares both forms on all 2^32 t against a set of
 * rec.t values (tests/test_gpu_parity.py). Measured (round 5, 6 interleaved rounds on two boxes,
 * profiles/r05_itake_ab.log): c2 kernel 0.3635 against 0.3651 ms (-0.4 %), the reference's scene +0.3 %; the same
 * form confined to the uniform loop gained less on c2 (-0.15 %). */
__device__ __forceinline__ uint32_t take_bits(float t) { return __float_as_uint(t) - 1u; }
__device__ __forceinline__ bool accept_uvw(float u, float v, float w) { return minimum3(u, v, w) >= 0.0f; }

/* pathTracer.comp:121-133 with the two edges given: e1 = b - a, e2 = c - a (:122-123); returns t or -1 */
template <int A = kArithExact>
__device__ __forceinline__ float rayTriangleE(const Ray& r, f3 a, f3 edgeAB, f3 edgeAC)
{
    constexpr int TA = kTriA<A>;
    const f3 oa = r.origin - a;
    const f3 crossRDE2 = cross_a<TA>(r.direction, edgeAC);
    const float inv = rcp_a<TA>(dot_a<TA>(edgeAB, crossRDE2));
    const f3 crossROAE1 = cross_a<TA>(oa, edgeAB);
    const float u = dot_a<TA>(oa, crossRDE2) * inv;
    const float v = dot_a<TA>(r.direction, crossROAE1 * inv);
    const float t = dot_a<TA>(edgeAC, crossROAE1) * inv;
    return accept_tri(t, u, v, u + v) ? t : -1.0f;
}

/* Derived triangle records. For each draw command the runtime derives from the draw's index and vertex buffers,
 * triangle k = index positions 3k..3k+2, with e1 = b - a and e2 = c - a computed by the same binary32
 * subtractions as :122-123, two record arrays:
 *   single records, 48 B per triangle: (a.xyz, e1.x) (e1.yz, e2.xy) (e2.z, n.xyz), where n = normalize(cross(e1,
 *     e2)) is the geometric normal of :173 evaluated once per triangle with the same operations (it depends on
 *     the triangle only), so the hit epilogue reads it instead of re-gathering three indices and vertices;
 *   pair records, 80 B per triangle pair (2j, 2j+1): the nine components of both triangles as float2
 *     {tri 2j, tri 2j+1} + 8 B pad. One lane then tests two triangles at once with packed-FP32 instructions
 *     (v_pk_mul_f32 / v_pk_add_f32 perform two independent binary32 ops each -- exactly the reference's ops),
 *     halving the VALU issue slots of the Möller-Trumbore arithmetic; the two results are applied in
 *     reference order (2j first, then 2j+1, strict <).
 * A leaf test reads aligned 16-byte loads instead of an index fetch plus three dependent vertex gathers, and
 * the edge subtractions leave the inner loop. Pairs pay off for fat leaves (the Cornell box: ~17 triangles per
 * leaf, VALU-bound); single records for thin leaves (the atrium: ~2 triangles per leaf, fetch-latency-bound).
 * The reference's BVH keeps each leaf's index triples contiguous (PathTracingRenderer.jai:233), so a leaf's
 * records are contiguous. A leaf whose first index position is not a multiple of 3 (never produced by the
 * reference's builder) or that reaches past the draw's indexCount uses the index path.
 * The per-draw table entry (kTriTableWords x u64, word indices kTriWord*, flags kTriFlag*) and the record sizes are
 * declared once for the kernels and the runtime: frame_prep.h. */
/* table word 3, bits 32..63: vertices in the draw's vertex buffer (0xFFFFFFFF: unknown, not a context buffer) */
__device__ __forceinline__ uint32_t draw_vertex_count(const uint64_t* __restrict__ tri_records, uint32_t draw)
{
    return (uint32_t)(tri_records[kTriTableWords * draw + kTriWordFlags] >> 32);
}
typedef const WCPT_GLOBAL v4f* gtri_ptr;
struct TriE { f3 a, e1, e2; };
/* a single record's three 16-byte rows: (a.xyz, e1.x) (e1.yz, e2.xy) (e2.z, n.xyz) */
__device__ __forceinline__ TriE unpack_tri(v4f r0, v4f r1, v4f r2)
{
    TriE e;
    e.a = mk3(r0.x, r0.y, r0.z);
    e.e1 = mk3(r0.w, r1.x, r1.y);
    e.e2 = mk3(r1.z, r1.w, r2.x);
    return e;
}
__device__ __forceinline__ TriE load_tri(gtri_ptr t, uint32_t k)
{
    const gtri_ptr q = t + 3ull * k;
    return unpack_tri(q[0], q[1], q[2]);
}
constexpr uint32_t kPairRecordFloat4s = kPairRecordBytes / 16u; /* 5 */
struct TriPair { v2f ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z; };
constexpr uint32_t kNoTag = 0xFFFFFFFFu;

/* The pair record at byte offset `off` from the record base (pair j at off = kPairRecordBytes j). */
template <class P>
__device__ __forceinline__ TriPair unpack_pair(P q)
{
    const v4f r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
    TriPair p;
    p.ax = r0.xy;  p.ay = r0.zw;
    p.az = r1.xy;  p.e1x = r1.zw;
    p.e1y = r2.xy; p.e1z = r2.zw;
    p.e2x = r3.xy; p.e2y = r3.zw;
    p.e2z = r4.xy;
    return p;
}
__device__ __forceinline__ TriPair load_pair_at(const WCPT_GLOBAL char* base, uint32_t off)
{
    return unpack_pair(reinterpret_cast<gtri_ptr>(base + off));
}
/* The same record through the constant address space (4): the records are read-only for the whole launch, and a
 * wave-uniform offset then lowers to scalar loads (s_load_dwordx16 / s_load_dwordx4 through the scalar cache) whose
 * values the packed-FP32 instructions read straight from SGPRs. */
typedef const __attribute__((address_space(4))) v4f* ctri_ptr;
__device__ __forceinline__ TriPair load_pair_const(const WCPT_GLOBAL char* base, uint32_t off)
{
    return unpack_pair((ctri_ptr)(uintptr_t)(base + off));
}
__device__ __forceinline__ v2f bc2(float s) { v2f r = {s, s}; return r; }
/* rayTriangleE for the two triangles of a pair: t for triangle 2j (.x) and 2j+1 (.y), and whether each passed
 * the reference's acceptance test (t > 0, u, v, u + v in range). A triangle is taken iff it passed and t < rec.t;
 * that equals the reference's `t != -1 && t < rec.t` on its -1-for-miss result (a pass implies t > 0). */
struct PairHit { v2f t; bool hit0, hit1; };
template <int A = kArithExact>
__device__ __forceinline__ PairHit rayTrianglePair(const Ray& r, const TriPair& p)
{
    constexpr int TA = kTriA<A>;
    const v2f dx = bc2(r.direction.x), dy = bc2(r.direction.y), dz = bc2(r.direction.z);
    const v2f oax = bc2(r.origin.x) - p.ax, oay = bc2(r.origin.y) - p.ay, oaz = bc2(r.origin.z) - p.az;
    /* crossRDE2 = cross(d, e2) */
    const v2f px = msub2_a<TA>(dy, p.e2z, p.e2y, dz);
    const v2f py = msub2_a<TA>(dz, p.e2x, p.e2z, dx);
    const v2f pz = msub2_a<TA>(dx, p.e2y, p.e2x, dy);
    const v2f det = dot2_a<TA>(p.e1x, p.e1y, p.e1z, px, py, pz);
    /* crossROAE1 = cross(oa, e1) */
    const v2f qx = msub2_a<TA>(oay, p.e1z, p.e1y, oaz);
    const v2f qy = msub2_a<TA>(oaz, p.e1x, p.e1z, oax);
    const v2f qz = msub2_a<TA>(oax, p.e1y, p.e1x, oay);
    const v2f un = dot2_a<TA>(oax, oay, oaz, px, py, pz);          /* dot(oa, crossRDE2) */
    const v2f tn = dot2_a<TA>(p.e2x, p.e2y, p.e2z, qx, qy, qz);    /* dot(edgeAC, crossROAE1) */
    /* computed before the reciprocal: its fallback branch would otherwise split the block, and these independent
     * products would be sunk past it instead of filling the det -> rcp -> Newton chain's dependency stalls */
    asm volatile("" ::"v"(qx), "v"(qy), "v"(qz), "v"(un), "v"(tn));
    const v2f inv = rcp2_a<TA>(det);
    const v2f u = un * inv;
    const v2f v = dot2_a<TA>(dx, dy, dz, qx * inv, qy * inv, qz * inv);
    const v2f t = tn * inv;
    const v2f uv = u + v;
    PairHit h;
    h.t = t;
    /* t > 0 is part of the take's integer compare (take_bits) */
    const v2f w = bc2(1.0f) - uv;
    h.hit0 = accept_uvw(u.x, v.x, w.x);
    h.hit1 = accept_uvw(u.y, v.y, w.y);
    return h;
}
/* Primary-ray pair records. Every primary ray of a frame starts at the camera (pathTracer.comp:299-302, SceneData
 * position), so the terms of rayTrianglePair that depend only on the origin and the triangle -- oa = o - a, q =
 * cross(oa, e1) and the t numerator dot(e2, q) (:124-125, :127, :130) -- are the same for every primary ray. The
 * runtime derives them once per camera position (build_primary_pairs, the same binary32 operations in the same
 * order, so the values are bit-identical) and the first segment of each sample tests its leaves from these records:
 * 51 instead of 68 VALU per pair. 112 B per pair: (e1x, e1y) (e1z, e2x) (e2y, e2z) (oax, oay) (oaz, qx) (qy, qz)
 * (tq, pad), each a float2 {triangle 2j, 2j+1}. */
constexpr uint32_t kPrimPairFloat4s = kPrimPairRecordBytes / 16u; /* 7 */
struct TriPairP { v2f e1x, e1y, e1z, e2x, e2y, e2z, oax, oay, oaz, qx, qy, qz, tq; };
template <class P>
__device__ __forceinline__ TriPairP unpack_pairP(P q)
{
    const v4f r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4], r5 = q[5], r6 = q[6];
    TriPairP p;
    p.e1x = r0.xy; p.e1y = r0.zw;
    p.e1z = r1.xy; p.e2x = r1.zw;
    p.e2y = r2.xy; p.e2z = r2.zw;
    p.oax = r3.xy; p.oay = r3.zw;
    p.oaz = r4.xy; p.qx = r4.zw;
    p.qy = r5.xy;  p.qz = r5.zw;
    p.tq = r6.xy;
    return p;
}
__device__ __forceinline__ TriPairP load_pairP_at(const WCPT_GLOBAL char* base, uint32_t off)
{
    return unpack_pairP(reinterpret_cast<gtri_ptr>(base + off));
}
__device__ __forceinline__ TriPairP load_pairP_const(const WCPT_GLOBAL char* base, uint32_t off)
{
    return unpack_pairP((ctri_ptr)(uintptr_t)(base + off));
}
/* Exact sign pre-reject of a primary pair (execute fewer triangle tests).
 * The reference's t is RN(tn * RN(1 / det)) (:126, :130), and a take needs t > 0 (:132). The primary records hold tn
 * itself (tq, bit-identical to the test's), and det is the test's first result, so before the rest of the test: when
 * the sign bits of tq and det differ, t is negative, -0 (an underflow) or NaN (a NaN operand) -- never > 0 -- and when
 * det is +-0 or tq is +-0 with different signs the same holds (t = -inf, -0 or NaN). Such a triangle cannot be taken,
 * whatever rec.t is. A wave whose every lane has both triangles of a pair in that case skips the pair's remaining
 * operations (reciprocal, u, v, t, acceptance: 39 of its 53 VALU); a lane that may take either runs the whole test,
 * so every result is the reference's. On primary rays (all from the camera, directions within one 8x8 tile) the sign
 * of det -- which side of the triangle's plane the ray heads to -- is nearly uniform across a wave: on Cornell ~21 %
 * of the primary pair steps are skippable by the whole wave (tools/prereject_sim.py; under 3 % on bounce rays, whose
 * directions are random per lane, where the test therefore is not made).
 * The argument needs only sign(rcp(det)) = sign(det) and rcp(+-0) = +-inf. Both hold for the bare v_rcp_f32 of the fast
 * arithmetic mode as for the corrected reciprocal (the instruction keeps the operand's sign, and a denormal det it may
 * flush is a zero of the same sign), so the fast kernels skip the same way: there t = RN(tq * rcp(det)). */
template <int A = kArithExact>
__device__ __forceinline__ v2f pairP_det(const Ray& r, const TriPairP& p, v2f& px, v2f& py, v2f& pz)
{
    constexpr int TA = kTriA<A>;
    const v2f dx = bc2(r.direction.x), dy = bc2(r.direction.y), dz = bc2(r.direction.z);
    px = msub2_a<TA>(dy, p.e2z, p.e2y, dz);
    py = msub2_a<TA>(dz, p.e2x, p.e2z, dx);
    pz = msub2_a<TA>(dx, p.e2y, p.e2x, dy);
    return dot2_a<TA>(p.e1x, p.e1y, p.e1z, px, py, pz);
}
/* the rest of the test after det; t > 0 is part of the take's integer compare (take_bits) */
template <int A = kArithExact>
__device__ __forceinline__ PairHit pairP_finish(const Ray& r, const TriPairP& p, v2f px, v2f py, v2f pz, v2f det)
{
    constexpr int TA = kTriA<A>;
    const v2f dx = bc2(r.direction.x), dy = bc2(r.direction.y), dz = bc2(r.direction.z);
    const v2f inv = rcp2_a<TA>(det);
    const v2f u = dot2_a<TA>(p.oax, p.oay, p.oaz, px, py, pz) * inv;
    const v2f v = dot2_a<TA>(dx, dy, dz, p.qx * inv, p.qy * inv, p.qz * inv);
    const v2f t = p.tq * inv;
    const v2f uv = u + v;
    PairHit h;
    h.t = t;
    const v2f w = bc2(1.0f) - uv;
    h.hit0 = accept_uvw(u.x, v.x, w.x);
    h.hit1 = accept_uvw(u.y, v.y, w.y);
    return h;
}
/* rayTrianglePair with the origin terms taken from the record: the remaining operations are rayTrianglePair's, in the
 * two steps below (the uniform leaf loop tests the determinants' signs between them) */
template <int A = kArithExact>
__device__ __forceinline__ PairHit rayTrianglePairP(const Ray& r, const TriPairP& p)
{
    v2f px, py, pz;
    const v2f det = pairP_det<A>(r, p, px, py, pz);
    return pairP_finish<A>(r, p, px, py, pz, det);
}
/* whether a lane may take either triangle of the pair: the sign bits of tq and det agree for at least one of them */
__device__ __forceinline__ bool pairP_may_take(const TriPairP& p, v2f det)
{
    return (int32_t)(__float_as_uint(det.x) ^ __float_as_uint(p.tq.x)) >= 0 ||
           (int32_t)(__float_as_uint(det.y) ^ __float_as_uint(p.tq.y)) >= 0;
}

/* The origin terms of one triangle (half h of pair record q) for origin o: build_primary_pairs */
__device__ __forceinline__ void primary_terms(float ox, float oy, float oz, float ax, float ay, float az, float e1x,
                                              float e1y, float e1z, float e2x, float e2y, float e2z, float out[7])
{
    const float oax = ox - ax, oay = oy - ay, oaz = oz - az;
    const float qx = oay * e1z - e1y * oaz;
    const float qy = oaz * e1x - e1z * oax;
    const float qz = oax * e1y - e1x * oay;
    out[0] = oax; out[1] = oay; out[2] = oaz;
    out[3] = qx;  out[4] = qy;  out[5] = qz;
    out[6] = (e2x * qx + e2y * qy) + e2z * qz;
}

/* Vertex i of a draw whose vertex buffer holds nvert vertices (table word 3, high half; 0xFFFFFFFF when the buffer
 * is not a context buffer): a vertex index past the buffer reads NaN instead of memory past it, so that triangle is
 * never accepted (every comparison with NaN fails) -- the same rule the derived records follow (tri_fields). */
__device__ __forceinline__ f3 ld_vertex(gf32_ptr vtx, uint32_t i, uint32_t nvert)
{
    if (__builtin_expect(i < nvert, 1)) return ld3(vtx + 3ull * i);
    const float qnan = __uint_as_float(0x7fc00000u);
    return mk3(qnan, qnan, qnan);
}
__device__ __forceinline__ TriE tri_from_indices(gu32_ptr idx, gf32_ptr vtx, uint32_t first, uint32_t nvert)
{
    const f3 a = ld_vertex(vtx, idx[first + 0], nvert);
    const f3 b = ld_vertex(vtx, idx[first + 1], nvert);
    const f3 c = ld_vertex(vtx, idx[first + 2], nvert);
    TriE e;
    e.a = a;
    e.e1 = b - a;
    e.e2 = c - a;
    return e;
}
/* Leaf cursor into the records: triangle index of the leaf's first triangle, or kNoRecord for a leaf that does not
 * start on a triangle boundary or is not fully covered by the draw's `ntri` records. The per-draw table entry
 * is {record address, ntri} (2 x u64). */
constexpr uint32_t kNoRecord = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t leaf_record(uint32_t first, uint32_t count, uint32_t ntri)
{
    const uint32_t k = first / 3u;
    return (k * 3u == first && (uint64_t)k + (count + 2u) / 3u <= ntri) ? k : kNoRecord;
}
/* v_mul_u32_u24 (full rate). __umul24 is not enough here: only the low 24 bits of its product are used, so the
 * optimizer drops its 24-bit operand masks and the backend then emits the quarter-rate v_mul_lo_u32 (seen in the ISA
 * of both kernels). */
__device__ __forceinline__ uint32_t mul_u32_u24(uint32_t a, uint32_t b_uniform)
{
    uint32_t r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "s"(b_uniform), "v"(a));
    return r;
}
/* The single record of the triangle at index position `pos` (the reference reads indices pos..pos+2, :174-176) as a
 * byte offset, for kTriFlagIndex24 draws: record k = pos / 3 was derived from exactly those indices when pos is a
 * multiple of 3 and k < ntri (pos < lim3 = 3 * ntri); else kNoRecord (the index path). Per triangle, so a leaf's
 * cursor needs no record offset of its own. 48 B per triangle = 16 B per index position, so the record is at 16 * pos,
 * and no division: for pos < 2^24, pos % 3 == 0 exactly when (pos * 0xAAAAAB) mod 2^24 <= 0x555555 (0xAAAAAB is the
 * inverse of 3 mod 2^24; checked for every pos < 2^24), one full-rate v_mul_u32_u24 instead of leaf_record's
 * quarter-rate v_mul_hi_u32 pair. lim3 < 2^24 for these draws, so an accepted pos is < 2^24 and the test is exact. */
__device__ __forceinline__ uint32_t tri_record_off24(uint32_t pos, uint32_t lim3)
{
    const bool aligned = (mul_u32_u24(pos, 0xAAAAABu) & 0xFFFFFFu) <= 0x555555u;
    return (aligned && pos < lim3) ? pos * 16u : kNoRecord;
}
/* leaf_record as a byte offset for any draw (records beyond 4 GiB take the index path) */
__device__ __forceinline__ uint32_t leaf_record_off(uint32_t first, uint32_t count, uint32_t ntri)
{
    const uint32_t k = leaf_record(first, count, ntri);
    return (k != kNoRecord && k < (1u << 26)) ? k * 48u : kNoRecord;
}
/* Single records through a buffer resource of ntri records (48 B each; ntri < 2^24 / 3 for the draws that use it):
 * an offset past the records reads zeros (hardware range check), i.e. a = e1 = e2 = 0, whose det is 0 and whose test
 * never accepts (0 * inf = NaN fails every comparison) */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tri_rsrc(gtri_ptr t, uint32_t ntri)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)t, (short)0, (int)(ntri * 48u), kBufferDword3);
}
__device__ __forceinline__ TriE load_tri_rsrc(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    const v4f r0 = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    const v4f r1 = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, off + 16, 0, 0));
    const v4f r2 = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, off + 32, 0, 0));
    return unpack_tri(r0, r1, r2);
}
__device__ __forceinline__ TriE load_tri_at(gtri_ptr t, uint32_t off)
{
    const gtri_ptr q = reinterpret_cast<gtri_ptr>(reinterpret_cast<const WCPT_GLOBAL char*>(t) + off);
    return unpack_tri(q[0], q[1], q[2]);
}

} // namespace wcpt::dev

#endif /* WCPT_PT_GEOMETRY_H */
