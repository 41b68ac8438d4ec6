/* primary_hit.h -- what one record of the primary-hit buffer (wcpt_trace_primary, wcpt_pick; include/wcpt.h
 * wcpt_primary_hit) holds, stated once: the words, their packing, the miss values and where a pixel's record lies. Plain
 * C++, no HIP: the kernel (pt_primary.hip), the runtime (wcpt_render.hip) and tests/primary_hit_shim.cpp (g++) share it.
 *
 * A record is what Intersect (pathTracer.comp:135-211) leaves for a pixel's primary ray, with the identity of the primitive
 * that won. Twelve 32-bit words, three 16-byte rows:
 *
 *   0-2   direction.xyz  the primary ray's direction (primary_direction)
 *   3     t              the hit distance; kInfinity (kPrimHitMissT) on a miss
 *   4-6   normal.xyz     as resolve_hit returns it (flipped towards the ray); zeros on a miss
 *   7     kind           kPrimHitMiss / Sphere / Triangle in bits 0-1, kPrimHitFrontBit = resolve_hit's `front`
 *   8     material       the sphere's material; 0 for a triangle (:175) and for a miss
 *   9     index          sphere index, or the triangle's number in its draw's index buffer (index position / 3); 0 on a miss
 *   10    draw           draw command of a triangle hit; 0 otherwise
 *   11    0
 *
 * No value is narrowed: every float word is the value's own bits (-0.0 and NaN payloads included). p is not stored: it is
 * origin + t * direction on these bits.
 *
 * Layout: row-major over the window the pass covers -- the context's rows back to back for wcpt_trace_primary, one pixel
 * for wcpt_pick: record (ly, x) of a window `width` pixels wide lies at primary_hit_offset(ly, x, width). Which frame row
 * local row ly is, the frame's row map says (row_map.h). */
#ifndef WCPT_PRIMARY_HIT_H
#define WCPT_PRIMARY_HIT_H

#include <stdint.h>

#ifdef __HIPCC__
#define WCPT_PRIM_HIT_HD __host__ __device__
#else
#define WCPT_PRIM_HIT_HD
#endif

namespace wcpt {

constexpr uint32_t kPrimHitWords = 12;                  /* 32-bit words per pixel */
constexpr uint32_t kPrimHitBytes = kPrimHitWords * 4u;  /* 48 B per pixel: sizeof(wcpt_primary_hit) */
constexpr uint32_t kPrimHitMiss = 0u, kPrimHitSphere = 1u, kPrimHitTriangle = 2u; /* WCPT_HIT_* */
constexpr uint32_t kPrimHitKindMask = 3u;
constexpr uint32_t kPrimHitFrontBit = 0x80000000u;
constexpr uint32_t kPrimHitMissT = 0x7F7FFFFFu;         /* kInfinity (pt_math.h): the largest finite binary32 */
/* the primitive as the traversal names it (pt_geometry.h kNoPrim, kSpherePrim): none, kPrimHitSpherePrim | sphere index,
 * or the index position of a triangle's first index */
constexpr uint32_t kPrimHitNoPrim = 0xFFFFFFFFu, kPrimHitSpherePrim = 0x80000000u;

/* A record, every float as its bits. */
struct PrimaryHit {
    uint32_t dir[3];
    uint32_t t;
    uint32_t normal[3];
    uint32_t kind;     /* kPrimHitMiss / Sphere / Triangle */
    bool front;
    uint32_t material, index, draw;
};

/* byte offset of record (ly, x) in a window of `width` pixels per row */
WCPT_PRIM_HIT_HD inline uint64_t primary_hit_offset(uint64_t ly, uint64_t x, uint64_t width)
{
    return (ly * width + x) * kPrimHitBytes;
}
/* the bytes a window of width x rows pixels takes */
WCPT_PRIM_HIT_HD inline uint64_t primary_hit_bytes(uint64_t width, uint64_t rows) { return primary_hit_offset(rows, 0, width); }

/* The record of the traversal's winner `prim` of draw `draw` (pt_traversal.h closest_hit) with resolve_hit's t, normal,
 * front and material for it. A miss gets the miss values whatever the other arguments hold. */
WCPT_PRIM_HIT_HD inline PrimaryHit primary_hit_of(const uint32_t dir[3], uint32_t t, const uint32_t normal[3], bool front,
                                                  uint32_t material, uint32_t prim, uint32_t draw)
{
    PrimaryHit r;
    r.dir[0] = dir[0];
    r.dir[1] = dir[1];
    r.dir[2] = dir[2];
    if (prim == kPrimHitNoPrim) {
        r.t = kPrimHitMissT;
        r.normal[0] = r.normal[1] = r.normal[2] = 0u;
        r.kind = kPrimHitMiss;
        r.front = false;
        r.material = r.index = r.draw = 0u;
        return r;
    }
    const bool sphere = (prim & kPrimHitSpherePrim) != 0u;
    r.t = t;
    r.normal[0] = normal[0];
    r.normal[1] = normal[1];
    r.normal[2] = normal[2];
    r.kind = sphere ? kPrimHitSphere : kPrimHitTriangle;
    r.front = front;
    r.material = sphere ? material : 0u;
    r.index = sphere ? (prim & ~kPrimHitSpherePrim) : prim / 3u;
    r.draw = sphere ? 0u : draw;
    return r;
}

WCPT_PRIM_HIT_HD inline void primary_hit_pack(const PrimaryHit& r, uint32_t w[kPrimHitWords])
{
    w[0] = r.dir[0];
    w[1] = r.dir[1];
    w[2] = r.dir[2];
    w[3] = r.t;
    w[4] = r.normal[0];
    w[5] = r.normal[1];
    w[6] = r.normal[2];
    w[7] = (r.kind & kPrimHitKindMask) | (r.front ? kPrimHitFrontBit : 0u);
    w[8] = r.material;
    w[9] = r.index;
    w[10] = r.draw;
    w[11] = 0u;
}

WCPT_PRIM_HIT_HD inline PrimaryHit primary_hit_unpack(const uint32_t w[kPrimHitWords])
{
    PrimaryHit r;
    r.dir[0] = w[0];
    r.dir[1] = w[1];
    r.dir[2] = w[2];
    r.t = w[3];
    r.normal[0] = w[4];
    r.normal[1] = w[5];
    r.normal[2] = w[6];
    r.kind = w[7] & kPrimHitKindMask;
    r.front = (w[7] & kPrimHitFrontBit) != 0u;
    r.material = w[8];
    r.index = w[9];
    r.draw = w[10];
    return r;
}

} // namespace wcpt

#endif
