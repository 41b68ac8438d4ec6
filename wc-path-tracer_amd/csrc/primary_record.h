/* primary_record.h -- what one entry of the megakernel's primary cache (WCPT_OPTION_PRIMARY_CACHE) holds, stated once:
 * the words, their packing and where a pixel's entry lies. Plain C++, no HIP: the kernels (pt_path.h, pt_kernels.hip),
 * the runtime's allocation (pt_kernels.hip launch_megakernel) and tests/primary_record_shim.cpp (g++) share it.
 *
 * An entry is the resolved primary segment of a pixel: the primary ray's direction and what resolve_hit returned for it.
 * All of it depends only on what primary_cache_key.h's key covers (the pixel, the camera, the geometry, the arithmetic
 * mode through the generation); nothing of a material's contents or of the RNG is in it. Eight 32-bit words:
 *
 *   0-2  dir.xyz     the primary ray's direction (primary_direction)
 *   3    t | front   the hit distance's bits with `front` in the sign bit: every accepted t is > 0, so the bit is free.
 *                    A miss is kInfinity (no accepted t is infinite -- a hit needs t < kInfinity), so `hit` needs no bit
 *   4-6  normal.xyz  as resolve_hit returns it (already flipped towards the ray); a miss stores resolve_hit's zeros
 *   7    material    the full 32-bit index
 *
 * No value is narrowed: every float word is the value's own bits (-0.0 and NaN payloads included). h.p is not stored: the
 * reader evaluates the same axpy(origin, direction, t) on the same bits. The entry is resolved, so it needs no draw
 * index: one- and multi-draw renders share the format.
 *
 * Layout: tile-major, entry index (ty * tilesX + tx) * 64 + lane, each entry two 16-byte halves side by side: a wave
 * reads or writes one contiguous 2 KiB run with two 16-byte accesses per lane. */
#ifndef WCPT_PRIMARY_RECORD_H
#define WCPT_PRIMARY_RECORD_H

#include <stdint.h>

#ifdef __HIPCC__
#define WCPT_PRIM_REC_HD __host__ __device__
#else
#define WCPT_PRIM_REC_HD
#endif

namespace wcpt {

constexpr uint32_t kPrimRecWords = 8;                       /* 32-bit words per pixel */
constexpr uint32_t kPrimRecBytes = kPrimRecWords * 4u;      /* 32 B per pixel */
constexpr uint32_t kPrimRecTileWords = 64u * kPrimRecWords; /* one wave's 8x8 tile: 2 KiB */
constexpr uint32_t kPrimRecMissBits = 0x7F7FFFFFu;          /* kInfinity (pt_math.h): the largest finite binary32 */
constexpr uint32_t kPrimRecFrontBit = 0x80000000u;

/* The resolved primary segment, every float as its bits. */
struct PrimaryRecord {
    uint32_t dir[3];
    uint32_t normal[3];
    uint32_t t;        /* > 0; kPrimRecMissBits on a miss */
    uint32_t material;
    bool hit, front;
};

/* the cache's size for a render of `tiles` 8x8 tiles (partial tiles hold whole entries) */
WCPT_PRIM_REC_HD inline uint64_t primary_record_bytes(uint64_t tiles) { return tiles * 64ull * kPrimRecBytes; }
/* word offset of lane `lane`'s entry in a cache whose tile `tile` = ty * tilesX + tx */
WCPT_PRIM_REC_HD inline uint64_t primary_record_word(uint64_t tile, uint32_t lane)
{
    return tile * kPrimRecTileWords + (uint64_t)(lane & 63u) * kPrimRecWords;
}

/* `hit` is not packed: it is t != kInfinity, which every hit satisfies and every miss (t = kInfinity) does not. */
WCPT_PRIM_REC_HD inline void primary_record_pack(const PrimaryRecord& r, uint32_t w[kPrimRecWords])
{
    w[0] = r.dir[0];
    w[1] = r.dir[1];
    w[2] = r.dir[2];
    w[3] = r.t | (r.front ? kPrimRecFrontBit : 0u);
    w[4] = r.normal[0];
    w[5] = r.normal[1];
    w[6] = r.normal[2];
    w[7] = r.material;
}

WCPT_PRIM_REC_HD inline PrimaryRecord primary_record_unpack(const uint32_t w[kPrimRecWords])
{
    PrimaryRecord r;
    r.dir[0] = w[0];
    r.dir[1] = w[1];
    r.dir[2] = w[2];
    r.t = w[3] & ~kPrimRecFrontBit;
    r.front = (w[3] & kPrimRecFrontBit) != 0u;
    r.hit = r.t != kPrimRecMissBits;
    r.normal[0] = w[4];
    r.normal[1] = w[5];
    r.normal[2] = w[6];
    r.material = w[7];
    return r;
}

} // namespace wcpt

#endif
