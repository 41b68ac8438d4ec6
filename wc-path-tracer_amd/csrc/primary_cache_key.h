/* primary_cache_key.h — when the megakernel's primary cache (WCPT_OPTION_PRIMARY_CACHE) is valid. Host only, no HIP:
 * tests/primary_cache_key_shim.cpp compiles it with g++.
 *
 * A cache entry is a pixel's resolved primary segment (primary_record.h: the primary ray's direction and resolve_hit's
 * result for it -- distance, facing, normal, material index). It is a function of the primary ray (the pixel, W, H,
 * inverseProjection, inverseView, position: pt_device.h primary_direction, no random number), of the geometry the
 * ray meets (spheres, draw commands and what they point at; a sphere's material index comes from the sphere buffer) and
 * of the arithmetic mode, which bumps the generation. A material's contents are not in it: they are read every frame.
 * The key holds all of it that the runtime can see: the
 * camera's bytes, the two counts, the frame and the context's rows of it (they decide which pixel a record index is),
 * the addresses the kernel reads the geometry through, the leaf-record choice, and the context's generation counter,
 * which every buffer alloc / upload / free and every option change bumps. maxBounceCount, samples, the materials and
 * renderedFramesCount are not in it: the entry does not depend on them. (renderedFramesCount == 0 drops the cache
 * whatever the key says: primary_cache_decide.) */
#ifndef WCPT_PRIMARY_CACHE_KEY_H
#define WCPT_PRIMARY_CACHE_KEY_H

#include <stdint.h>
#include <string.h>

#include "../../include/wcpt.h"

namespace wcpt {

struct PrimaryCacheKey {
    uint32_t inverseProjection[16]; /* bit patterns: -0.0 and NaN payloads count as changes */
    uint32_t inverseView[16];
    uint32_t position[3];
    uint32_t sphereCount, drawCommandCount;
    uint32_t W, H, y0, rows, row_shift, row_gap;
    uint64_t spheres, draws, tri_records; /* device addresses: sphere buffer, draw commands, record table */
    uint32_t pair_records;                /* leaf tests on pair records (1) or singles (0) */
    uint64_t generation;
};

inline PrimaryCacheKey primary_cache_key(const wcpt_scene_data& sd, uint32_t W, uint32_t H, uint32_t y0, uint32_t rows,
                                         uint32_t row_shift, uint32_t row_gap, uint64_t spheres, uint64_t draws,
                                         uint64_t tri_records, bool pair_records, uint64_t generation)
{
    PrimaryCacheKey k;
    memcpy(k.inverseProjection, sd.inverseProjection, sizeof(k.inverseProjection));
    memcpy(k.inverseView, sd.inverseView, sizeof(k.inverseView));
    memcpy(k.position, sd.position, sizeof(k.position));
    k.sphereCount = sd.sphereCount;
    k.drawCommandCount = sd.drawCommandCount;
    k.W = W;
    k.H = H;
    k.y0 = y0;
    k.rows = rows;
    k.row_shift = row_shift;
    k.row_gap = row_gap;
    k.spheres = spheres;
    k.draws = draws;
    k.tri_records = tri_records;
    k.pair_records = pair_records ? 1u : 0u;
    k.generation = generation;
    return k;
}

inline bool primary_cache_key_equal(const PrimaryCacheKey& a, const PrimaryCacheKey& b)
{
    return memcmp(a.inverseProjection, b.inverseProjection, sizeof(a.inverseProjection)) == 0 &&
           memcmp(a.inverseView, b.inverseView, sizeof(a.inverseView)) == 0 &&
           memcmp(a.position, b.position, sizeof(a.position)) == 0 && a.sphereCount == b.sphereCount &&
           a.drawCommandCount == b.drawCommandCount && a.W == b.W && a.H == b.H && a.y0 == b.y0 && a.rows == b.rows &&
           a.row_shift == b.row_shift && a.row_gap == b.row_gap && a.spheres == b.spheres && a.draws == b.draws &&
           a.tri_records == b.tri_records && a.pair_records == b.pair_records && a.generation == b.generation;
}

/* What one megakernel render does with the cache: nothing, trace and store the records, or read them. */
enum PrimaryCacheMode : int { kPrimaryCacheNone = 0, kPrimaryCacheWrite = 1, kPrimaryCacheRead = 2 };

/* The rule. enabled: the option is on (with the triangle cache) and this is a render, not a counting run. Frame 0
 * (renderedFramesCount == 0: accumulation restarts, which is also what an application does after it rewrote a buffer
 * behind the runtime) drops the cache and renders plainly, so a camera that moves every frame pays nothing; a later
 * frame reads when the stored key matches, and otherwise writes (the caller then stores `key`). */
inline PrimaryCacheMode primary_cache_decide(bool enabled, uint32_t renderedFramesCount, bool stored_valid,
                                             const PrimaryCacheKey& stored, const PrimaryCacheKey& key)
{
    if (!enabled || renderedFramesCount == 0u) return kPrimaryCacheNone;
    return stored_valid && primary_cache_key_equal(stored, key) ? kPrimaryCacheRead : kPrimaryCacheWrite;
}

} // namespace wcpt

#endif
