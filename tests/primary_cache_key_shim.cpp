// Test shim (CPU): exposes the primary cache's key and rule (wc-path-tracer_amd/csrc/primary_cache_key.h, what
// launch_megakernel applies) to tests/test_primary_cache_key.py over ctypes. Built by the test with g++; no HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/primary_cache_key.h"

// geom: {W, H, y0, rows, row_shift, row_gap, spheres, draws, tri_records, pair_records, generation}
static wcpt::PrimaryCacheKey key_of(const wcpt_scene_data* sd, const uint64_t* g)
{
    return wcpt::primary_cache_key(*sd, (uint32_t)g[0], (uint32_t)g[1], (uint32_t)g[2], (uint32_t)g[3], (uint32_t)g[4],
                                   (uint32_t)g[5], g[6], g[7], g[8], g[9] != 0, g[10]);
}

extern "C" int pck_equal(const wcpt_scene_data* sd_a, const uint64_t* geom_a, const wcpt_scene_data* sd_b,
                         const uint64_t* geom_b)
{
    return wcpt::primary_cache_key_equal(key_of(sd_a, geom_a), key_of(sd_b, geom_b)) ? 1 : 0;
}

// The mode of a render of (sd, geom) on a context whose stored key is that of (stored_sd, stored_geom).
extern "C" int pck_decide(int enabled, int stored_valid, const wcpt_scene_data* stored_sd, const uint64_t* stored_geom,
                          const wcpt_scene_data* sd, const uint64_t* geom)
{
    return (int)wcpt::primary_cache_decide(enabled != 0, sd->renderedFramesCount, stored_valid != 0,
                                           key_of(stored_sd, stored_geom), key_of(sd, geom));
}

extern "C" int pck_scene_data_bytes(void) { return (int)sizeof(wcpt_scene_data); }
