/* pt_mk_tiny.h -- the launches of pt_mk_tiny.hip, for pt_kernels.hip launch_megakernel: the walk-only head and tail that
 * a tiny tree's split render takes in the places of the general ones (mk_tiny_rule.h mk_tiny_kernels). */
#ifndef WCPT_PT_MK_TINY_H
#define WCPT_PT_MK_TINY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace wcpt {

/* The head's tiles, as launch_mega passes them to pt_megakernel: the grid, tile_of_block's arguments, where the tiles'
 * times are recorded (or null) and the primary cache (null with the cache off). */
struct TinyHeadLaunch {
    uint32_t grid, tilesX, tiles, scatter;
    const uint32_t* order;
    uint32_t* cost;
    uint32_t* prim_cache;
};
/* pt_tiny_head<pcmode> (kPrimaryCacheNone / Write / Read) on `stream`; any other pcmode is an error */
hipError_t launch_tiny_head(const LaunchArgs& a, int pcmode, const TinyHeadLaunch& h, const dev::SplitQueue& q,
                            hipStream_t stream);
/* pt_tiny_tail behind it: one wave per 64 entries of the queue's capacity */
hipError_t launch_tiny_tail(const LaunchArgs& a, const dev::SplitQueue& q, hipStream_t stream);

} // namespace wcpt

#endif
