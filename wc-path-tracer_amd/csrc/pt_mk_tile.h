/* pt_mk_tile.h -- what every megakernel translation unit shares of a launch's frame side: the pixel tile of a wave, the
 * tile a block renders (tile_of_block) and the end of a pixel (accumulate_store). Included by pt_kernels.hip (the general
 * kernels) and pt_mk_tiny.hip (the walk-only kernels of tiny-tree renders). */
#ifndef WCPT_PT_MK_TILE_H
#define WCPT_PT_MK_TILE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_device.h"

namespace wcpt {
namespace dev {

/* Pixel tile of one wave64: kTileW x kTileH. Measured on c2: 8x8 and 4x16 equal, 16x4 +3%, 32x2 +4%. */
#ifndef WCPT_TILE_W
#define WCPT_TILE_W 8
#endif
constexpr uint32_t kTileW = WCPT_TILE_W, kTileH = 64u / WCPT_TILE_W;

/* Pixel tile -> block mapping. Blocks are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md,
 * "Workgroup dispatch"); remapping the linear block id so that each XCD walks a contiguous band of tiles
 * keeps neighbouring (coherent) tiles on one XCD's L2. Speed only; any placement is correct. */
__device__ __forceinline__ void tile_of_block(uint32_t tilesX, uint32_t tilesTotal, uint32_t scatter,
                                              const uint32_t* __restrict__ order, uint32_t& tx, uint32_t& ty)
{
    const uint32_t b = blockIdx.x;
    uint32_t t = b;
    if (order != nullptr) {
        t = order[b]; /* cost-ordered: a permutation of [0, tilesTotal), longest tile first */
    } else if (scatter & 1u) {
        t = (uint32_t)(((uint64_t)b * scatter) % tilesTotal);   /* odd: scattered, multiplier `scatter` */
    } else if ((tilesTotal & 7u) == 0u) {
        /* blocks go to the XCDs round-robin (block b -> XCD b mod 8): XCD x walks the x-th eighth of a tile list */
        t = (b & 7u) * (tilesTotal >> 3) + (b >> 3);
        if (scatter != 0u) {
            /* even scatter = 2h: striped list. Stripes of h tile rows, listed by (stripe mod 8, stripe / 8), each in
             * raster order, so XCD x walks (about) the stripes s = x mod 8: neighbouring tiles stay together on an
             * XCD, and every XCD sees every part of the frame (one contiguous band per XCD can leave a few XCDs with
             * the heavy regions of the image) */
            const uint32_t h = scatter >> 1;
            const uint32_t tilesY = tilesTotal / tilesX;
            const uint32_t full = tilesY / (8u * h), rem = tilesY % (8u * h);
            for (uint32_t j = 0; j < 8u; j++) {
                const uint32_t part = rem > j * h ? min(rem - j * h, h) : 0u;
                const uint32_t seg = (full * h + part) * tilesX;   /* tiles of the rows in stripes s = j mod 8 */
                if (t < seg) {
                    const uint32_t lr = t / tilesX;
                    t = (((lr / h) * 8u + j) * h + lr % h) * tilesX + t % tilesX;
                    break;
                }
                t -= seg;
            }
        }
    }
    tx = t % tilesX;
    ty = t / tilesX;
}

/* The end of a pixel (pathTracer.comp:312-323): the mean of the samples' radiance `result`, accumulated into the
 * image's value `old` (read early by the caller) and stored. Shared by the whole kernel, the heads and the tails. */
__device__ __forceinline__ void accumulate_store(const wcpt_scene_data& sd, float4* __restrict__ image,
                                                 float* __restrict__ wire, uint32_t wire_ch, const RowMap& wm, uint32_t W,
                                                 uint32_t lx, uint32_t ly, float4 old, f3 result)
{
    result = result / (float)sd.samples; /* :312 */
    f3 acc;
    if (sd.renderedFramesCount == 0) { /* :318 — the loaded value would be discarded */
        acc = result;
    } else {
        const float4 o = old;                                             /* :314 */
        const float weight = 1.0f / (float)(sd.renderedFramesCount + 1u); /* :316 */
        const float iw = 1.0f - weight;
        acc = mk3(o.x * iw + result.x * weight, o.y * iw + result.y * weight, o.z * iw + result.z * weight);
    }
    store_pixel(image, wire, wire_ch, wm, W, lx, ly, acc); /* :323 */
}

} // namespace dev
} // namespace wcpt

#endif /* WCPT_PT_MK_TILE_H */
