/*
 * pt_mk_tiny.hip -- the walk-only megakernels for gfx950: the head and the tail of a split render whose one draw has a
 * tiny tree (mk_tiny_rule.h: a root leaf, or a root over two leaves -- a box, a panel, the Cornell room).
 *
 * A translation unit of its own, so that nothing of the traversal loop is compiled beside the walk (pt_tiny.h): these
 * kernels hold no LDS stack, no spill stack, no mode loop, no draw loop, no PeelCache and no overflow flag -- a walk
 * cannot overflow -- and the general kernels of pt_kernels.hip hold nothing of the walk. launch_megakernel takes this
 * pair in the places of the general head and tail exactly where mk_tiny_kernels (mk_tiny_rule.h) says so: a render, the
 * draw's tiny-tree flag, a split, pair records, one draw command, exact arithmetic. Everything else of a head and a
 * tail is here as it is there: the tile mapping with its cost-ordered and piped lists and the tile times, the split
 * queue and its counters, the primary cache's write and read, the primary pair records with their sign pre-reject, the
 * row maps, the gather payload and accumulate_store -- through the same device functions, so the same bits.
 *
 * Four kernels: pt_tiny_head<PC> for PC none / write / read, and pt_tiny_tail. One sample, as every split render.
 */
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_mk_tile.h"
#include "pt_mk_tiny.h"
#include "pt_tiny.h"

namespace wcpt {
namespace dev {

/* Occupancy floors (__launch_bounds__'s minimum waves per SIMD), chosen by measurement (profiles/tiny_regs_ab.log sections
 * 3 and 4; the earlier sweep is profiles/tiny_kernels_ab.log section 3). With the accumulation read behind the trace (below)
 * the compiler's own allocation is 79-83 VGPRs for the heads and 73 for the tail. A floor of 7 on all four -- 72 VGPRs; 32-48
 * bytes of scratch in the heads, none in the tail, which pays its one register with SGPRs spilled to VGPR lanes -- measured c2
 * 0.2335 ms against 0.2363 at the earlier floor of 6 with the early read. The floors only pay together: heads 7 with the tail
 * at 6 measured 0.2381, heads 6 with the tail at 7 0.2389, 6 / 6 0.2359, heads 8 0.2376. The two pipes' heads and tails share
 * the SIMDs, and seven waves fit in any mix only when every kernel is at 72. */
#ifndef WCPT_TINY_HEAD_WAVES
#define WCPT_TINY_HEAD_WAVES 7
#endif
#ifndef WCPT_TINY_TAIL_WAVES
#define WCPT_TINY_TAIL_WAVES 7
#endif
/* For experiments (tools/ab_build.sh): dynamic LDS bytes per wave that the kernels never touch, which caps the waves
 * a CU holds at 160 KiB / this, with the same instruction stream. */
#ifndef WCPT_TINY_LDS_PAD
#define WCPT_TINY_LDS_PAD 0
#endif

constexpr int kTinyA = kArithExact;

/* One pixel of the head (pathTracer.comp:290-323; shade_pixel and TraceRay of a head, one sample): segments before
 * q.cut; a path still alive there goes to the queue and the tail stores its pixel, any other pixel is stored here. */
template <int PC>
__device__ __forceinline__ void tiny_head_pixel(const wcpt_scene_data& sd, const wcpt_material* __restrict__ mats,
                                                const wcpt_sphere* __restrict__ spheres,
                                                const wcpt_draw_command* __restrict__ draws,
                                                const uint64_t* __restrict__ tri_records, float4* __restrict__ image,
                                                float* __restrict__ wire, uint32_t wire_ch, uint32_t W, uint32_t H,
                                                const RowMap& rm, const RowMap& wm, uint32_t lx, uint32_t ly,
                                                uint32_t* __restrict__ pcache, const SplitQueue& q)
{
    constexpr int A = kTinyA;
    const uint32_t x = lx, y = frame_row(rm, ly); /* the frame row: a row block or interleaved stripes (row_map.h) */
    /* a read build takes the direction from the pixel's cache entry */
    f3 dir = mk3(0.0f, 0.0f, 0.0f);
    if constexpr (PC != kPrimCacheRead) dir = primary_direction(sd, x, y, W, H);
    const uint32_t pixel_index = x + y * W + sd.renderedFramesCount * 719393u; /* :304 */
    uint32_t rng = pcg_hash(pixel_index);
    const uint32_t pixel = (uint32_t)((size_t)ly * W + lx);
    const f3 origin = mk3(sd.position[0], sd.position[1], sd.position[2]);
    PathState ps;
    f3 L = mk3(0.0f, 0.0f, 0.0f);
    if constexpr (PC == kPrimCacheRead) {
        const PrimEntry entry = prim_cache_load(pcache);
        /* path_begin without the direction's reciprocal: path_shade sets invDirection before an intersect reads it */
        ps.ray.origin = origin;
        ps.ray.invDirection = mk3(0.0f, 0.0f, 0.0f);
        ps.totalLight = mk3(0.0f, 0.0f, 0.0f);
        ps.transmittance = mk3(1.0f, 1.0f, 1.0f);
        ps.bounce = 0;
        /* entered at path_shade with the entry's Hit: each turn shades segment `seg` and then intersects seg + 1 */
        Hit h = prim_entry_hit<kShadeA<A>>(entry, origin, ps.ray.direction);
        for (uint32_t seg = 0;; seg++) {
            const bool done = path_shade<kShadeA<A>>(ps, h, rng, sd, mats, L, true);
            if (seg + 1u == q.cut) { /* wave-uniform, as seg is */
                split_append(q, !done, ps, rng, pixel);
                if (!done) return;
                break;
            }
            if (done) break;
            h = tiny_intersect<A>(ps.ray, sd, spheres, draws, tri_records, false);
        }
    } else {
        path_begin<A>(ps, origin, dir);
        for (uint32_t seg = 0;; seg++) {
            /* segment 0 (origin = the camera) is the primary one for the whole wave */
            const Hit h = tiny_intersect<A>(ps.ray, sd, spheres, draws, tri_records, seg == 0u);
            if constexpr (PC == kPrimCacheWrite) {
                if (seg == 0u) prim_cache_store(pcache, ps.ray.direction, h);
            }
            const bool done = path_shade<kShadeA<A>>(ps, h, rng, sd, mats, L, true);
            if (seg + 1u == q.cut) { /* wave-uniform, as seg is */
                split_append(q, !done, ps, rng, pixel);
                if (!done) return;
                break;
            }
            if (done) break;
        }
    }
    /* The accumulation read (:314) behind the trace, unlike shade_pixel's, which reads ahead of it: there the four words are
     * live across every segment, registers that the floor of 7 would have to spill. The pixel is this lane's alone, in the
     * head or in the tail, so the value is the same; the other waves of the SIMD cover the read's latency, once per pixel. */
    float4 old = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sd.renderedFramesCount != 0) old = image[(size_t)ly * W + lx];
    /* shade_pixel's `result + TraceRay(...)` from a zero sum: the same addition, so a -0 radiance becomes +0 here too */
    accumulate_store(sd, image, wire, wire_ch, wm, W, lx, ly, old, mk3(0.0f, 0.0f, 0.0f) + L);
}

/* The head: pt_megakernel<..., PC, exact, head> on the walk. One 64-lane wave per pixel tile (pt_mk_tile.h). */
template <int PC>
__global__ __launch_bounds__(64, WCPT_TINY_HEAD_WAVES) void pt_tiny_head(
    const wcpt_scene_data sd, const wcpt_material* __restrict__ mats, const wcpt_sphere* __restrict__ spheres,
    const wcpt_draw_command* __restrict__ draws, const uint64_t* __restrict__ tri_records, float4* __restrict__ image,
    float* __restrict__ wire, uint32_t wire_ch, uint32_t W, uint32_t H, const RowMap rm, const RowMap wm, uint32_t rows,
    uint32_t tilesX, uint32_t tilesTotal, uint32_t scatter, const uint32_t* __restrict__ tile_order,
    uint32_t* __restrict__ tile_cost, uint32_t* __restrict__ prim_cache, const SplitQueue q)
{
    const uint64_t c0 = tile_cost ? __builtin_amdgcn_s_memtime() : 0ull;
    uint32_t tx, ty;
    tile_of_block(tilesX, tilesTotal, scatter, tile_order, tx, ty);
    const uint32_t lx = tx * kTileW + (threadIdx.x % kTileW);
    const uint32_t ly = ty * kTileH + (threadIdx.x / kTileW);
    /* the tile's primary-cache entries (primary_record.h): wave-uniform, the lane's offset is added at the use */
    uint32_t* const pcache = PC == kPrimCacheNone ? nullptr : prim_cache + primary_record_word(ty * tilesX + tx, 0u);
    if (lx < W && ly < rows)
        tiny_head_pixel<PC>(sd, mats, spheres, draws, tri_records, image, wire, wire_ch, W, H, rm, wm, lx, ly, pcache, q);
    if (tile_cost && (threadIdx.x & 63u) == 0u) {
        /* this tile's time, for the next renders' order: a running average, halved into the previous value */
        uint32_t* const tc = tile_cost + ty * tilesX + tx;
        const uint64_t c = (__builtin_amdgcn_s_memtime() - c0) >> 1;
        *tc = (*tc >> 1) + (c > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)c);
    }
}

/* The tail: pt_mk_tail<pairs, single, exact> on the walk. Wave b finishes the paths of queue entries [64 b, 64 b + 64),
 * one per lane, and stores their pixels. The grid is the queue's capacity; a wave past the count exits at once. */
__global__ __launch_bounds__(64, WCPT_TINY_TAIL_WAVES) void pt_tiny_tail(
    const wcpt_scene_data sd, const wcpt_material* __restrict__ mats, const wcpt_sphere* __restrict__ spheres,
    const wcpt_draw_command* __restrict__ draws, const uint64_t* __restrict__ tri_records, float4* __restrict__ image,
    float* __restrict__ wire, uint32_t wire_ch, uint32_t W, const RowMap wm, const SplitQueue q)
{
    constexpr int A = kTinyA;
    /* the pipe's next frame counts in the other counter (no memset between frames): zeroed here, behind the previous
     * frame's tail, which read it last, and before the next frame's head on the same stream */
    if (blockIdx.x == 0u)
        for (uint32_t s = threadIdx.x; s < kMkSplitSubQueues; s += 64u) q.count_next[s * kMkSplitCounterStride] = 0u;
    /* entries [64 c, 64 c + 64) of sub-queue j (mk_split_rule.h) */
    const uint32_t blocks = q.cap / 64u, j = blockIdx.x % kMkSplitSubQueues, c = blockIdx.x / kMkSplitSubQueues;
    const uint32_t n = min(q.count[j * kMkSplitCounterStride], mk_split_sub_cap(blocks, j));
    const uint32_t k = c * 64u + threadIdx.x;
    const uint32_t i = mk_split_sub_first(blocks, j) + k;
    if (k >= n || i >= q.cap) return;
    PathState ps;
    uint32_t rng, pixel;
    split_load<A>(q, i, ps, rng, pixel);
    /* TraceTail: from segment `cut` on, never a primary segment, the pixel's one and last sample */
    f3 L;
    for (;;) {
        const Hit h = tiny_intersect<A>(ps.ray, sd, spheres, draws, tri_records, false);
        if (path_shade<kShadeA<A>>(ps, h, rng, sd, mats, L, true)) break;
    }
    /* the pixel's coordinates and its accumulation read behind the trace, as in the head: six registers that the
     * segments do not hold (77 -> 73 VGPRs of its own; the floor takes the last one) */
    const uint32_t lx = pixel % W, ly = pixel / W;
    float4 old = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sd.renderedFramesCount != 0) old = image[pixel];
    accumulate_store(sd, image, wire, wire_ch, wm, W, lx, ly, old, mk3(0.0f, 0.0f, 0.0f) + L);
}

} // namespace dev

static_assert(dev::kPrimCacheNone == kPrimaryCacheNone && dev::kPrimCacheWrite == kPrimaryCacheWrite &&
                  dev::kPrimCacheRead == kPrimaryCacheRead, "primary-cache modes");

template <int PC>
static hipError_t launch_tiny_head_pc(const LaunchArgs& a, const TinyHeadLaunch& h, const dev::SplitQueue& q,
                                      hipStream_t stream)
{
    hipLaunchKernelGGL((dev::pt_tiny_head<PC>), dim3(h.grid), dim3(64), WCPT_TINY_LDS_PAD, stream, a.sd, a.materials,
                       a.spheres, a.draws, a.tri_records, a.image, a.wire, a.wire_ch, a.W, a.H,
                       RowMap{a.y0, a.row_shift, a.row_gap}, a.wire_rows, a.rows, h.tilesX, h.tiles, h.scatter, h.order,
                       h.cost, h.prim_cache, q);
    return hipGetLastError();
}

hipError_t launch_tiny_head(const LaunchArgs& a, int pcmode, const TinyHeadLaunch& h, const dev::SplitQueue& q,
                            hipStream_t stream)
{
    switch (pcmode) {
    case kPrimaryCacheNone: return launch_tiny_head_pc<kPrimaryCacheNone>(a, h, q, stream);
    case kPrimaryCacheWrite: return launch_tiny_head_pc<kPrimaryCacheWrite>(a, h, q, stream);
    case kPrimaryCacheRead: return launch_tiny_head_pc<kPrimaryCacheRead>(a, h, q, stream);
    default: return hipErrorInvalidValue; /* no such kernel */
    }
}

hipError_t launch_tiny_tail(const LaunchArgs& a, const dev::SplitQueue& q, hipStream_t stream)
{
    hipLaunchKernelGGL(dev::pt_tiny_tail, dim3((q.cap + 63u) / 64u), dim3(64), WCPT_TINY_LDS_PAD, stream, a.sd,
                       a.materials, a.spheres, a.draws, a.tri_records, a.image, a.wire, a.wire_ch, a.W, a.wire_rows, q);
    return hipGetLastError();
}

} // namespace wcpt
