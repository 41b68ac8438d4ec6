/* pt_path.h -- the megakernel's segment loops and the pixel's output: the split queue, TraceTail, TraceRay, the primary
 * ray direction, the display transform and store_pixel. Part of pt_device.h. */
#ifndef WCPT_PT_PATH_H
#define WCPT_PT_PATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wcpt.h"
#include "mk_split_rule.h"
#include "pt_counters.h"
#include "pt_shading.h"
#include "pt_traversal.h"
#include "row_map.h"
#include "wcpt_composite.h"

namespace wcpt::dev {

/* Split launches (WCPT_OPTION_MK_SPLIT, mk_split_rule.h): the one-sample render runs as a head launch, which traces the
 * segments before `cut` and appends the paths still alive to a queue, and a tail launch, which finishes them one per
 * lane in full waves (pt_kernels.hip pt_mk_tail). An entry is the PathState between two segments without
 * invDirection (the tail takes the same rcp3_a of the same direction), the RNG word and the pixel's image index:
 * kSplitWords arrays of `cap` u32 (structure of arrays, so a wave's survivors are one contiguous run of each). `cap`
 * is the launch's lanes, so an append cannot pass it; the stores are guarded all the same. The queue is divided into
 * sub-queues with a counter each (mk_split_rule.h mk_split_sub_first has why and how). */
constexpr int kStageWhole = 0, kStageHead = 1, kStageTail = 2;
constexpr uint32_t kSplitWords = 14;
struct SplitQueue {
    uint32_t* state;      /* kSplitWords arrays of cap u32 */
    uint32_t* count;      /* this frame's counter set (sub-queue j's entries at j * kMkSplitCounterStride): the head
                             adds to it, the tail reads it */
    uint32_t* count_next; /* the counter set of the pipe's next frame: the tail zeroes it */
    uint32_t cap;
    uint32_t cut;         /* the head leaves the segment loop before segment `cut` (>= 1) */
};
/* the queue argument of a megakernel instance: only the head has one */
struct NoSplitQueue {};
template <int STAGE> struct StageQueue { typedef NoSplitQueue type; };
template <> struct StageQueue<kStageHead> { typedef SplitQueue type; };

/* Every lane still in the segment loop calls it; the lanes with `alive` append to the block's sub-queue: one atomicAdd
 * per wave, entries at base + rank. */
__device__ __forceinline__ void split_append(const SplitQueue& q, bool alive, const PathState& ps, uint32_t rng,
                                             uint32_t pixel)
{
    const unsigned long long m = __ballot(alive);
    if (m == 0ull) return;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int leader = __ffsll(m) - 1;
    uint32_t base = 0u;
    const uint32_t blocks = q.cap / 64u, j = blockIdx.x % kMkSplitSubQueues;
    if ((int)(threadIdx.x & 63u) == leader)
        base = atomicAdd(q.count + j * kMkSplitCounterStride, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    const uint32_t k = base + rank, i = mk_split_sub_first(blocks, j) + k;
    if (alive && k < mk_split_sub_cap(blocks, j) && i < q.cap) {
        uint32_t* s = q.state + i;
        const size_t c = q.cap;
        s[0 * c] = __float_as_uint(ps.ray.origin.x);
        s[1 * c] = __float_as_uint(ps.ray.origin.y);
        s[2 * c] = __float_as_uint(ps.ray.origin.z);
        s[3 * c] = __float_as_uint(ps.ray.direction.x);
        s[4 * c] = __float_as_uint(ps.ray.direction.y);
        s[5 * c] = __float_as_uint(ps.ray.direction.z);
        s[6 * c] = __float_as_uint(ps.totalLight.x);
        s[7 * c] = __float_as_uint(ps.totalLight.y);
        s[8 * c] = __float_as_uint(ps.totalLight.z);
        s[9 * c] = __float_as_uint(ps.transmittance.x);
        s[10 * c] = __float_as_uint(ps.transmittance.y);
        s[11 * c] = __float_as_uint(ps.transmittance.z);
        s[12 * c] = rng;
        s[13 * c] = pixel;
    }
}

/* The tail's side of split_append: entry i of the queue; ps.bounce is the cut (every path that reaches segment `cut`
 * has bounced `cut` times: path_shade), which is why the entry does not hold it. */
template <int A>
__device__ __forceinline__ void split_load(const SplitQueue& q, uint32_t i, PathState& ps, uint32_t& rng, uint32_t& pixel)
{
    const uint32_t* s = q.state + i;
    const size_t c = q.cap;
    ps.ray.origin = mk3(__uint_as_float(s[0 * c]), __uint_as_float(s[1 * c]), __uint_as_float(s[2 * c]));
    ps.ray.direction = mk3(__uint_as_float(s[3 * c]), __uint_as_float(s[4 * c]), __uint_as_float(s[5 * c]));
    ps.ray.invDirection = rcp3_a<kShadeA<A>>(ps.ray.direction); /* path_shade's, of the same bits */
    ps.totalLight = mk3(__uint_as_float(s[6 * c]), __uint_as_float(s[7 * c]), __uint_as_float(s[8 * c]));
    ps.transmittance = mk3(__uint_as_float(s[9 * c]), __uint_as_float(s[10 * c]), __uint_as_float(s[11 * c]));
    ps.bounce = q.cut;
    rng = s[12 * c];
    pixel = s[13 * c];
}

/* The tail's segment loop: TraceRay's from segment `cut` on (never a primary segment, no primary cache, the pixel's
 * one and last sample). */
template <bool PAIRS, bool SINGLE, class Stack, int A>
__device__ __forceinline__ f3 TraceTail(PathState& ps, uint32_t& rng, const wcpt_scene_data& sd,
                                        const wcpt_material* __restrict__ mats, const wcpt_sphere* __restrict__ spheres,
                                        const wcpt_draw_command* __restrict__ draws,
                                        const uint64_t* __restrict__ tri_records, Stack& stk, Counters& cnt,
                                        bool& overflow)
{
    f3 L;
    float4 prim_rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (;;) {
        const Hit h = intersect<false, false, PAIRS, SINGLE, Stack, A>(ps.ray, sd, spheres, draws, tri_records, stk, cnt,
                                                                      overflow, false, prim_rec, false);
        if (path_shade<kShadeA<A>>(ps, h, rng, sd, mats, L, true)) return L;
    }
}

/* pathTracer.comp:241-284. prim_rec: the primary segment's Intersect record (t, primitive, draw), written by the
 * first sample; reuse_primary: a later sample, whose primary segment reads it instead of tracing the same ray again
 * (intersect). STAGE == kStageHead: the loop ends before segment q->cut, and the lanes whose path is still alive there
 * append it to the queue (`pixel`: its image index) and return with `appended` set.
 * Primary cache (pt_traversal.h): a write build stores sample 0's resolved primary segment right after its intersect,
 * where the direction and the Hit are in registers. A read build gets the pixel's entry instead of a direction
 * (ray.direction and ray.invDirection are not read): segment 0 is path_shade on the entry's Hit, from the camera along
 * the entry's direction, and has no intersect -- its half of the loop is peeled off, so nothing of the entry is
 * loop-carried -- and no intersect of that kernel is a primary segment's. */
template <bool COUNT, bool DIAG, bool PAIRS, bool SINGLE, class Stack, bool REUSE = false, int PC = kPrimCacheNone,
          int A = kArithExact, int STAGE = kStageWhole>
__device__ __forceinline__ f3 TraceRay(Ray ray, uint32_t& rng, const wcpt_scene_data& sd,
                                       const wcpt_material* __restrict__ mats, const wcpt_sphere* __restrict__ spheres,
                                       const wcpt_draw_command* __restrict__ draws,
                                       const uint64_t* __restrict__ tri_records, Stack& stk,
                                       Counters& cnt, bool& overflow, bool lastSample, float4& prim_rec,
                                       bool reuse_primary, uint32_t* __restrict__ pcache = nullptr,
                                       const SplitQueue* q = nullptr, uint32_t pixel = 0u, bool* appended = nullptr,
                                       const PrimEntry* entry = nullptr)
{
    PathState ps;
    f3 L;
    if constexpr (STAGE == kStageHead) L = mk3(0.0f, 0.0f, 0.0f); /* what an appending lane returns (not read) */
    if constexpr (PC == kPrimCacheRead) {
        /* path_begin without the direction's reciprocal: path_shade sets invDirection before an intersect reads it */
        ps.ray.origin = ray.origin;
        ps.ray.invDirection = mk3(0.0f, 0.0f, 0.0f);
        ps.totalLight = mk3(0.0f, 0.0f, 0.0f);
        ps.transmittance = mk3(1.0f, 1.0f, 1.0f);
        ps.bounce = 0;
        /* the loop below, entered at its path_shade with the entry's Hit: each turn shades segment `seg` and then
         * intersects segment seg + 1, so the kernel holds one path_shade and one intersect as before */
        Hit h = prim_entry_hit<kShadeA<A>>(*entry, ray.origin, ps.ray.direction);
        for (uint32_t seg = 0;; seg++) {
            const bool done = path_shade<kShadeA<A>>(ps, h, rng, sd, mats, L, lastSample);
            phase_mark(cnt, 5);
            if constexpr (STAGE == kStageHead) {
                if (seg + 1u == q->cut) { /* wave-uniform, as seg is */
                    split_append(*q, !done, ps, rng, pixel);
                    *appended = !done;
                    return L;
                }
            }
            if (done) return L;
            h = intersect<COUNT, DIAG, PAIRS, SINGLE, Stack, A>(ps.ray, sd, spheres, draws, tri_records, stk, cnt,
                                                                      overflow, false, prim_rec, false);
        }
    } else {
    path_begin<A>(ps, ray.origin, ray.direction);
    /* segment counter of this sample: uniform across the wave's lanes (all start a sample together), so `primary`
     * (segment 0: origin = the camera) is a wave-uniform branch condition */
    for (uint32_t seg = 0;; seg++) {
        const bool primary = seg == 0u;
        const bool reuse = REUSE && seg == 0u && reuse_primary;
        const Hit h = intersect<COUNT, DIAG, PAIRS, SINGLE, Stack, A>(ps.ray, sd, spheres, draws, tri_records, stk, cnt,
                                                                      overflow, primary, prim_rec, reuse);
        /* a traced primary segment: sample 0's. (The sample-reuse write build keeps the Intersect record in prim_rec
         * anyway and stores from the caller, after its sample loop: with the store here this toolchain's register
         * allocator crashes on that instance.) */
        if constexpr (PC == kPrimCacheWrite && !REUSE) {
            if (seg == 0u && !reuse_primary) prim_cache_store(pcache, ps.ray.direction, h);
        }
        const bool done = path_shade<kShadeA<A>>(ps, h, rng, sd, mats, L, lastSample);
        phase_mark(cnt, 5);
        if constexpr (STAGE == kStageHead) {
            if (seg + 1u == q->cut) { /* wave-uniform, as seg is */
                split_append(*q, !done, ps, rng, pixel);
                *appended = !done;
                return L;
            }
        }
        if (done) return L;
    }
    }
}

/* pathTracer.comp:290-302 — primary ray direction for pixel (x, y) of a W x H frame. */
__device__ __forceinline__ f3 primary_direction(const wcpt_scene_data& sd, uint32_t x, uint32_t y, uint32_t W, uint32_t H)
{
    const float imgW = (float)W, imgH = (float)H;
    float cx = (float)x / imgW, cy = (float)y / imgH;
    cx = cx + (1.0f / imgW) * 0.5f;
    cy = cy + (1.0f / imgH) * 0.5f;
    cy = 1.0f - cy;
    cx = cx * 2.0f - 1.0f;
    cy = cy * 2.0f - 1.0f;
    const float* P = sd.inverseProjection;
    float tg[4];
#pragma unroll
    for (int r = 0; r < 4; r++) tg[r] = P[0 * 4 + r] * cx + P[1 * 4 + r] * cy + P[2 * 4 + r] * 1.0f + P[3 * 4 + r] * 1.0f;
    const f3 d = normalize(mk3(tg[0], tg[1], tg[2]) / tg[3]);
    const float* V = sd.inverseView;
    float wd[3];
#pragma unroll
    for (int r = 0; r < 3; r++) wd[r] = V[0 * 4 + r] * d.x + V[1 * 4 + r] * d.y + V[2 * 4 + r] * d.z + V[3 * 4 + r] * 0.0f;
    return normalize(mk3(wd[0], wd[1], wd[2]));
}

/* Final store of a pixel (pathTracer.comp:323, `vec4(acc, 1)`): the accumulation image, plus the gather payload
 * (wcpt_set_gather_output) when the host asked for one, same row-major pixel index: RGB (3 floats), RGBA (4 floats),
 * or WCPT_PAYLOAD_DISPLAY_RGBA8 -- the display step of composite.comp:36-53 (gamma 1/2.2 + PBR Neutral, then UNORM8)
 * applied to the accumulated value as it is stored, so a multi-device frame travels at 4 B/px
 * with no composite pass over the image. */
__device__ __noinline__ uint32_t display_rgba8(f3 acc)
{
    const float in[4] = {acc.x, acc.y, acc.z, 1.0f};
    float o[4];
    wcpt_composite_texel(in, o);
    return (uint32_t)wcpt_unorm8(o[0]) | ((uint32_t)wcpt_unorm8(o[1]) << 8) | ((uint32_t)wcpt_unorm8(o[2]) << 16) |
           (255u << 24);
}
/* Gather-output rows (row_map.h): the map {0, 31, 0} (row = ly) addresses a payload that holds the context's rows back
 * to back; the context's own row map addresses a whole frame (WCPT_OPTION_GATHER_FRAME_ROWS). */

/* :323 imageStore of pixel (lx, ly) of the context's rows into the accumulation image (index i = ly * W + lx), and
 * into the gather output (wcpt_set_gather_output) at row frame_row(wm, ly) of that output */
__device__ __forceinline__ void store_pixel(float4* __restrict__ image, float* __restrict__ wire, uint32_t wire_ch,
                                            const RowMap& wm, uint32_t W, uint32_t lx, uint32_t ly, f3 acc)
{
    const size_t i = (size_t)ly * W + lx;
    image[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
    if (wire) {
        const size_t j = (size_t)frame_row(wm, ly) * W + lx;
        if (wire_ch == 3u) {
            float* w = wire + 3u * j;
            w[0] = acc.x;
            w[1] = acc.y;
            w[2] = acc.z;
        } else if (wire_ch == 4u) {
            reinterpret_cast<float4*>(wire)[j] = make_float4(acc.x, acc.y, acc.z, 1.0f);
        } else {
            reinterpret_cast<uint32_t*>(wire)[j] = display_rgba8(acc);
        }
    }
}

} // namespace wcpt::dev

#endif /* WCPT_PT_PATH_H */
