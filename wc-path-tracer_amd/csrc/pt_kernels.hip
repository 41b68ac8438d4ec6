/*
 * pt_kernels.hip — the path-tracing megakernel for gfx950 (reference: src/shaders/pathTracer.comp:286-324).
 *
 * Launch shape: one 64-lane wave per 8x8 pixel tile (the reference's 4x4 = 16-invocation workgroups would
 * leave 48 of 64 lanes idle on wave64 CDNA). A bounds guard makes any width/height legal (the reference
 * has none, :289). SceneData arrives by value in the kernarg segment.
 *
 * Instantiations: COUNT=false renders; COUNT=true runs the same frame without writing the image and counts the
 * reference algorithm's work; DIAG=true additionally counts SIMD lane/wave steps with a
 * __ballot inside the traversal loop (tools/diag.py only — kept out of the COUNT build the parity tests use).
 * The render builds come in three primary-cache modes (PC; pt_device.h TraceRay, primary_cache_key.h): none, write
 * (stores each pixel's resolved primary segment, primary_record.h) and read (shades the primary segment from it).
 * mk_variant.h is the list of the instances: 96 render, 24 head (the first launch of a split render) and 16 counting
 * instances of pt_megakernel and 8 of pt_mk_tail; the dispatcher below (mk_dispatch) instantiates exactly those.
 * Four more kernels are no instances of these and live in pt_mk_tiny.hip: pt_tiny_head<PC none / write / read> and
 * pt_tiny_tail, the head and the tail of a split render whose one draw has a tiny tree (mk_tiny_rule.h
 * mk_tiny_kernels), which hold the tiny-tree walk and nothing of the traversal loop; launch_megakernel takes them in the
 * places of the head and tail that mk_variant_select chose. The kernels here hold nothing of the walk.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <utility>

#include "mk_tiny_rule.h"
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_mk_tile.h"
#include "pt_mk_tiny.h"

namespace wcpt {
namespace dev {

/* Shade one pixel (pathTracer.comp:290-323) with the given traversal stack. */
template <bool COUNT, bool DIAG, bool PAIRS, bool SINGLE, bool REUSE, int PC, int A, int STAGE, class Stack>
__device__ __forceinline__ void shade_pixel(const wcpt_scene_data& sd, const wcpt_material* __restrict__ mats,
                                            const wcpt_sphere* __restrict__ spheres,
                                            const wcpt_draw_command* __restrict__ draws,
                                            const uint64_t* __restrict__ tri_records, float4* __restrict__ image,
                                            float* __restrict__ wire, uint32_t wire_ch,
                                            uint32_t W, uint32_t H, const RowMap& rm, const RowMap& wm, uint32_t lx,
                                            uint32_t ly, Stack& stk, Counters& cnt, bool& overflow,
                                            uint32_t* __restrict__ pcache,
                                            const typename StageQueue<STAGE>::type& q)
{
    const uint32_t x = lx, y = frame_row(rm, ly); /* the frame row: a row block or interleaved stripes (row_map.h) */
    /* a read build takes the direction from the pixel's cache entry (TraceRay) */
    f3 dir = mk3(0.0f, 0.0f, 0.0f);
    if constexpr (PC != kPrimCacheRead) dir = primary_direction(sd, x, y, W, H);
    const uint32_t pixel_index = x + y * W + sd.renderedFramesCount * 719393u; /* :304 */
    uint32_t seed = pcg_hash(pixel_index);
    /* The accumulation read (:314) is issued before the trace, so its HBM latency hides behind the segments
     * instead of stalling the wave at its end (the image is the one buffer that does not live in L2). */
    float4* px = image + (size_t)ly * W + lx;
    float4 old = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!COUNT && sd.renderedFramesCount != 0) old = *px;
    phase_mark(cnt, 0);
    f3 result = mk3(0.0f, 0.0f, 0.0f);
    const f3 origin = mk3(sd.position[0], sd.position[1], sd.position[2]);
    float4 prim_rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f); /* sample 0's primary Intersect record (sample reuse) */
    /* the resolved primary segment as an earlier frame stored it (primary_record.h): loaded beside the image read. The
     * sample-reuse read build loads it again for every sample instead of holding its 8 registers across the loop */
    PrimEntry entry = {};
    if constexpr (PC == kPrimCacheRead && !REUSE) entry = prim_cache_load(pcache);
    /* the one-sample read build (mk_variant.h mk_variant_select) has its sample count as a constant */
    /* so has a head launch (STAGE; the runtime splits one-sample renders only) */
    const uint32_t samples = ((PC == kPrimCacheRead && !REUSE) || STAGE == kStageHead) ? 1u : sd.samples;
    bool appended = false; /* head: the path went to the tail's queue, and the tail stores this pixel */
    const SplitQueue* qp = nullptr;
    if constexpr (STAGE == kStageHead) qp = &q;
    for (uint32_t s = 0; s < samples; s++) { /* :309-310, all samples share the primary ray */
        Ray r;
        r.origin = origin;
        r.direction = dir;
        if constexpr (PC == kPrimCacheRead) {
            r.invDirection = dir; /* neither is read (TraceRay) */
            if constexpr (REUSE) {
                /* through an opaque copy of the (wave-uniform) pointer: a plain load is loop-invariant, and the
                 * compiler then hoists it and holds the 8 registers across the sample loop after all */
                uint32_t* pc = pcache;
                asm volatile("" : "+s"(pc));
                entry = prim_cache_load(pc);
            }
        } else {
            r.invDirection = rcp3(dir);
        }
        if constexpr (STAGE == kStageHead)
            result = result + TraceRay<COUNT, DIAG, PAIRS, SINGLE, Stack, REUSE, PC, A, STAGE>(r, seed, sd, mats, spheres, draws, tri_records, stk, cnt, overflow,
                                                           s + 1u == samples, prim_rec, s > 0u, pcache, qp,
                                                           (uint32_t)((size_t)ly * W + lx), &appended, &entry);
        else
            result = result + TraceRay<COUNT, DIAG, PAIRS, SINGLE, Stack, REUSE, PC, A>(r, seed, sd, mats, spheres, draws, tri_records, stk, cnt, overflow,
                                                           s + 1u == samples, prim_rec, s > 0u, pcache, nullptr, 0u, nullptr,
                                                           &entry);
    }
    if constexpr (STAGE == kStageHead) {
        if (appended) return;
    }
    if constexpr (PC == kPrimCacheWrite && REUSE) {
        /* this build (samples > 1) holds sample 0's Intersect record in prim_rec (intersect): the entry is resolve_hit
         * of it and the primary ray once more -- the same function on the same bits as in sample 0's intersect */
        Ray r;
        r.origin = origin;
        r.direction = dir;
        r.invDirection = dir; /* not read */
        const Hit h = resolve_hit<kShadeA<A>>(r, prim_rec.x, __float_as_uint(prim_rec.y), __float_as_uint(prim_rec.z),
                                              spheres, draws, tri_records);
        prim_cache_store(pcache, dir, h);
    }
    if (!COUNT) accumulate_store(sd, image, wire, wire_ch, wm, W, lx, ly, old, result);
    if (COUNT) cnt.pixels++;
    phase_mark(cnt, 6);
}

/* Stack kinds: 0 = private (scratch) stack of kPrivateStack entries; 1 = LDS stack of kLdsStack entries per
 * lane with a kSpillStack-entry private spill. */
/* Occupancy floor for experiments (tools/ab_build.sh): __launch_bounds__'s minimum waves per SIMD. */
#ifndef WCPT_MK_WAVES
#define WCPT_MK_WAVES 1
#endif
/* A: the arithmetic mode (pt_device.h kArithExact / kArithFast, WCPT_OPTION_ARITH). A template parameter, so the fast
 * and the exact kernel of one configuration are two symbols; render builds only.
 * The nine template parameters are the fields of an MkVariant: mk_variant.h states which combinations are instantiated
 * (mk_variant_built: 136 of this kernel and 8 of pt_mk_tail per code object) and which one a launch takes. */
template <bool COUNT, bool DIAG, int SK, bool PAIRS, bool SINGLE, bool REUSE, int PC, int A, int STAGE>
__global__ __launch_bounds__(64, WCPT_MK_WAVES) void pt_megakernel(const wcpt_scene_data sd, const wcpt_material* __restrict__ mats,
                                                    const wcpt_sphere* __restrict__ spheres,
                                                    const wcpt_draw_command* __restrict__ draws,
                                                    const uint64_t* __restrict__ tri_records,
                                                    float4* __restrict__ image, float* __restrict__ wire,
                                                    uint32_t wire_ch, uint32_t W, uint32_t H, const RowMap rm,
                                                    const RowMap wm, uint32_t rows, uint32_t tilesX, uint32_t tilesTotal,
                                                    uint32_t scatter, const uint32_t* __restrict__ tile_order,
                                                    uint32_t* __restrict__ tile_cost, uint32_t* __restrict__ status,
                                                    unsigned long long* __restrict__ counters,
                                                    uint32_t* __restrict__ prim_cache,
                                                    const typename StageQueue<STAGE>::type q)
{
    const uint64_t c0 = (!COUNT && tile_cost) ? __builtin_amdgcn_s_memtime() : 0ull;
    uint32_t tx, ty;
    tile_of_block(tilesX, tilesTotal, scatter, tile_order, tx, ty);
    const uint32_t lx = tx * kTileW + (threadIdx.x % kTileW);
    const uint32_t ly = ty * kTileH + (threadIdx.x / kTileW);
    Counters cnt = {};
    phase_start(cnt);
    bool overflow = false;
    /* the tile's primary-cache entries (primary_record.h): wave-uniform, the lane's offset is added at the use */
    uint32_t* const pcache = PC == kPrimCacheNone ? nullptr
        : prim_cache + primary_record_word(ty * tilesX + tx, 0u);
    if (lx < W && ly < rows) {
        if constexpr (SK == 0) {
            uint64_t mem[kPrivateStack];
            PrivateStack<kPrivateStack> stk;
            stk.mem = (priv_u64_ptr)mem;
            shade_pixel<COUNT, DIAG, PAIRS, SINGLE, REUSE, PC, A, STAGE>(sd, mats, spheres, draws, tri_records, image, wire, wire_ch, W, H, rm, wm, lx, ly, stk,
                                            cnt, overflow, pcache, q);
        } else {
            __shared__ uint64_t s_stack[kLdsStack * 64];
            uint64_t spill[kSpillStack];
            LdsStack<kLdsStack, kSpillStack> stk;
            stk.base = (lds_u64_ptr)(s_stack + (threadIdx.x & 63u));
            stk.spill = (priv_u64_ptr)spill;
            shade_pixel<COUNT, DIAG, PAIRS, SINGLE, REUSE, PC, A, STAGE>(sd, mats, spheres, draws, tri_records, image, wire, wire_ch, W, H, rm, wm, lx, ly, stk,
                                            cnt, overflow, pcache, q);
        }
    }
    if (overflow) atomicOr(status, 1u);
    flush_counters<COUNT>(cnt, counters);
    if (!COUNT && tile_cost && (threadIdx.x & 63u) == 0u) {
        /* this tile's time, for the next renders' order: a running average (each frame draws new bounce directions,
         * the primary rays repeat), halved into the previous value */
        uint32_t* const tc = tile_cost + ty * tilesX + tx;
        const uint64_t c = (__builtin_amdgcn_s_memtime() - c0) >> 1;
        *tc = (*tc >> 1) + (c > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)c);
    }
#if WCPT_MK_TIMERS
    if (!COUNT && (threadIdx.x & 63u) == 0u)
        for (int k = 0; k < kPhaseTimers; k++) atomicAdd(&counters[k], (unsigned long long)cnt.tim[k]);
#endif
}

/* The tail of a split render (pt_device.h SplitQueue): wave b finishes the paths of queue entries [64 b, 64 b + 64), one
 * per lane, and stores their pixels as the whole kernel does, gather payload included. The grid is the queue's
 * capacity (the host never reads the count); a wave past the count exits at once. LDS stack, like its head. */
template <bool PAIRS, bool SINGLE, int A>
__global__ __launch_bounds__(64, WCPT_MK_WAVES) void pt_mk_tail(const wcpt_scene_data sd, const wcpt_material* __restrict__ mats,
                                                 const wcpt_sphere* __restrict__ spheres,
                                                 const wcpt_draw_command* __restrict__ draws,
                                                 const uint64_t* __restrict__ tri_records, float4* __restrict__ image,
                                                 float* __restrict__ wire, uint32_t wire_ch, uint32_t W, const RowMap wm,
                                                 uint32_t* __restrict__ status, const SplitQueue q)
{
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
    const uint32_t lx = pixel % W, ly = pixel / W;
    /* the accumulation read first, as in shade_pixel */
    float4 old = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sd.renderedFramesCount != 0) old = image[pixel];
    __shared__ uint64_t s_stack[kLdsStack * 64];
    uint64_t spill[kSpillStack];
    LdsStack<kLdsStack, kSpillStack> stk;
    stk.base = (lds_u64_ptr)(s_stack + (threadIdx.x & 63u));
    stk.spill = (priv_u64_ptr)spill;
    Counters cnt = {};
    bool overflow = false;
    /* shade_pixel's `result + TraceRay(...)` from a zero sum: the same addition, so a -0 radiance becomes +0 here too */
    const f3 result = mk3(0.0f, 0.0f, 0.0f) +
                      TraceTail<PAIRS, SINGLE, LdsStack<kLdsStack, kSpillStack>, A>(ps, rng, sd, mats, spheres, draws,
                                                                                   tri_records, stk, cnt, overflow);
    accumulate_store(sd, image, wire, wire_ch, wm, W, lx, ly, old, result);
    if (overflow) atomicOr(status, 1u);
}

/* Derived triangle records (pt_device.h), single and pair formats: one thread per pair. Same subtractions as
 * rayTriangleE's edges (:122-123). The second slot of the last pair of an odd count is NaN (never inside a leaf's range:
 * leaf_record bounds leaves by the triangle count). A vertex index past the vertex buffer gives NaN vertices. */
__device__ __forceinline__ void tri_fields(const uint32_t* __restrict__ idx, const float* __restrict__ vtx, uint32_t nvert,
                                           uint64_t k, float f[9])
{
    const uint32_t ia = idx[3ull * k + 0], ib = idx[3ull * k + 1], ic = idx[3ull * k + 2];
    const float qnan = __uint_as_float(0x7fc00000u);
    const f3 nan3 = mk3(qnan, qnan, qnan);
    const f3 a = ia < nvert ? ld3(vtx + 3ull * ia) : nan3;
    const f3 b = ib < nvert ? ld3(vtx + 3ull * ib) : nan3;
    const f3 c = ic < nvert ? ld3(vtx + 3ull * ic) : nan3;
    const f3 e1 = b - a, e2 = c - a;
    f[0] = a.x; f[1] = a.y; f[2] = a.z;
    f[3] = e1.x; f[4] = e1.y; f[5] = e1.z;
    f[6] = e2.x; f[7] = e2.y; f[8] = e2.z;
}

/* The BVH's leaves against the fast layout's assumptions (bits: frame_prep.h): *flags |= kLeafScanBigLeaf when some leaf
 * has triangleCount >= kRefFetch (a stack entry of it would not carry its count), |= kLeafScanOffRecords when some leaf
 * does not start at a triangle boundary or reaches past the draw's derived records (first % 3 != 0 or first + count >
 * lim3 = 3 * triangles: its triangles would need the index path). */
__global__ __launch_bounds__(256) void scan_leaf_counts(const wcpt_node* __restrict__ bvh, uint32_t nodes, uint32_t lim3,
                                                        uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nodes) return;
    const uint32_t first = bvh[i].leftNodeOrTriangleIndex, count = bvh[i].triangleCount;
    if (count == 0u) return;
    uint32_t f = count >= kRefFetch ? kLeafScanBigLeaf : 0u;
    if (first % 3u != 0u || first > lim3 || count > lim3 - first) f |= kLeafScanOffRecords;
    if (f) atomicOr(flags, f);
}

/* The tiny-tree rule (mk_tiny_rule.h) on the BVH buffer's nodes: *flags |= kLeafScanTinyTree for a root leaf or a root
 * over two leaves, each on the draw's derived records. One thread; behind scan_leaf_counts on the same stream. */
__global__ void scan_tiny_tree(const wcpt_node* __restrict__ bvh, uint32_t nodes, uint32_t lim3, uint32_t* __restrict__ flags)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u && mk_tiny_leaves(bvh, nodes, lim3) != 0u) atomicOr(flags, kLeafScanTinyTree);
}

__global__ __launch_bounds__(256) void build_tri_records(const uint32_t* __restrict__ idx, const float* __restrict__ vtx,
                                                         uint32_t ntri, uint32_t nvert, float4* __restrict__ singles,
                                                         float4* __restrict__ out)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (2ull * j >= ntri) return;
    float v[2][9];
    for (uint32_t h = 0; h < 2; h++) {
        const uint64_t k = 2ull * j + h;
        if (k >= ntri) {
            for (int c = 0; c < 9; c++) v[h][c] = __uint_as_float(0x7fc00000u);
            continue;
        }
        tri_fields(idx, vtx, nvert, k, v[h]);
        const f3 e1 = mk3(v[h][3], v[h][4], v[h][5]), e2 = mk3(v[h][6], v[h][7], v[h][8]);
        const f3 n = normalize(cross(e1, e2)); /* :173 */
        singles[3ull * k + 0] = make_float4(v[h][0], v[h][1], v[h][2], v[h][3]);
        singles[3ull * k + 1] = make_float4(v[h][4], v[h][5], v[h][6], v[h][7]);
        singles[3ull * k + 2] = make_float4(v[h][8], n.x, n.y, n.z);
    }
    float4* o = out + (uint64_t)kPairRecordFloat4s * j;
    o[0] = make_float4(v[0][0], v[1][0], v[0][1], v[1][1]);
    o[1] = make_float4(v[0][2], v[1][2], v[0][3], v[1][3]);
    o[2] = make_float4(v[0][4], v[1][4], v[0][5], v[1][5]);
    o[3] = make_float4(v[0][6], v[1][6], v[0][7], v[1][7]);
    o[4] = make_float4(v[0][8], v[1][8], 0.0f, 0.0f);
}

/* Primary-ray pair records from pair records (one thread per pair): the origin terms of both triangles with
 * primary_terms, the same operations as rayTrianglePair's for that origin. */
__global__ __launch_bounds__(256) void build_primary_pairs(const float4* __restrict__ pairs, uint32_t npairs, float ox,
                                                           float oy, float oz, float4* __restrict__ out)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= npairs) return;
    const float4* q = pairs + (uint64_t)kPairRecordFloat4s * j;
    const float4 r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
    /* pair record: (ax, ay) (az, e1x) (e1y, e1z) (e2x, e2y) (e2z, pad) as {tri 2j, tri 2j+1} float2 */
    const float ax[2] = {r0.x, r0.y}, ay[2] = {r0.z, r0.w}, az[2] = {r1.x, r1.y}, e1x[2] = {r1.z, r1.w};
    const float e1y[2] = {r2.x, r2.y}, e1z[2] = {r2.z, r2.w}, e2x[2] = {r3.x, r3.y}, e2y[2] = {r3.z, r3.w};
    const float e2z[2] = {r4.x, r4.y};
    float t[2][7];
    for (int h = 0; h < 2; h++)
        primary_terms(ox, oy, oz, ax[h], ay[h], az[h], e1x[h], e1y[h], e1z[h], e2x[h], e2y[h], e2z[h], t[h]);
    float4* o = out + (uint64_t)kPrimPairFloat4s * j;
    o[0] = make_float4(e1x[0], e1x[1], e1y[0], e1y[1]);
    o[1] = make_float4(e1z[0], e1z[1], e2x[0], e2x[1]);
    o[2] = make_float4(e2y[0], e2y[1], e2z[0], e2z[1]);
    o[3] = make_float4(t[0][0], t[1][0], t[0][1], t[1][1]); /* oax, oay */
    o[4] = make_float4(t[0][2], t[1][2], t[0][3], t[1][3]); /* oaz, qx */
    o[5] = make_float4(t[0][4], t[1][4], t[0][5], t[1][5]); /* qy, qz */
    o[6] = make_float4(t[0][6], t[1][6], 0.0f, 0.0f);       /* tq */
}

} // namespace dev

/* ------------------------------------------------------------------------------------------------ */
hipError_t launch_build_tri_records(const uint32_t* indices, const float* vertices, uint32_t triangles,
                                    uint32_t vertex_count, void* singles, void* pairs, hipStream_t stream)
{
    if (triangles == 0) return hipSuccess;
    const uint32_t npairs = (uint32_t)((triangles + 1ull) / 2ull);
    hipLaunchKernelGGL(dev::build_tri_records, dim3((npairs + 255u) / 256u), dim3(256), 0, stream, indices, vertices,
                       triangles, vertex_count, static_cast<float4*>(singles), static_cast<float4*>(pairs));
    return hipGetLastError();
}

hipError_t launch_scan_leaf_counts(const void* bvh, uint32_t nodes, uint32_t triangles, uint32_t* flags,
                                   hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess || nodes == 0) return e;
    hipLaunchKernelGGL(dev::scan_leaf_counts, dim3((nodes + 255u) / 256u), dim3(256), 0, stream,
                       static_cast<const wcpt_node*>(bvh), nodes, 3u * triangles, flags);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::scan_tiny_tree, dim3(1), dim3(1), 0, stream, static_cast<const wcpt_node*>(bvh), nodes,
                       3u * triangles, flags);
    return hipGetLastError();
}

hipError_t launch_build_primary_pairs(const void* pairs, uint32_t npairs, float ox, float oy, float oz, void* out,
                                      hipStream_t stream)
{
    if (npairs == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::build_primary_pairs, dim3((npairs + 255u) / 256u), dim3(256), 0, stream,
                       static_cast<const float4*>(pairs), npairs, ox, oy, oz, static_cast<float4*>(out));
    return hipGetLastError();
}

static_assert(dev::kPrimCacheNone == kPrimaryCacheNone && dev::kPrimCacheWrite == kPrimaryCacheWrite &&
                  dev::kPrimCacheRead == kPrimaryCacheRead, "primary-cache modes");
static_assert(dev::kArithExact == WCPT_ARITH_EXACT && dev::kArithFast == WCPT_ARITH_FAST, "arithmetic modes");
static_assert(dev::kSplitWords * 4u == kMkSplitEntryBytes, "split queue entry");
static_assert(dev::kStageWhole == kMkStageWhole && dev::kStageHead == kMkStageHead && dev::kStageTail == kMkStageTail,
              "launch stages");
/* One launch of launch_megakernel: the frame's arguments, the stream (the context's or a pipe's), its share of the
 * cost-ordered tiles (list / grid; null: every tile, in the order below) and, for a split render, the pipe's queue. */
struct MkLaunch {
    const LaunchArgs& a;
    MkState& mk;
    hipStream_t stream;
    uint32_t tilesX, tiles;
    const uint32_t* list;
    uint32_t grid;
    dev::SplitQueue q;
};

/* The tile order of a launch: tile_of_block's `scatter` and `order`, and where the launch records its tiles' times. */
struct MkTiles {
    uint32_t scatter;
    const uint32_t* order;
    uint32_t* cost;
};
static MkTiles mk_tiles(const MkLaunch& l, bool count)
{
    const LaunchArgs& a = l.a;
    MkState& mk = l.mk;
    const uint32_t tiles = l.tiles;
    /* scattered tile order: block b renders tile (b * m) mod tiles for an m coprime with tiles near 0.618 * tiles,
     * so the tiles resident on one CU at once come from all over the frame */
    /* 3, 4, 5, 6: striped XCD bands of 1, 2, 4, 8 tile rows (tile_of_block: even scatter = 2 x stripe height);
     * 2 (auto, default): scattered for a launch of about one round of resident waves (below), else stripes of one tile
     * row. Measured (round 3, 10 frames x 4 interleaved rounds): the reference's Init scene 1.91 ms (bands) -> 1.48 ms
     * (stripes of 1; 2 / 4 / 8 rows: 1.50 / 1.69 / 1.98 ms; scattered 1.52), the atrium on the megakernel 12.15 ->
     * 11.24 ms; the Cornell box 0.379 -> 0.382 ms (its tiles cost alike, so bands only keep neighbours together) */
    uint32_t scatter = a.mk_tile_order >= 3 ? (2u << (a.mk_tile_order - 3)) : (a.mk_tile_order == 2 ? 2u : 0u);
    const bool one_round = (uint64_t)tiles <= 16ull * (uint64_t)mk.cus; /* <= ~4 resident waves per SIMD */
    if ((a.mk_tile_order == 1 || (a.mk_tile_order == 2 && one_round)) && tiles > 2) {
        uint32_t m = (uint32_t)((uint64_t)tiles * 618034u / 1000000u) | 1u;
        auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t r = x % y; x = y; y = r; } return x; };
        while (gcd(m, tiles) != 1u) m += 2u;
        scatter = m;
    }
    /* cost-ordered tiles (auto order, render launches): this render records every tile's time, and the renders after
     * a sort (launch_megakernel) take the tiles longest first */
    const bool cost_order = !count && a.mk_tile_order == 2 && mk.cost != nullptr;
    const uint32_t* order = l.list ? l.list : (cost_order && mk.order_valid ? mk.order : nullptr);
    return {scatter, order, cost_order ? mk.cost : nullptr};
}

template <bool COUNT, bool DIAG, int SK, bool PAIRS, bool SINGLE, bool REUSE, int PC, int A, int STAGE>
static hipError_t launch_mega(const MkLaunch& l)
{
    const LaunchArgs& a = l.a;
    const MkTiles t = mk_tiles(l, COUNT);
    typename dev::StageQueue<STAGE>::type qa; /* only a head has a queue argument */
    if constexpr (STAGE == dev::kStageHead) qa = l.q;
    hipLaunchKernelGGL((dev::pt_megakernel<COUNT, DIAG, SK, PAIRS, SINGLE, REUSE, PC, A, STAGE>),
                       dim3(l.list ? l.grid : l.tiles), dim3(64), 0, l.stream, a.sd, a.materials, a.spheres, a.draws,
                       a.tri_records, a.image, a.wire, a.wire_ch, a.W, a.H, RowMap{a.y0, a.row_shift, a.row_gap},
                       a.wire_rows, a.rows, l.tilesX, l.tiles, t.scatter, t.order, t.cost, a.status,
                       a.counters, PC != kPrimaryCacheNone ? static_cast<uint32_t*>(l.mk.prim_mem) : nullptr, qa);
    return hipGetLastError();
}

/* The walk-only pair of a tiny tree's split render (pt_mk_tiny.hip), in the places of the general head and tail. */
static hipError_t launch_tiny_pair(const MkLaunch& l, int pcmode)
{
    const LaunchArgs& a = l.a;
    const MkTiles t = mk_tiles(l, false);
    TinyHeadLaunch h;
    h.grid = l.list ? l.grid : l.tiles;
    h.tilesX = l.tilesX;
    h.tiles = l.tiles;
    h.scatter = t.scatter;
    h.order = t.order;
    h.cost = t.cost;
    h.prim_cache = pcmode != kPrimaryCacheNone ? static_cast<uint32_t*>(l.mk.prim_mem) : nullptr;
    hipError_t e = launch_tiny_head(a, pcmode, h, l.q, l.stream);
    if (e == hipSuccess) e = launch_tiny_tail(a, l.q, l.stream);
    return e;
}

/* the tail behind its head on the same stream: one wave per 64 entries of the queue's capacity */
template <bool PAIRS, bool SINGLE, int A>
static hipError_t launch_tail(const MkLaunch& l)
{
    const LaunchArgs& a = l.a;
    hipLaunchKernelGGL((dev::pt_mk_tail<PAIRS, SINGLE, A>), dim3((l.q.cap + 63u) / 64u), dim3(64), 0, l.stream, a.sd,
                       a.materials, a.spheres, a.draws, a.tri_records, a.image, a.wire, a.wire_ch, a.W, a.wire_rows,
                       a.status, l.q);
    return hipGetLastError();
}

/* The dispatcher: a runtime MkVariant becomes the kernels' template arguments. Every field combination has a number
 * (mk_variant_code), each number a launch function, and only the combinations mk_variant_built admits have a kernel
 * behind theirs -- so mk_variant.h is the list of the instances this file compiles. */
template <uint32_t CODE>
static hipError_t launch_variant(const MkLaunch& l)
{
    constexpr MkVariant v = mk_variant_decode(CODE);
    if constexpr (!mk_variant_built(v)) return hipErrorInvalidValue;
    else if constexpr (v.stage == kMkStageTail) return launch_tail<v.pairs, v.single, v.arith>(l);
    else return launch_mega<v.count, v.diag, v.stack, v.pairs, v.single, v.reuse, v.pcache, v.arith, v.stage>(l);
}
template <size_t... CODE>
static hipError_t mk_dispatch(const MkVariant& v, const MkLaunch& l, std::index_sequence<CODE...>)
{
    static constexpr hipError_t (*table[])(const MkLaunch&) = {&launch_variant<(uint32_t)CODE>...};
    return mk_variant_built(v) ? table[mk_variant_code(v)](l) : hipErrorInvalidValue;
}
static hipError_t mk_dispatch(const MkVariant& v, const MkLaunch& l)
{
    return mk_dispatch(v, l, std::make_index_sequence<kMkVariantCodes>{});
}

__global__ void fill_iota(uint32_t* __restrict__ v, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i;
}

__global__ void split_tiles(const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ out)
{
    const uint32_t half = (n + 1u) / 2u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[(i & 1u) ? half + (i >> 1) : (i >> 1)] = order[i];
}

/* the caller has synchronised the context's stream after mk_join */
void mk_release(MkState& mk)
{
    for (uint32_t p = 0; p < kMkPipes; p++) {
        if (mk.pipe[p]) (void)hipStreamDestroy(mk.pipe[p]);
        if (mk.join[p]) (void)hipEventDestroy(mk.join[p]);
    }
    if (mk.fork) (void)hipEventDestroy(mk.fork);
    if (mk.mem) (void)hipFree(mk.mem);
    if (mk.prim_mem) (void)hipFree(mk.prim_mem);
    if (mk.split_mem) (void)hipFree(mk.split_mem);
    const int cus = mk.cus;
    mk = MkState{};
    mk.cus = cus;
}

/* Longest-first tile order from the costs the renders record (tile time in shader cycles). Measured (round 3,
 * a per-tile timing build, 20 frames x 4 interleaved rounds): tile times vary with a coefficient of variation of 0.5-0.66
 * across a frame and repeat from frame to frame for a still camera (the same primary rays); starting the longest
 * tiles first leaves the short ones to fill the launch's last round: the Cornell box 0.3863 -> 0.3761 ms, its
 * 270-row block 0.1251 -> 0.1209 ms, the reference's scene 1.486 -> 1.284 ms. Sorted after the first render of a
 * geometry, after its 4th and 16th and then every kResortEvery renders (a radix sort of one key per tile, ~tens of
 * microseconds). */
constexpr uint32_t kResortEvery = 64;

/* Replace one of the launch state's device buffers (the tile costs, the primary cache, the split queues) by a larger
 * one, behind everything that may still read the old one: both pipes joined into the stream -- so the next piped render
 * forks again, behind whatever the caller queues on the stream to initialise the new buffer -- then, when there is an
 * old buffer, the stream synchronised and the buffer freed; then the allocation. The tile-cost buffer used to grow
 * without the join: it is a no-op when no frame is pending on the pipes, and the safe direction otherwise. The caller
 * zeroes its capacity first, so a failure leaves a buffer that the next render grows again. */
static hipError_t mk_grow(MkState& mk, hipStream_t stream, void*& mem, size_t bytes)
{
    hipError_t e = mk_join(mk, stream);
    if (e == hipSuccess && mem) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if (mem) (void)hipFree(mem);
    mem = nullptr;
    return hipMalloc(&mem, bytes);
}

static hipError_t cost_order_prepare(const LaunchArgs& a, MkState& mk, uint32_t tiles, hipStream_t stream)
{
    if (tiles > mk.cap) {
        size_t temp = 0;
        hipError_t e = hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp, (const uint32_t*)nullptr,
                                                                    (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                                                    (uint32_t*)nullptr, (int)tiles, 0, 32, stream);
        if (e != hipSuccess) return e;
        const size_t words = 5ull * tiles;
        const size_t bytes = ((words * 4ull + 255ull) & ~255ull) + temp;
        mk.cap = 0;
        e = mk_grow(mk, stream, mk.mem, bytes);
        if (e != hipSuccess) return e;
        void* const m = mk.mem;
        uint32_t* u = static_cast<uint32_t*>(m);
        mk.cost = u;
        mk.keys = u + tiles;
        mk.iota = u + 2ull * tiles;
        mk.order = u + 3ull * tiles;
        mk.split = u + 4ull * tiles;
        mk.temp = static_cast<char*>(m) + ((words * 4ull + 255ull) & ~255ull);
        mk.temp_bytes = temp;
        mk.cap = tiles;
        mk.geom_tiles = 0; /* forces the reset below */
    }
    if (mk.geom_tiles != tiles || mk.geom_w != a.W || mk.geom_rows != a.rows || mk.geom_y0 != a.y0 ||
        mk.geom_shift != a.row_shift || mk.geom_gap != a.row_gap) {
        mk.geom_tiles = tiles;
        mk.geom_w = a.W;
        mk.geom_rows = a.rows;
        mk.geom_y0 = a.y0;
        mk.geom_shift = a.row_shift;
        mk.geom_gap = a.row_gap;
        mk.renders = 0;
        mk.order_valid = false;
        mk.split_valid = false;
        return hipMemsetAsync(mk.cost, 0, (size_t)tiles * 4u, stream); /* the running averages start at 0 */
    }
    return hipSuccess;
}

static hipError_t cost_order_sort(MkState& mk, uint32_t tiles, hipStream_t stream)
{
    hipLaunchKernelGGL(fill_iota, dim3(std::min<uint32_t>((tiles + 255u) / 256u, 1024u)), dim3(256), 0, stream,
                       mk.iota, tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t temp = mk.temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairsDescending(mk.temp, temp, mk.cost, mk.keys, mk.iota, mk.order, (int)tiles, 0,
                                                     32, stream);
    if (e != hipSuccess) return e;
    mk.order_valid = true;
    /* the frame-overlap pipes' tile lists: the order's even positions, then its odd ones (each list longest first) */
    hipLaunchKernelGGL(split_tiles, dim3(std::min<uint32_t>((tiles + 255u) / 256u, 1024u)), dim3(256), 0, stream,
                       mk.order, tiles, mk.split);
    e = hipGetLastError();
    mk.split_valid = e == hipSuccess;
    return e;
}

hipError_t mk_join(MkState& mk, hipStream_t stream)
{
    if (!mk.pending) return hipSuccess;
    mk.pending = false;
    hipError_t first = hipSuccess;
    for (uint32_t p = 1; p < kMkPipes; p++) { /* pipe 0 is the context's stream itself */
        hipError_t e = hipEventRecord(mk.join[p], mk.pipe[p]);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, mk.join[p], 0);
        if (e != hipSuccess && first == hipSuccess) first = e;
    }
    return first;
}

/* Frame overlap: a launch leaves its last round of waves with fewer and fewer tiles (the cost order puts the shortest
 * last) and the next frame's launch on the same stream cannot start before the last one ends -- the in-order queue
 * sets each dispatch's barrier bit, and gfx9 has no any-order launch (hip_ext.h). Two contexts rendering the Cornell
 * box round-robin finish 5.0 % more frames than one (0.3441 against 0.3614 ms, tools/stream_overlap.py,
 * profiles/r06_stream_overlap.log): that tail, overlapped by the other stream's work. Here one context does it with
 * two pipes: each takes half the cost-ordered tiles (every other position of the order, so both halves cost alike),
 * pipe 0 on the context's stream and pipe 1 on a stream of its own (one stream more per context: a one-rank group's
 * communication stream still fits the device's four hardware queues), and a pipe's next frame queues behind its own
 * previous frame only. A pixel belongs to the
 * same pipe in every frame while the order stands, so its frames accumulate in order; a re-sort, a new geometry,
 * another kernel or any other entry point first joins both pipes into the context's stream (mk_join). Auto: from 1.5
 * rounds of resident waves up (c2 4-way blocks, 2 rounds: 0.1168 -> 0.0916 ms, 2-way 0.1976 -> 0.1759 ms; an 8-way block
 * is one round, and there the overlap measured +0.9 %; profiles/r06_block_overlap.log). */
constexpr uint32_t kMkOverlapMinTilesPerCu = 24;

hipError_t launch_megakernel(const LaunchArgs& a, int mode, int stack_kind, MkState& mk, hipStream_t stream, int overlap)
{
    const uint32_t tilesX = (a.W + dev::kTileW - 1u) / dev::kTileW;
    const uint32_t tilesY = (a.rows + dev::kTileH - 1u) / dev::kTileH;
    const uint32_t tiles = tilesX * tilesY;
    if (mk.cus == 0) { /* CU count of the context's device, cached per context */
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&mk.cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
    }
    const bool cost_order = mode == kModeRender && a.mk_tile_order == 2;
    const bool same_geometry = mk.geom_tiles == tiles && mk.geom_w == a.W && mk.geom_rows == a.rows &&
                               mk.geom_y0 == a.y0 && mk.geom_shift == a.row_shift && mk.geom_gap == a.row_gap;
    const bool pipes = overlap != 0 && cost_order && same_geometry && mk.order_valid && mk.split_valid && tiles >= 2u &&
                       (overlap == 2 || (uint64_t)tiles >= (uint64_t)kMkOverlapMinTilesPerCu * (uint64_t)mk.cus);
    hipError_t e = hipSuccess;
    if (mk.pending && !(pipes && mk.pending_tiles == tiles)) {
        e = mk_join(mk, stream);
        if (e != hipSuccess) return e;
    }
    if (tiles == 0) return hipSuccess;
    if (cost_order) {
        e = cost_order_prepare(a, mk, tiles, stream);
        if (e != hipSuccess) return e;
    }
    /* Primary cache (primary_cache_key.h has the rule). Counting runs leave it as it is. A write needs no join of its
     * own, and neither does the read that follows it: a pixel belongs to the same pipe while the tile order stands, and
     * every re-sort, new geometry or other kernel joins both pipes into the stream first (above and below), so the
     * write of frame n is ordered before the read of frame n + 1 by the rule that orders the image's read-modify-write.
     * The step from unpiped to piped launches keeps it too: the fork event is recorded on the stream behind the
     * unpiped write, and pipe 1 waits for it before its first read. */
    int pcmode = kPrimaryCacheNone;
    if (mode == kModeRender) {
        const PrimaryCacheKey none = {};
        pcmode = primary_cache_decide(a.prim_key != nullptr, a.sd.renderedFramesCount, mk.prim_valid, mk.prim_key,
                                      a.prim_key ? *a.prim_key : none);
        if (pcmode == kPrimaryCacheNone) mk.prim_valid = false;
    }
    if (pcmode == kPrimaryCacheWrite) {
        mk.prim_valid = false;
        const uint64_t bytes = primary_record_bytes(tiles);
        if (bytes > mk.prim_bytes) {
            mk.prim_bytes = 0;
            e = mk_grow(mk, stream, mk.prim_mem, bytes);
            if (e != hipSuccess) return e;
            mk.prim_bytes = bytes;
        }
    }
    /* Split render (mk_split_rule.h has the rule and the queues' layout): head and tail go onto the pipe's stream one
     * after the other, so whatever orders the pipes' frames -- the image's read-modify-write, the primary cache, every
     * join -- orders them as it orders whole launches; a pixel's frames still accumulate in stream order, whichever
     * stage stores it. The tile costs become the head's times (the tail has no tiles). */
    const uint32_t cut = mk_split_cut(a.mk_split, mode == kModeRender && stack_kind == 1, a.sd.samples,
                                      a.sd.maxBounceCount, tiles, 16ull * (uint64_t)mk.cus, a.triangles);
    const MkSplitLayout lay = mk_split_layout(tiles, pipes);
    /* the instance or instances of this render: mk_variant.h has the rule */
    const MkSelection sel = mk_variant_select(mode, stack_kind, a.pair_records, a.sd.drawCommandCount, a.sd.samples, pcmode,
                                              a.arith, cut != 0u);
    const bool split = sel.n == 2u;
    /* a tiny tree's split render runs on the walk-only head and tail (mk_tiny_rule.h has the condition) */
    const bool tiny = mk_tiny_kernels(mode, a.tiny_tree, split, sel.v[0].pairs, sel.v[0].single, sel.v[0].arith);
    if (split && lay.entries > mk.split_entries) { /* first: both counters of each pipe zero */
        mk.split_entries = 0;
        const size_t state_bytes = (size_t)lay.entries * kMkSplitEntryBytes;
        const size_t ctr_bytes = 2u * kMkPipes * kMkSplitCounterWords * sizeof(uint32_t);
        e = mk_grow(mk, stream, mk.split_mem, state_bytes + ctr_bytes);
        if (e != hipSuccess) return e;
        mk.split_ctr = reinterpret_cast<uint32_t*>(static_cast<char*>(mk.split_mem) + state_bytes);
        mk.split_parity[0] = mk.split_parity[1] = 0u;
        e = hipMemsetAsync(mk.split_ctr, 0, ctr_bytes, stream);
        if (e != hipSuccess) return e;
        mk.split_entries = lay.entries;
    }
    auto launch = [&](const LaunchArgs& la, hipStream_t s, const uint32_t* list, uint32_t grid, uint32_t p) {
        MkLaunch l = {la, mk, s, tilesX, tiles, list, grid, dev::SplitQueue{}};
        if (split) { /* pipe p's queue and this frame's counter; the pipe's next frame takes the other */
            l.q.state = static_cast<uint32_t*>(mk.split_mem) + (size_t)dev::kSplitWords * lay.first[p];
            l.q.count = mk.split_ctr + (size_t)(2u * p + mk.split_parity[p]) * kMkSplitCounterWords;
            l.q.count_next = mk.split_ctr + (size_t)(2u * p + (mk.split_parity[p] ^ 1u)) * kMkSplitCounterWords;
            l.q.cap = lay.cap[p];
            l.q.cut = cut;
        }
        hipError_t le = hipSuccess; /* the whole kernel, or the head and then its tail */
        if (tiny) le = launch_tiny_pair(l, sel.v[0].pcache);
        for (uint32_t i = 0; i < sel.n && !tiny && le == hipSuccess; i++) le = mk_dispatch(sel.v[i], l);
        if (le == hipSuccess && split) mk.split_parity[p] ^= 1u;
        return le;
    };
    if (pipes) {
        if (!mk.pending) { /* fork: pipe 1 after everything queued on the context's stream */
            for (uint32_t p = 1; p < kMkPipes && e == hipSuccess; p++) {
                if (!mk.pipe[p]) e = hipStreamCreateWithFlags(&mk.pipe[p], hipStreamNonBlocking);
                if (e == hipSuccess && !mk.join[p]) e = hipEventCreateWithFlags(&mk.join[p], hipEventDisableTiming);
            }
            if (e == hipSuccess && !mk.fork) e = hipEventCreateWithFlags(&mk.fork, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(mk.fork, stream);
            for (uint32_t p = 1; p < kMkPipes && e == hipSuccess; p++) e = hipStreamWaitEvent(mk.pipe[p], mk.fork, 0);
            if (e != hipSuccess) return e;
        }
        const uint32_t half = (tiles + 1u) / 2u;
        e = launch(a, stream, mk.split, half, 0u);
        /* pending from the first enqueue on: a failed second launch still leaves the first to join */
        mk.pending = true;
        mk.pending_tiles = tiles;
        if (e == hipSuccess && a.pipe1_prepare) e = a.pipe1_prepare(a.pipe1_user, mk.pipe[1]);
        if (e == hipSuccess) {
            LaunchArgs a1 = a;
            if (a.tri_records_pipe1) a1.tri_records = a.tri_records_pipe1;
            e = launch(a1, mk.pipe[1], mk.split + half, tiles - half, 1u);
        }
    } else {
        e = launch(a, stream, nullptr, 0, 0u);
    }
    if (e == hipSuccess && split) mk.split_renders++;
    if (e == hipSuccess && tiny) mk.tiny_renders++;
    if (e == hipSuccess && pcmode == kPrimaryCacheWrite) {
        mk.prim_key = *a.prim_key;
        mk.prim_valid = true;
        mk.prim_writes++;
    } else if (e == hipSuccess && pcmode == kPrimaryCacheRead) {
        mk.prim_reads++;
    }
    if (e != hipSuccess || !cost_order) return e;
    /* sorted after renders 1, 4 and 16 of a geometry (the running averages settle), then every kResortEvery; the sort
     * rewrites the order the pipes read, so they are joined first and the next render forks after it */
    const uint32_t r = ++mk.renders;
    if (r == 1u || r == 4u || r == 16u || r % kResortEvery == 0u) {
        e = mk_join(mk, stream);
        if (e != hipSuccess) return e;
        return cost_order_sort(mk, tiles, stream);
    }
    return hipSuccess;
}

} // namespace wcpt
