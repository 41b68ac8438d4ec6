/*
 * pt_primary.hip — the primary-hit pass for gfx950 (wcpt_trace_primary, wcpt_pick): segment 0 of every pixel of a window,
 * stopped after Intersect (pathTracer.comp:135-211) and written out as a wcpt_primary_hit record (primary_hit.h) with the
 * identity of the primitive that won.
 *
 * Launch shape: the megakernel's -- one 64-lane wave per 8x8 pixel tile of the window, so a wave's rays are coherent and
 * the frame's row map (row_map.h) is the render's. The window is `width` x `rows` pixels whose first column is frame
 * column x0 and whose local row ly is frame row frame_row(rm, ly): the context's rows for the whole pass, one pixel for
 * the pick -- one kernel for both. A lane outside the window or the frame traverses nothing and stores nothing.
 *
 * The closest hit is pt_traversal.h closest_hit (the sphere loop and the multi-draw traversal loop of intersect on the LDS
 * stack with its spill), resolved by resolve_hit<kArithExact>: always exact arithmetic. One instance, on the general
 * multi-draw loop, which also serves one draw and none; its leaves read the record layout the frame's plan chose for the
 * renders (pair records for fat leaves, single records for thin ones: frame_prep.h frame_plan) through a kernel-uniform
 * switch -- every draw's table entry holds both. Each lane stores its record as three 16-byte vector stores; the eight
 * lanes of a tile row write 384 contiguous bytes.
 */
#include <hip/hip_runtime.h>

#include "primary_hit.h"
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_mk_tile.h"

namespace wcpt {
namespace dev {

__global__ __launch_bounds__(64) void pt_primary(const wcpt_scene_data sd, const wcpt_sphere* __restrict__ spheres,
                                                 const wcpt_draw_command* __restrict__ draws,
                                                 const uint64_t* __restrict__ tri_records, uint4* __restrict__ dst,
                                                 uint32_t W, uint32_t H, uint32_t x0, uint32_t width, uint32_t rows,
                                                 const RowMap rm, uint32_t tilesX, uint32_t tilesTotal,
                                                 uint32_t pairs, uint32_t* __restrict__ status)
{
    uint32_t tx, ty;
    tile_of_block(tilesX, tilesTotal, 0u, nullptr, tx, ty);
    const uint32_t lx = tx * kTileW + (threadIdx.x % kTileW);
    const uint32_t ly = ty * kTileH + (threadIdx.x / kTileW);
    bool overflow = false;
    if (lx < width && ly < rows) {
        const uint32_t x = x0 + lx, y = frame_row(rm, ly);
        if (x < W && y < H) {
            __shared__ uint64_t s_stack[kLdsStack * 64];
            uint64_t spill[kSpillStack];
            LdsStack<kLdsStack, kSpillStack> stk;
            stk.base = (lds_u64_ptr)(s_stack + (threadIdx.x & 63u));
            stk.spill = (priv_u64_ptr)spill;
            stk.reset();
            Ray r;
            r.origin = mk3(sd.position[0], sd.position[1], sd.position[2]);
            r.direction = primary_direction(sd, x, y, W, H);
            r.invDirection = rcp3(r.direction);
            const ClosestHit c = closest_hit(r, sd, spheres, draws, tri_records, stk, overflow, true, pairs != 0u);
            const Hit h = resolve_hit<kArithExact>(r, c.t, c.prim, c.draw, spheres, draws, tri_records);
            const uint32_t dir[3] = {__float_as_uint(r.direction.x), __float_as_uint(r.direction.y),
                                     __float_as_uint(r.direction.z)};
            const uint32_t nrm[3] = {__float_as_uint(h.normal.x), __float_as_uint(h.normal.y), __float_as_uint(h.normal.z)};
            uint32_t w[kPrimHitWords];
            primary_hit_pack(primary_hit_of(dir, __float_as_uint(h.t), nrm, h.front, h.material, c.prim, c.draw), w);
            uint4* const p = dst + (size_t)(primary_hit_offset(ly, lx, width) / sizeof(uint4));
            p[0] = make_uint4(w[0], w[1], w[2], w[3]);
            p[1] = make_uint4(w[4], w[5], w[6], w[7]);
            p[2] = make_uint4(w[8], w[9], w[10], w[11]);
        }
    }
    if (overflow) atomicOr(status, 1u);
}

} // namespace dev

static_assert(kPrimHitNoPrim == dev::kNoPrim && kPrimHitSpherePrim == dev::kSpherePrim, "primary_hit.h: the traversal's primitive");
static_assert(kPrimHitBytes == sizeof(wcpt_primary_hit) && kPrimHitBytes % sizeof(uint4) == 0, "primary_hit.h: the record");
static_assert(kPrimHitMiss == WCPT_HIT_MISS && kPrimHitSphere == WCPT_HIT_SPHERE && kPrimHitTriangle == WCPT_HIT_TRIANGLE,
              "primary_hit.h: the kinds");

hipError_t launch_primary(const PrimaryPass& p, hipStream_t stream)
{
    const uint64_t tilesX = ((uint64_t)p.width + dev::kTileW - 1u) / dev::kTileW;
    const uint64_t tilesY = ((uint64_t)p.rows + dev::kTileH - 1u) / dev::kTileH;
    const uint64_t tiles = tilesX * tilesY;
    if (tiles == 0) return hipSuccess;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue; /* the runtime admits a renderable frame only (screen_layout.h) */
    hipLaunchKernelGGL(dev::pt_primary, dim3((uint32_t)tiles), dim3(64), 0, stream, p.sd, p.spheres, p.draws, p.tri_records,
                       static_cast<uint4*>(p.dst), p.W, p.H, p.x0, p.width, p.rows, p.rm, (uint32_t)tilesX, (uint32_t)tiles,
                       p.pair_records ? 1u : 0u, p.status);
    return hipGetLastError();
}

} // namespace wcpt
