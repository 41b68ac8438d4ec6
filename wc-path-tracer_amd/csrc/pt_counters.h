/* pt_counters.h -- what the kernels count and time beside the image: the per-lane work counters and their flush, the
 * reference's stack depth (RefStack), the megakernel's phase timers and the cost-attribution switches (WCPT_DUP_*).
 * Part of pt_device.h. */
#ifndef WCPT_PT_COUNTERS_H
#define WCPT_PT_COUNTERS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wcpt::dev {

/* Megakernel phase timers (tools only: a library built with -DWCPT_MK_TIMERS=1, tools/mk_phases.py). Each wave
 * attributes the s_memtime ticks since its previous mark to the phase that just ended: 0 primary ray, 1 sphere
 * loop, 2 BVH interior steps + pops, 3 leaf triangle tests, 4 hit resolution, 5 shading, 6 accumulation/store.
 * Ticks include the time other waves of the SIMD issue in between: read the shares, not absolute costs. */
#ifndef WCPT_MK_TIMERS
#define WCPT_MK_TIMERS 0
#endif
constexpr int kPhaseTimers = 8;

/* Cost attribution (tools only, tools/ab_build.sh): WCPT_DUP_<part>=1 evaluates that part a second time on
 * laundered inputs and discards the result, so the A/B time difference is the part's cost. Never on by default. */
#ifndef WCPT_DUP_SPHERES
#define WCPT_DUP_SPHERES 0
#endif
#ifndef WCPT_DUP_RANDDIR
#define WCPT_DUP_RANDDIR 0
#endif
#ifndef WCPT_DUP_PAIR
#define WCPT_DUP_PAIR 0
#endif
#ifndef WCPT_DUP_BOX
#define WCPT_DUP_BOX 0
#endif
__device__ __forceinline__ float launder(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ uint32_t launder_u(uint32_t x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ void sink(float x) { asm volatile("" ::"v"(x)); }
__device__ __forceinline__ void sink_u(uint32_t x) { asm volatile("" ::"v"(x)); }

/* Per-lane work counters; reduced per wave and added to global u64 counters. */
struct Counters {
    uint32_t pixels, segments, sphere_tests, node_pops, interior_visits, triangle_tests, hits, draw_fetches;
    uint32_t wave_int, lane_int, wave_tri, lane_tri, wave_seg, lane_seg; /* SIMD-efficiency diagnostics */
    uint32_t ref_over;  /* segments whose reference stack (uint nodeStack[32], :151) is written past index 31 */
    uint32_t ref_max;   /* deepest reference stack (entries after a push), 0xFFFFFFFF when it could not be tracked */
    bool ref_seg;       /* the current segment overflowed the reference stack */
#if WCPT_MK_TIMERS
    uint64_t tim[kPhaseTimers], tprev;
#endif
};

/* The reference's traversal stack, tracked exactly in the counting builds.
 * pathTracer.comp pushes the root (:155) and, at every interior node that survives its box test, BOTH children
 * (:192-198), culling a child only when it is popped (:162). So while a node is visited, its stack index (the entries
 * below it) is the number of its ancestors whose second-popped child is still pending -- the ancestors where the walk
 * went into the first-popped ("near") child. The kernels push only far children that pass their box test, so this
 * index is kept as two path masks instead of a second stack: bit k of `near` = the ancestor at depth k was left
 * through its near child (its far child is still pending in the reference), bit k of `pushed` = that far child is on
 * this kernel's stack. An interior visit pushes at indices rs and rs + 1 with rs = popcount(near); rs >= 31 writes
 * nodeStack[32], out of bounds (undefined behaviour in the reference). A pop of this kernel's stack takes the far
 * child of the deepest `pushed` ancestor k; the reference pops (and culls) every pending entry above it first. */
struct RefStack {
    uint64_t nearm, pushed;
    uint32_t depth;
};
constexpr uint32_t kRefStackSize = 32u;  /* uint nodeStack[32] (pathTracer.comp:151) */
constexpr uint32_t kRefUnknown = 0xFFFFFFFFu;
template <bool COUNT>
__device__ __forceinline__ void ref_root(RefStack& r, Counters& cnt)
{
    if (!COUNT) return;
    r.nearm = 0;
    r.pushed = 0;
    r.depth = 0;
    if (cnt.ref_max < 1u) cnt.ref_max = 1u; /* the root push (:155) */
}
template <bool COUNT>
__device__ __forceinline__ void ref_interior(RefStack& r, bool pushed_far, Counters& cnt)
{
    if (!COUNT) return;
    const uint32_t rs = (uint32_t)__popcll(r.nearm);
    if (rs + 2u > kRefStackSize) cnt.ref_seg = true;
    if (r.depth < 64u) {
        if (cnt.ref_max != kRefUnknown && cnt.ref_max < rs + 2u) cnt.ref_max = rs + 2u;
        const uint64_t b = 1ull << r.depth;
        r.nearm |= b;
        if (pushed_far) r.pushed |= b;
    } else {
        cnt.ref_max = kRefUnknown; /* deeper than the masks: not tracked */
    }
    r.depth++;
}
template <bool COUNT>
__device__ __forceinline__ void ref_pop(RefStack& r)
{
    if (!COUNT || r.pushed == 0) return;
    const uint32_t k = 63u - (uint32_t)__clzll((long long)r.pushed);
    const uint64_t below = (1ull << k) - 1ull;
    r.nearm &= below;
    r.pushed &= below;
    r.depth = k + 1u;
}
template <bool COUNT>
__device__ __forceinline__ void ref_segment_end(Counters& cnt)
{
    if (!COUNT) return;
    if (cnt.ref_seg) cnt.ref_over++;
    cnt.ref_seg = false;
}

__device__ __forceinline__ void phase_start(Counters& c)
{
#if WCPT_MK_TIMERS
    for (int k = 0; k < kPhaseTimers; k++) c.tim[k] = 0;
    c.tprev = __builtin_amdgcn_s_memtime();
#else
    (void)c;
#endif
}
__device__ __forceinline__ void phase_mark(Counters& c, int k)
{
#if WCPT_MK_TIMERS
    const uint64_t t = __builtin_amdgcn_s_memtime();
    c.tim[k] += t - c.tprev;
    c.tprev = t;
#else
    (void)c;
    (void)k;
#endif
}

/* Diagnostic step counting (COUNT kernels only): every executing lane adds a lane-step, the lowest active
 * lane adds the wave-step. */
template <bool DIAG>
__device__ __forceinline__ void simd_step(uint32_t& wave, uint32_t& lane_steps)
{
    if (!DIAG) return;
    const unsigned long long m = __ballot(1);
    lane_steps++;
    if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) wave++;
}

template <bool COUNT, bool DIAG>
__device__ __forceinline__ void count_tri(Counters& cnt)
{
    if (COUNT) {
        cnt.triangle_tests++;
        simd_step<DIAG>(cnt.wave_tri, cnt.lane_tri);
    }
}

/* Wave-level sum of a per-lane u32 counter, one u64 atomic per wave. */
__device__ __forceinline__ void wave_add_u64(unsigned long long* dst, uint32_t v)
{
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(dst, s);
}

/* Wave-reduce the per-lane counters into the 16 global u64 counters (wcpt_counters order; the last is a maximum).
 * All 64 lanes of the wave must call it. */
template <bool COUNT>
__device__ __forceinline__ void flush_counters(const Counters& cnt, unsigned long long* __restrict__ counters)
{
    if (COUNT) {
        wave_add_u64(&counters[0], cnt.pixels);
        wave_add_u64(&counters[1], cnt.segments);
        wave_add_u64(&counters[2], cnt.sphere_tests);
        wave_add_u64(&counters[3], cnt.node_pops);
        wave_add_u64(&counters[4], cnt.interior_visits);
        wave_add_u64(&counters[5], cnt.triangle_tests);
        wave_add_u64(&counters[6], cnt.hits);
        wave_add_u64(&counters[7], cnt.draw_fetches);
        wave_add_u64(&counters[8], cnt.wave_int);
        wave_add_u64(&counters[9], cnt.lane_int);
        wave_add_u64(&counters[10], cnt.wave_tri);
        wave_add_u64(&counters[11], cnt.lane_tri);
        wave_add_u64(&counters[12], cnt.wave_seg);
        wave_add_u64(&counters[13], cnt.lane_seg);
        wave_add_u64(&counters[14], cnt.ref_over);
        uint32_t m = cnt.ref_max;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&counters[15], (unsigned long long)m);
    }
}

} // namespace wcpt::dev

#endif /* WCPT_PT_COUNTERS_H */
