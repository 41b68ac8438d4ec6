/*
 * pt_bvh_build.hip — wcpt_bvh_build_device: the midpoint BVH of wcpt_bvh_build built on the device, level by level.
 *
 * What is computed is stated in bvh_midpoint.h (bvh_step_*: one call per triangle position and step, the same
 * functions tests/bvh_levels_shim.cpp runs as host loops); this file is how the steps are spread over the machine.
 * Every step is one launch of one thread per position over the whole triangle array, whatever the level: a position
 * finds its node through owner[], so 140,000 two-triangle segments cost what one segment of 262,144 costs, and no
 * thread ever loops over a segment. A step reads what the step before wrote; stream order is the only synchronisation
 * between workgroups, and there is no device-side recursion or launch.
 *
 * Per level (at most 32): classify -> prefix sum of the left flags (2048-element blocks by wave shuffles and LDS, then,
 * for more than one block, a launch over the block totals) -> rank tables -> scatter of the permutation (and the
 * children's allocation by each splitting node's first position) -> descend (owner[] moves to the child; the child's bounds as 64-bit integer
 * minima, reduced over each run of equal nodes inside a wave by shuffles first, so a large node costs six atomics per
 * wave and a node smaller than a wave six in all) -> finalize (the bounds' bits read back from the winning positions).
 * The host reads the level's split count (16 bytes) and stops at the first level that splits nothing.
 * Then: prefix sum of the interior starts, emit (each temporary node to its preorder place), index permutation.
 *
 * Bounds of what is read: the index check runs alone first and reads only the index buffer; no vertex is gathered
 * unless every index is below vertex_count. All other addresses are positions < ntri or temporary nodes < 2 ntri.
 */
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "pt_kernels.h"
#include "bvh_midpoint.h"

namespace wcpt {
namespace dev {

constexpr uint32_t kBvhBlock = 256u;
constexpr uint32_t kBvhNoNode = 0xFFFFFFFFu;

enum BvhStep { kStepCheckIndex, kStepPrepare, kStepFinalize, kStepClassify, kStepRank, kStepScatter, kStepEmit, kStepPermute };

template <int STEP>
__global__ __launch_bounds__(kBvhBlock) void bvh_step_kernel(const BvhBuild b, uint32_t n, uint32_t level)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kBvhBlock + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    if (STEP == kStepCheckIndex) bvh_step_check_index(b, i);
    if (STEP == kStepPrepare) bvh_step_prepare(b, i);
    if (STEP == kStepFinalize) bvh_step_finalize(b, i, level);
    if (STEP == kStepClassify) bvh_step_classify(b, i, level);
    if (STEP == kStepRank) bvh_step_rank(b, i, level);
    if (STEP == kStepScatter) bvh_step_scatter(b, i, level);
    if (STEP == kStepEmit) bvh_step_emit(b, i);
    if (STEP == kStepPermute) bvh_step_permute(b, i);
}

/* bvh_step_descend (ROOT: bvh_step_accumulate into the root), with the keys of each run of lanes that fall into one
 * node combined by shuffles before the run's first lane issues the atomics. The keys' minimum / maximum are integer
 * and commutative, so the grouping does not show in the result. Every lane of a wave reaches every shuffle. */
template <bool ROOT>
__global__ __launch_bounds__(kBvhBlock) void bvh_descend_kernel(const BvhBuild b, uint32_t level)
{
    const uint64_t p64 = (uint64_t)blockIdx.x * kBvhBlock + threadIdx.x;
    const uint32_t p = (uint32_t)p64;
    uint32_t node = kBvhNoNode;
    if (p64 < b.ntri) {
        if (ROOT) {
            node = 0u;
        } else {
            const uint32_t child = bvh_child_of(b, p, level);
            if (child != 0u) {
                b.owner[p] = child;
                node = child;
            }
        }
    }
    unsigned long long keys[6];
    for (int c = 0; c < 3; c++) {
        keys[c] = kBvhMinKeyInit;
        keys[3 + c] = kBvhMaxKeyInit;
    }
    if (node != kBvhNoNode) bvh_bounds_keys(b, p, keys);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        /* lanes of one node are contiguous: equal nodes at distance d mean one run, whose far part lane + d has */
        const bool same = __shfl_down(node, d) == node && lane + d < 64u;
        for (int c = 0; c < 3; c++) {
            const unsigned long long lo = __shfl_down(keys[c], d), hi = __shfl_down(keys[3 + c], d);
            if (same && lo < keys[c]) keys[c] = lo;
            if (same && hi > keys[3 + c]) keys[3 + c] = hi;
        }
    }
    const bool head = __shfl_up(node, 1u) != node || lane == 0u;
    if (head && node != kBvhNoNode) bvh_keys_into(b.tn[node], keys);
}

/* the block's exclusive prefix sum of one value per thread; total: the block's sum (all threads) */
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t& total)
{
    __shared__ uint32_t wave_sum[kBvhBlock / 64u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    __syncthreads(); /* wave_sum of an earlier call has been read */
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
    for (uint32_t w = 0; w < kBvhBlock / 64u; w++) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    return before + incl - v;
}

/* scan[i] = the exclusive prefix sum of in[] within i's block of 1 << kBvhScanShift elements; off[block] = its sum, for
 * bvh_scan_offsets_kernel -- or, when one block is the whole array, its offset 0 at once */
__global__ __launch_bounds__(kBvhBlock) void bvh_scan_blocks_kernel(const uint32_t* __restrict__ in, uint32_t n,
                                                                    uint32_t* __restrict__ scan, uint32_t* __restrict__ off)
{
    constexpr uint32_t kPer = (1u << kBvhScanShift) / kBvhBlock;
    const uint64_t base = ((uint64_t)blockIdx.x << kBvhScanShift) + (uint64_t)threadIdx.x * kPer;
    uint32_t v[kPer], sum = 0u;
    for (uint32_t k = 0; k < kPer; k++) {
        v[k] = base + k < n ? in[base + k] : 0u;
        sum += v[k];
    }
    uint32_t total;
    uint32_t at = block_exclusive_scan(sum, total);
    for (uint32_t k = 0; k < kPer; k++) {
        if (base + k < n) scan[base + k] = at;
        at += v[k];
    }
    if (threadIdx.x == 0u) off[blockIdx.x] = gridDim.x == 1u ? 0u : total;
}

/* off[0..nb) into its exclusive prefix sum, by one block */
__global__ __launch_bounds__(kBvhBlock) void bvh_scan_offsets_kernel(uint32_t* off, uint32_t nb)
{
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < nb; base += kBvhBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? off[i] : 0u;
        uint32_t total;
        const uint32_t at = block_exclusive_scan(v, total);
        if (i < nb) off[i] = carry + at;
        carry += total;
    }
}

} // namespace dev

namespace {

uint64_t align256(uint64_t x) { return (x + 255u) & ~255ull; }

uint32_t scan_blocks(uint32_t ntri) { return (uint32_t)(((uint64_t)ntri + 1u + (1u << kBvhScanShift) - 1u) >> kBvhScanShift); }

/* the scratch arrays of a build of ntri triangles, carved from `base` (null: sizes only); returns the bytes */
uint64_t bvh_carve(char* base, uint32_t ntri, BvhBuild& b)
{
    uint64_t at = 0;
    auto take = [&](auto*& p, uint64_t count) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at = align256(at + count * sizeof(T));
    };
    const uint64_t T = ntri;
    take(b.ctrl, kBvhCtrlWords);
    take(b.cen, 3 * T);
    take(b.tmin, 3 * T);
    take(b.tmax, 3 * T);
    take(b.perm, T);
    take(b.perm_next, T);
    take(b.owner, T);
    take(b.flag, T + 1);
    take(b.scan, T + 1);
    take(b.scan_off, scan_blocks(ntri));
    take(b.tab, T);
    take(b.starts, T + 1);
    take(b.lvl0, T);
    take(b.tn, 2 * T);
    take(b.idx_tmp, 3 * T);
    return at;
}

template <int STEP>
hipError_t launch_step(const BvhBuild& b, uint32_t n, uint32_t level, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)n + dev::kBvhBlock - 1u) / dev::kBvhBlock);
    hipLaunchKernelGGL(dev::bvh_step_kernel<STEP>, dim3(grid), dim3(dev::kBvhBlock), 0, stream, b, n, level);
    return hipGetLastError();
}

/* the prefix sums of in[0 .. ntri] into b.scan / b.scan_off (bvh_scan_at) */
hipError_t launch_scan(const BvhBuild& b, const uint32_t* in, hipStream_t stream)
{
    return bvh_launch_scan(in, b.ntri + 1u, b.scan, b.scan_off, stream);
}

hipError_t read_ctrl(const BvhBuild& b, uint32_t ctrl[kBvhCtrlWords], hipStream_t stream)
{
    const hipError_t e = hipMemcpyAsync(ctrl, b.ctrl, sizeof(uint32_t) * kBvhCtrlWords, hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

} // namespace

hipError_t bvh_launch_scan(const uint32_t* in, uint32_t n, uint32_t* scan, uint32_t* off, hipStream_t stream)
{
    const uint32_t nb = (uint32_t)(((uint64_t)n + (1u << kBvhScanShift) - 1u) >> kBvhScanShift);
    hipLaunchKernelGGL(dev::bvh_scan_blocks_kernel, dim3(nb), dim3(dev::kBvhBlock), 0, stream, in, n, scan, off);
    if (nb > 1u) hipLaunchKernelGGL(dev::bvh_scan_offsets_kernel, dim3(1), dim3(dev::kBvhBlock), 0, stream, off, nb);
    return hipGetLastError();
}

uint64_t bvh_build_scratch_bytes(uint32_t index_count)
{
    BvhBuild b{};
    return bvh_carve(nullptr, index_count / 3u, b);
}

#define BVH_TRY(expr)                    \
    do {                                 \
        const hipError_t _e = (expr);    \
        if (_e != hipSuccess) return _e; \
    } while (0)

hipError_t bvh_build_device(const float* vertices, uint32_t vertex_count, uint32_t* indices, uint32_t index_count,
                            void* nodes, void* scratch, uint32_t* status, uint32_t* nodes_used, hipStream_t stream)
{
    BvhBuild b{};
    b.vertices = vertices;
    b.vertex_count = vertex_count;
    b.indices = indices;
    b.ntri = index_count / 3u;
    b.out = static_cast<wcpt_node*>(nodes);
    bvh_carve(static_cast<char*>(scratch), b.ntri, b);
    const uint32_t T = b.ntri;
    const uint32_t grid = (T + dev::kBvhBlock - 1u) / dev::kBvhBlock;
    uint32_t ctrl[kBvhCtrlWords] = {0u, 0u, 0u, 0u};
    *status = 0u;

    /* nothing but the index buffer is read until every index has passed, and nothing of the caller's is written
     * until every referenced coordinate has */
    BVH_TRY(hipMemsetAsync(b.ctrl, 0, sizeof(uint32_t) * kBvhCtrlWords, stream));
    BVH_TRY(launch_step<dev::kStepCheckIndex>(b, index_count, 0u, stream));
    BVH_TRY(read_ctrl(b, ctrl, stream));
    if (ctrl[kBvhCtrlStatus]) {
        *status = ctrl[kBvhCtrlStatus];
        return hipSuccess;
    }
    BVH_TRY(launch_step<dev::kStepPrepare>(b, T, 0u, stream));
    BVH_TRY(read_ctrl(b, ctrl, stream));
    if (ctrl[kBvhCtrlStatus]) {
        *status = ctrl[kBvhCtrlStatus];
        return hipSuccess;
    }
    hipLaunchKernelGGL(dev::bvh_descend_kernel<true>, dim3(grid), dim3(dev::kBvhBlock), 0, stream, b, 0u);
    BVH_TRY(hipGetLastError());
    BVH_TRY(launch_step<dev::kStepFinalize>(b, T, 0u, stream));
    for (uint32_t level = 0u; level < kBvhRootBudget; level++) {
        BVH_TRY(launch_step<dev::kStepClassify>(b, T, level, stream));
        BVH_TRY(launch_scan(b, b.flag, stream));
        BVH_TRY(launch_step<dev::kStepRank>(b, T, level, stream));
        BVH_TRY(launch_step<dev::kStepScatter>(b, T, level, stream));
        std::swap(b.perm, b.perm_next);
        hipLaunchKernelGGL(dev::bvh_descend_kernel<false>, dim3(grid), dim3(dev::kBvhBlock), 0, stream, b, level);
        BVH_TRY(hipGetLastError());
        BVH_TRY(launch_step<dev::kStepFinalize>(b, T, level + 1u, stream));
        BVH_TRY(read_ctrl(b, ctrl, stream));
        if (ctrl[kBvhCtrlSplits] == 0u) break;
    }
    const uint32_t used = ctrl[kBvhCtrlNodes];
    if (used == 0u || used > 2ull * T) return hipErrorUnknown; /* every node holds a triangle: at most 2 T - 1 */
    BVH_TRY(launch_scan(b, b.starts, stream));
    BVH_TRY(launch_step<dev::kStepEmit>(b, used, 0u, stream));
    BVH_TRY(launch_step<dev::kStepPermute>(b, T, 0u, stream));
    BVH_TRY(hipMemcpyAsync(indices, b.idx_tmp, sizeof(uint32_t) * 3ull * T, hipMemcpyDeviceToDevice, stream));
    BVH_TRY(hipStreamSynchronize(stream));
    *nodes_used = used;
    return hipSuccess;
}

#undef BVH_TRY

} // namespace wcpt
