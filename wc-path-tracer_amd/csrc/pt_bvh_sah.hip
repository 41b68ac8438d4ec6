/*
 * pt_bvh_sah.hip — wcpt_bvh_build_sah_device: the binned-SAH BVH of wcpt_bvh_build_sah built on the device, level by level.
 *
 * What is computed is stated in bvh_sah.h (sah_step_*: one call per triangle position, bin or open node and step, the
 * same functions tests/bvh_sah_levels_shim.cpp runs as host loops); this file is how the steps are spread over the
 * machine, in the shape of pt_bvh_build.hip: every step is one launch over the whole triangle array, a position finds its
 * node through owner[], stream order is the only synchronisation, and there is no device-side launch.
 *
 * Before the levels: the index check (reads only indices), prepare (triangle boxes, centroids, finiteness), the root's
 * boxes. Per level (at most 41): finalize (the bounds' bits read back from the winning positions) -> empty bins for the
 * level's open nodes -> bin (each position adds its triangle box and a count to its node's 3 x 16 bins: global atomics,
 * but a span of 1024 positions inside one node bins in LDS first, sah_bin_kernel) -> evaluate (one thread per open
 * node: the two sweeps in binary64, the decision, the scale refusals) -> classify -> prefix sum of the left flags (bvh_launch_scan, pt_bvh_build.hip) -> scatter of the
 * permutation (and the children's allocation by each splitting node's first position) -> descend (owner[] moves to the
 * child; the child's box as 64-bit key atomics and its centroid box as 32-bit ordered atomics, reduced over each run of
 * equal nodes inside a wave by shuffles first). The host reads the control words (16 bytes): a status refuses the build,
 * no split ends it, and the open-node count sizes the next level's bins.
 * Then: prefix sum of the interior starts, a scratch copy of the indices, emit, index permutation -- the only two
 * launches that write the caller's buffers.
 *
 * Bounds of what is read: no vertex is gathered unless every index is below vertex_count. All other addresses are
 * positions < ntri, temporary nodes < 2 ntri, open nodes below the count the bins were sized for, bins 0..15 (clamped).
 */
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "pt_kernels.h"
#include "bvh_sah.h"

namespace wcpt {
namespace dev {

constexpr uint32_t kSahBlock = 256u;
constexpr uint32_t kSahNoNode = 0xFFFFFFFFu;

enum SahStep { kSahCheckIndex, kSahPrepare, kSahFinalize, kSahBinInit, kSahEvaluate, kSahClassify, kSahScatter, kSahEmit, kSahPermute };

template <int STEP>
__global__ __launch_bounds__(kSahBlock) void sah_step_kernel(const SahBuild b, uint32_t n, uint32_t level)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kSahBlock + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    if (STEP == kSahCheckIndex) sah_step_check_index(b, i);
    if (STEP == kSahPrepare) sah_step_prepare(b, i);
    if (STEP == kSahFinalize) sah_step_finalize(b, i, level);
    if (STEP == kSahBinInit) sah_step_bin_init(b, i);
    if (STEP == kSahEvaluate) sah_step_evaluate(b, i);
    if (STEP == kSahClassify) sah_step_classify(b, i, level);
    if (STEP == kSahScatter) sah_step_scatter(b, i, level);
    if (STEP == kSahEmit) sah_step_emit(b, i);
    if (STEP == kSahPermute) sah_step_permute(b, i);
}

/* sah_step_bin over spans of kSahBinSpan positions, one block each. A span that lies in one open node altogether
 * (sah_span_private) collects its triangles in bins in LDS and adds them to the node's with one atomic per non-empty
 * bin word; every other span bins each position straight into its node's bins. At the atrium's root that is 257 x 336
 * global atomics on the node's 336 words instead of 262,288 x 21. */
__global__ __launch_bounds__(kSahBlock) void sah_bin_kernel(const SahBuild b, uint32_t level)
{
    __shared__ SahBin priv[kSahBinsPerNode];
    const uint64_t first = (uint64_t)blockIdx.x * kSahBinSpan; /* < ntri: the grid covers ntri */
    const uint64_t end = first + kSahBinSpan < b.ntri ? first + kSahBinSpan : b.ntri;
    const bool is_private = sah_span_private(b, (uint32_t)first, (uint32_t)(end - 1u), level); /* one value per block */
    if (!is_private) {
        for (uint64_t p = first + threadIdx.x; p < end; p += kSahBlock) sah_step_bin(b, (uint32_t)p, level);
        return;
    }
    if (threadIdx.x < kSahBinsPerNode) sah_bin_reset(priv[threadIdx.x]);
    __syncthreads();
    const SahTempNode& n = b.tn[b.owner[first]];
    for (uint64_t p = first + threadIdx.x; p < end; p += kSahBlock) sah_bin_into(b, n, (uint32_t)p, priv);
    __syncthreads();
    if (threadIdx.x < kSahBinsPerNode) sah_bin_merge(b.bins[(uint64_t)n.open * kSahBinsPerNode + threadIdx.x], priv[threadIdx.x]);
}

/* sah_step_descend (ROOT: sah_step_accumulate into the root), with the contributions of each run of lanes that fall
 * into one node merged by shuffles before the run's first lane issues the atomics. The merge is integer minima and
 * maxima, so the grouping does not show in the result. Every lane of a wave reaches every shuffle. */
template <bool ROOT>
__global__ __launch_bounds__(kSahBlock) void sah_descend_kernel(const SahBuild b, uint32_t level)
{
    const uint64_t p64 = (uint64_t)blockIdx.x * kSahBlock + threadIdx.x;
    const uint32_t p = (uint32_t)p64;
    uint32_t node = kSahNoNode;
    if (p64 < b.ntri) {
        if (ROOT) {
            node = 0u;
        } else {
            const uint32_t child = sah_child_of(b, p, level);
            if (child != 0u) {
                b.owner[p] = child;
                node = child;
            }
        }
    }
    SahContribution k;
    sah_contribution_none(k);
    if (node != kSahNoNode) sah_contribution(b, p, k);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        /* lanes of one node are contiguous: equal nodes at distance d mean one run, whose far part lane + d has */
        const bool same = __shfl_down(node, d) == node && lane + d < 64u;
        SahContribution o;
        for (int c = 0; c < 6; c++) {
            o.keys[c] = __shfl_down(k.keys[c], d);
            o.cen[c] = __shfl_down(k.cen[c], d);
        }
        if (same) sah_contribution_merge(k, o);
    }
    const bool head = __shfl_up(node, 1u) != node || lane == 0u;
    if (head && node != kSahNoNode) sah_contribution_into(b.tn[node], k);
}

} // namespace dev

namespace {

uint64_t align256(uint64_t x) { return (x + 255u) & ~255ull; }

uint32_t scan_blocks(uint32_t ntri) { return (uint32_t)(((uint64_t)ntri + 1u + (1u << kBvhScanShift) - 1u) >> kBvhScanShift); }

/* the scratch arrays of a build of ntri triangles, but the bins, carved from `base` (null: sizes only); returns the bytes */
uint64_t sah_carve(char* base, uint32_t ntri, SahBuild& b)
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
    take(b.starts, T + 1);
    take(b.lvl0, T);
    take(b.open_node, T);
    take(b.tn, 2 * T);
    take(b.idx_tmp, 3 * T);
    return at;
}

template <int STEP>
hipError_t launch_step(const SahBuild& b, uint64_t n, uint32_t level, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)((n + dev::kSahBlock - 1u) / dev::kSahBlock);
    hipLaunchKernelGGL(dev::sah_step_kernel<STEP>, dim3(grid), dim3(dev::kSahBlock), 0, stream, b, (uint32_t)n, level);
    return hipGetLastError();
}

hipError_t read_ctrl(const SahBuild& b, uint32_t ctrl[kBvhCtrlWords], hipStream_t stream)
{
    const hipError_t e = hipMemcpyAsync(ctrl, b.ctrl, sizeof(uint32_t) * kBvhCtrlWords, hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

} // namespace

uint64_t bvh_sah_scratch_bytes(uint32_t index_count)
{
    SahBuild b{};
    return sah_carve(nullptr, index_count / 3u, b);
}

#define SAH_TRY(expr)                    \
    do {                                 \
        const hipError_t _e = (expr);    \
        if (_e != hipSuccess) return _e; \
    } while (0)

hipError_t bvh_build_sah_device(const float* vertices, uint32_t vertex_count, uint32_t* indices, uint32_t index_count,
                                void* nodes, void* scratch, void** bins, uint64_t* bins_bytes, uint32_t* status,
                                uint32_t* nodes_used, hipStream_t stream)
{
    SahBuild b{};
    b.vertices = vertices;
    b.vertex_count = vertex_count;
    b.indices = indices;
    b.ntri = index_count / 3u;
    b.out = static_cast<wcpt_node*>(nodes);
    sah_carve(static_cast<char*>(scratch), b.ntri, b);
    const uint32_t T = b.ntri;
    const uint32_t grid = (T + dev::kSahBlock - 1u) / dev::kSahBlock;
    uint32_t ctrl[kBvhCtrlWords] = {0u, 0u, 0u, 0u};
    *status = 0u;

    /* nothing but the index buffer is read until every index has passed, and nothing of the caller's is written
     * before the last two launches */
    SAH_TRY(hipMemsetAsync(b.ctrl, 0, sizeof(uint32_t) * kBvhCtrlWords, stream));
    SAH_TRY(launch_step<dev::kSahCheckIndex>(b, index_count, 0u, stream));
    SAH_TRY(read_ctrl(b, ctrl, stream));
    if (ctrl[kBvhCtrlStatus]) {
        *status = ctrl[kBvhCtrlStatus];
        return hipSuccess;
    }
    SAH_TRY(launch_step<dev::kSahPrepare>(b, T, 0u, stream));
    SAH_TRY(read_ctrl(b, ctrl, stream));
    if (ctrl[kBvhCtrlStatus]) {
        *status = ctrl[kBvhCtrlStatus];
        return hipSuccess;
    }
    hipLaunchKernelGGL(dev::sah_descend_kernel<true>, dim3(grid), dim3(dev::kSahBlock), 0, stream, b, 0u);
    SAH_TRY(hipGetLastError());
    uint32_t open = sah_opens(T, 0u) ? 1u : 0u;
    for (uint32_t level = 0u; level <= kSahMaxDepth; level++) {
        SAH_TRY(launch_step<dev::kSahFinalize>(b, T, level, stream));
        if (open == 0u) break;
        if (open > T / 2u) return hipErrorUnknown; /* open nodes hold two triangles or more */
        const uint64_t need = (uint64_t)open * kSahBinsPerNode * sizeof(SahBin);
        if (*bins_bytes < need) { /* the stream is idle here: the control words were read */
            SAH_TRY(hipStreamSynchronize(stream));
            if (*bins) (void)hipFree(*bins);
            *bins = nullptr;
            *bins_bytes = 0;
            SAH_TRY(hipMalloc(bins, need));
            *bins_bytes = need;
        }
        b.bins = static_cast<SahBin*>(*bins);
        SAH_TRY(launch_step<dev::kSahBinInit>(b, (uint64_t)open * kSahBinsPerNode, level, stream));
        hipLaunchKernelGGL(dev::sah_bin_kernel, dim3((T + kSahBinSpan - 1u) / kSahBinSpan), dim3(dev::kSahBlock), 0, stream, b, level);
        SAH_TRY(hipGetLastError());
        SAH_TRY(launch_step<dev::kSahEvaluate>(b, open, level, stream));
        SAH_TRY(launch_step<dev::kSahClassify>(b, T, level, stream));
        SAH_TRY(bvh_launch_scan(b.flag, T + 1u, b.scan, b.scan_off, stream));
        SAH_TRY(launch_step<dev::kSahScatter>(b, T, level, stream));
        std::swap(b.perm, b.perm_next);
        hipLaunchKernelGGL(dev::sah_descend_kernel<false>, dim3(grid), dim3(dev::kSahBlock), 0, stream, b, level);
        SAH_TRY(hipGetLastError());
        SAH_TRY(read_ctrl(b, ctrl, stream));
        if (ctrl[kBvhCtrlStatus]) {
            *status = ctrl[kBvhCtrlStatus];
            return hipSuccess;
        }
        if (ctrl[kBvhCtrlSplits] == 0u) break;
        open = ctrl[kSahCtrlOpen];
    }
    const uint32_t used = ctrl[kBvhCtrlNodes];
    if (used == 0u || used > 2ull * T) return hipErrorUnknown; /* every node holds a triangle: at most 2 T - 1 */
    SAH_TRY(bvh_launch_scan(b.starts, T + 1u, b.scan, b.scan_off, stream));
    SAH_TRY(hipMemcpyAsync(b.idx_tmp, indices, sizeof(uint32_t) * 3ull * T, hipMemcpyDeviceToDevice, stream));
    SAH_TRY(launch_step<dev::kSahEmit>(b, used, 0u, stream));
    SAH_TRY(launch_step<dev::kSahPermute>(b, T, 0u, stream));
    SAH_TRY(hipStreamSynchronize(stream));
    *nodes_used = used;
    return hipSuccess;
}

#undef SAH_TRY

} // namespace wcpt
