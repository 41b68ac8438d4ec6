/*
 * pt_bvh_refit.hip — wcpt_bvh_refit_device: the boxes of a BVH recomputed from moved vertices, on the device.
 *
 * What is computed, and what is refused, is stated in bvh_refit.h (refit_step_*: one call per index or node and step, the
 * same functions tests/bvh_refit_shim.cpp runs as host loops); this file is how the steps are spread over the machine.
 * Every step is one launch of one thread per element. A step reads what the step before wrote: stream order is the only
 * synchronisation between workgroups, so there is no hand-off inside a launch and no fence in a kernel.
 *
 * memset (parents none, reference counts and control words 0) -> index check -> node step (validation, parents,
 * reference counts, the leaves' boxes) -> depth step -> the one read-back (status, deepest interior depth; a refusal
 * returns here, with nothing of the caller's written) -> one launch per depth, deepest first -> store.
 *
 * Bounds of what is read: a node number is < nodes_used (the children by the node step's check, before anything follows
 * them); a leaf's index range lies inside index_count by the same check; no index is used as an address once the index
 * check, which reads nothing else, has set its bit. All scratch arrays hold nodes_used elements.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pt_kernels.h"
#include "bvh_refit.h"

namespace wcpt {
namespace dev {

constexpr uint32_t kRefitBlock = 256u;

enum RefitStep { kRefitCheckIndex, kRefitNode, kRefitDepth, kRefitUnite, kRefitStore };

template <int STEP>
__global__ __launch_bounds__(kRefitBlock) void bvh_refit_kernel(const BvhRefit r, uint32_t n, uint32_t d)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    if (STEP == kRefitCheckIndex) refit_step_check_index(r, i);
    if (STEP == kRefitNode) refit_step_node(r, i);
    if (STEP == kRefitDepth) refit_step_depth(r, i);
    if (STEP == kRefitUnite) refit_step_unite(r, i, d);
    if (STEP == kRefitStore) refit_step_store(r, i);
}

} // namespace dev

namespace {

uint64_t align256(uint64_t x) { return (x + 255u) & ~255ull; }

/* the scratch arrays of a refit of `nodes` nodes, carved from `base` (null: sizes only); returns the bytes. parent[],
 * refs[] and ctrl[] are adjacent: one memset each of 0xFF and 0 covers them (refit_clear) */
uint64_t refit_carve(char* base, uint32_t nodes, BvhRefit& r)
{
    uint64_t at = 0;
    auto take = [&](auto*& p, uint64_t count) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at = align256(at + count * sizeof(T));
    };
    const uint64_t N = nodes;
    take(r.parent, N);
    take(r.refs, N);
    take(r.ctrl, kRefitCtrlWords);
    take(r.depth, N);
    take(r.box, N);
    return at;
}

template <int STEP>
hipError_t launch_refit(const BvhRefit& r, uint32_t n, uint32_t d, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)n + dev::kRefitBlock - 1u) / dev::kRefitBlock);
    hipLaunchKernelGGL(dev::bvh_refit_kernel<STEP>, dim3(grid), dim3(dev::kRefitBlock), 0, stream, r, n, d);
    return hipGetLastError();
}

} // namespace

uint64_t bvh_refit_scratch_bytes(uint32_t nodes_used)
{
    BvhRefit r{};
    return refit_carve(nullptr, nodes_used, r);
}

#define REFIT_TRY(expr)                  \
    do {                                 \
        const hipError_t _e = (expr);    \
        if (_e != hipSuccess) return _e; \
    } while (0)

hipError_t bvh_refit_device(const float* vertices, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                            void* nodes, uint32_t nodes_used, void* scratch, uint32_t* status, hipStream_t stream)
{
    BvhRefit r{};
    r.vertices = vertices;
    r.vertex_count = vertex_count;
    r.indices = indices;
    r.index_count = index_count;
    r.nodes = static_cast<wcpt_node*>(nodes);
    r.nodes_used = nodes_used;
    refit_carve(static_cast<char*>(scratch), nodes_used, r);
    const uint32_t N = nodes_used;
    *status = 0u;

    REFIT_TRY(hipMemsetAsync(r.parent, 0xFF, sizeof(uint32_t) * (uint64_t)N, stream));
    REFIT_TRY(hipMemsetAsync(r.refs, 0, reinterpret_cast<char*>(r.ctrl + kRefitCtrlWords) - reinterpret_cast<char*>(r.refs), stream));
    REFIT_TRY(launch_refit<dev::kRefitCheckIndex>(r, index_count, 0u, stream));
    REFIT_TRY(launch_refit<dev::kRefitNode>(r, N, 0u, stream));
    REFIT_TRY(launch_refit<dev::kRefitDepth>(r, N, 0u, stream));
    uint32_t ctrl[kRefitCtrlWords] = {0u, 0u, 0u, 0u};
    REFIT_TRY(hipMemcpyAsync(ctrl, r.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, stream));
    REFIT_TRY(hipStreamSynchronize(stream));
    if (ctrl[kRefitCtrlStatus]) {
        *status = ctrl[kRefitCtrlStatus];
        return hipSuccess;
    }
    if (ctrl[kRefitCtrlDepth] >= N) return hipErrorUnknown; /* an interior node of depth d has d ancestors */
    for (uint32_t d = ctrl[kRefitCtrlDepth] + 1u; d-- > 0u;) REFIT_TRY(launch_refit<dev::kRefitUnite>(r, N, d, stream));
    REFIT_TRY(launch_refit<dev::kRefitStore>(r, N, 0u, stream));
    return hipStreamSynchronize(stream);
}

#undef REFIT_TRY

} // namespace wcpt
