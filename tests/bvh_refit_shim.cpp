/* The level-by-level refit on the host, from wc-path-tracer_amd/csrc/bvh_refit.h alone: every launch of pt_bvh_refit.hip
 * becomes a loop over the indices its threads would have, calling the same refit_step_* function, in the device's launch
 * order: clear, index check, node step, depth step, the status read, one pass per depth from the deepest, store. The
 * loops can visit their indices in three orders (forward, backward, a stride coprime to the count), since no step may
 * depend on the order in which its threads run. Returns 0, or the status bits of a refused refit (kRefit*), with no
 * byte of `nodes` written. */
#include <cstdint>
#include <vector>

#include "../wc-path-tracer_amd/csrc/bvh_refit.h"

namespace {

using namespace wcpt;

template <class F>
void for_each(uint32_t n, int order, F f)
{
    if (order == 0) {
        for (uint32_t i = 0; i < n; i++) f(i);
    } else if (order == 1) {
        for (uint32_t i = n; i-- > 0;) f(i);
    } else {
        uint64_t stride = 7919;
        while (n % stride == 0) stride += 2; /* 7919 is prime: coprime unless it divides n */
        uint64_t at = n / 2;
        for (uint32_t i = 0; i < n; i++, at = (at + stride) % n) f((uint32_t)at);
    }
}

} // namespace

extern "C" int bvh_refit_levels(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                                wcpt_node* nodes, uint32_t nodes_used, int order)
{
    const uint32_t N = nodes_used;
    std::vector<RefitBox> box(N);
    std::vector<uint32_t> parent(N, kRefitNone), refs(N, 0u), depth(N, 0u), ctrl(kRefitCtrlWords, 0u);
    const BvhRefit r{positions, vertex_count, indices, index_count, nodes, N, box.data(), parent.data(), refs.data(),
                     depth.data(), ctrl.data()};
    for_each(index_count, order, [&](uint32_t i) { refit_step_check_index(r, i); });
    for_each(N, order, [&](uint32_t i) { refit_step_node(r, i); });
    for_each(N, order, [&](uint32_t i) { refit_step_depth(r, i); });
    if (ctrl[kRefitCtrlStatus]) return (int)ctrl[kRefitCtrlStatus];
    for (uint32_t d = ctrl[kRefitCtrlDepth] + 1u; d-- > 0u;) for_each(N, order, [&](uint32_t i) { refit_step_unite(r, i, d); });
    for_each(N, order, [&](uint32_t i) { refit_step_store(r, i); });
    return 0;
}

/* what the entry points say about a status */
extern "C" const char* bvh_refit_refusal_text(uint32_t status) { return refit_refusal(status); }
