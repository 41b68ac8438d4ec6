// Test shim (CPU): exposes the wavefront renderer's instance list, selection and frame plan
// (wc-path-tracer_amd/csrc/wf_plan.h, what launch_wavefront applies and pt_wavefront.hip's dispatcher instantiates) to
// tests/test_wf_plan.py over ctypes. Built by the test with g++; no HIP involved.
#include <cstddef>
#include <cstdint>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/wf_plan.h"

using namespace wcpt;

// a variant as five ints: count, diag, geo, ldsn, persist
static void put(const WfVariant& v, int* out)
{
    out[0] = v.count; out[1] = v.diag; out[2] = v.geo; out[3] = v.ldsn; out[4] = v.persist;
}
static WfVariant get(const int* f) { return WfVariant{f[0] != 0, f[1] != 0, f[2], f[3], f[4] != 0}; }

// the plan's inputs as 18 words: the base variant (5), mode, W, rows, samples, max_bounce, wf_fetch, wf_persist, pipes,
// sort, overlap, cus, trace_bpc, persist_bpc
constexpr int kIn = 18;
static WfFrameInputs inputs(const int64_t* w)
{
    const int v[5] = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], (int)w[4]};
    return WfFrameInputs{get(v), (int)w[5], (uint32_t)w[6], (uint32_t)w[7], (uint32_t)w[8], (uint32_t)w[9], (int)w[10],
                         (int)w[11], (int)w[12], w[13] != 0, (int)w[14], (int)w[15], (int)w[16], (int)w[17]};
}

extern "C" uint32_t wfp_codes(void) { return kWfVariantCodes; }
extern "C" int wfp_max_pipes(void) { return kWfMaxPipes; }
extern "C" void wfp_decode(uint32_t code, int* out) { put(wf_variant_decode(code), out); }
extern "C" uint32_t wfp_code(const int* f) { return wf_variant_code(get(f)); }
extern "C" int wfp_built(const int* f) { return wf_variant_built(get(f)) ? 1 : 0; }
extern "C" void wfp_select(int mode, uint32_t draws, int wf_fast, int lds_stack, int* out)
{
    put(wf_variant_select(mode, draws, wf_fast != 0, lds_stack), out);
}
extern "C" void wfp_persist_variant(int* out) { put(wf_persist_variant(), out); }
extern "C" int wfp_persist_eligible(const int* base, uint32_t samples, int sort, int wf_persist)
{
    return wf_persist_eligible(get(base), samples, sort != 0, wf_persist) ? 1 : 0;
}
extern "C" int wfp_short_queue(uint64_t paths, uint32_t trace_grid) { return wf_short_queue(paths, trace_grid) ? 1 : 0; }
extern "C" uint32_t wfp_iterations(int mode, uint32_t samples, uint32_t max_bounce)
{
    return wf_iterations(mode, samples, max_bounce);
}
// out: tiles, total, paths
extern "C" void wfp_share(uint32_t W, uint32_t rows, uint32_t j, uint32_t K, uint32_t* out)
{
    const WfShare s = wf_pipe_share(W, rows, j, K);
    out[0] = s.tiles; out[1] = s.total; out[2] = s.paths;
}

// out: ok, empty, persist, W, rows, K, trace_grid, shade_grid, persist_grid, then for each of kWfMaxPipes pipelines
// tiles, total, paths, init_grid, geo, iters and the five fields of the instance it launches (zeros past K)
constexpr int kHead = 9, kPipe = 11;
extern "C" void wfp_plan(const int64_t* w, int64_t* out)
{
    const WfFrameInputs in = inputs(w);
    const WfFramePlan p = wf_frame_plan(in);
    const int64_t head[kHead] = {p.ok, p.empty, p.persist, p.W, p.rows, p.K, p.trace_grid, p.shade_grid, p.persist_grid};
    for (int i = 0; i < kHead; i++) out[i] = head[i];
    for (uint32_t j = 0; j < (uint32_t)kWfMaxPipes; j++) {
        int64_t* o = out + kHead + kPipe * j;
        const WfPipePlan& q = p.pipe[j];
        const int64_t f[6] = {q.tiles, q.total, q.paths, q.init_grid, q.geo, q.iters};
        for (int i = 0; i < 6; i++) o[i] = f[i];
        int v[5] = {0, 0, 0, 0, 0};
        if (j < p.K) put(wf_pipe_variant(p, in.base, j), v);
        for (int i = 0; i < 5; i++) o[6 + i] = v[i];
    }
}

// pending: pending, pipes, W, rows, persist
extern "C" int wfp_continues(const int64_t* w, int mode, int overlap, const uint32_t* pending)
{
    const WfFramePlan p = wf_frame_plan(inputs(w));
    const WfPending q = {pending[0] != 0, pending[1], pending[2], pending[3], pending[4] != 0};
    return wf_frame_continues(p, mode, overlap, q) ? 1 : 0;
}

// ---- the launch record (include/wcpt.h wcpt_wf_plan_info, filled by launch_wavefront, read by wcpt_wf_last_plan) ----
// Its layout, for the Python mirror: the size, then the offsets of launches, mode, K, continued, pipe, pipe[1], base_code,
// persist_bpc.
extern "C" void wfp_record_layout(uint32_t* out)
{
    out[0] = (uint32_t)sizeof(wcpt_wf_plan_info);
    out[1] = (uint32_t)offsetof(wcpt_wf_plan_info, launches);
    out[2] = (uint32_t)offsetof(wcpt_wf_plan_info, mode);
    out[3] = (uint32_t)offsetof(wcpt_wf_plan_info, K);
    out[4] = (uint32_t)offsetof(wcpt_wf_plan_info, continued);
    out[5] = (uint32_t)offsetof(wcpt_wf_plan_info, pipe);
    out[6] = (uint32_t)(offsetof(wcpt_wf_plan_info, pipe) + sizeof(wcpt_wf_pipe_info));
    out[7] = (uint32_t)offsetof(wcpt_wf_plan_info, base_code);
    out[8] = (uint32_t)offsetof(wcpt_wf_plan_info, persist_bpc);
}
static_assert(WCPT_WF_MAX_PIPES == kWfMaxPipes, "the record holds every pipeline");

static WfFrameInputs record_inputs(const wcpt_wf_plan_info& r)
{
    return WfFrameInputs{wf_variant_decode(r.base_code), r.mode, r.width, r.rows, r.samples, r.max_bounce, r.wf_fetch,
                         r.wf_persist, r.pipes, r.sort != 0, r.overlap, r.cus, r.trace_bpc, r.persist_bpc};
}

// The model a GPU test holds a record against: what wf_frame_plan and wf_pipe_variant make of the inputs that `rec`
// reports, as a record. `launches` and `continued` are not the plan's and are copied (wfp_record_continues has the
// latter). Returns 0 if the reported base instance is not built or its code out of range (then *out is zeroed).
extern "C" int wfp_record_expect(const wcpt_wf_plan_info* rec, wcpt_wf_plan_info* out)
{
    *out = wcpt_wf_plan_info{};
    if (rec->base_code >= kWfVariantCodes) return 0;
    const WfFrameInputs in = record_inputs(*rec);
    if (!wf_variant_built(in.base) || in.base.persist) return 0;
    const WfFramePlan p = wf_frame_plan(in);
    *out = *rec; // the inputs, launches, continued
    out->ok = p.ok;
    out->empty = p.empty;
    out->persist = p.persist;
    out->K = p.K;
    out->trace_grid = p.trace_grid;
    out->shade_grid = p.shade_grid;
    out->persist_grid = p.persist_grid;
    for (uint32_t j = 0; j < (uint32_t)kWfMaxPipes; j++) {
        wcpt_wf_pipe_info& q = out->pipe[j];
        q = wcpt_wf_pipe_info{WCPT_WF_NO_VARIANT, 0u, 0u, 0u, 0u};
        if (j >= p.K) continue;
        q.variant_code = wf_variant_code(wf_pipe_variant(p, in.base, j));
        q.dispatches = p.persist ? 1u : p.pipe[j].iters;
        q.tiles = p.pipe[j].tiles;
        q.paths = p.pipe[j].paths;
        q.iters = p.pipe[j].iters;
    }
    return 1;
}

// Whether the launch `rec` reports continues behind the launch `prev` reports (null: nothing is pending -- the first
// launch, or another entry point joined the pipelines in between). A launch leaves its pipelines unjoined exactly when
// it ran several of them as a render under the overlap (launch_wavefront's last lines).
extern "C" int wfp_record_continues(const wcpt_wf_plan_info* rec, const wcpt_wf_plan_info* prev)
{
    WfPending q = {};
    if (prev && prev->ok && !prev->empty && prev->K > 1u && prev->overlap != 0 && prev->mode == kModeRender)
        q = WfPending{true, prev->K, prev->width, prev->rows, prev->persist != 0};
    return wf_frame_continues(wf_frame_plan(record_inputs(*rec)), rec->mode, rec->overlap, q) ? 1 : 0;
}

// the build's persistent GEO (WCPT_WF_PERSIST_GEO): the other persistent instance is compiled but never selected
extern "C" int wfp_persist_geo(void) { return WCPT_WF_PERSIST_GEO; }

// The selection and a plan evaluated by the compiler: the functions are usable in constant expressions (the
// dispatcher's `if constexpr (wf_variant_built(...))` needs that of the list). 1920x1080, one draw on the fast layout,
// one sample, every option automatic, overlap on, 256 CUs at 32 and 16 blocks per CU.
constexpr WfVariant kBase = wf_variant_select(kModeRender, 1u, true, 0);
static_assert(!kBase.count && !kBase.diag && kBase.geo == 2 && kBase.ldsn == 10 && !kBase.persist, "the fast-layout render");
static_assert(wf_variant_built(kBase) && wf_variant_built(wf_persist_variant()), "what a launch takes is built");
static_assert(wf_variant_select(kModeCount, 2u, true, 16).geo == 0 && wf_variant_select(kModeCount, 2u, true, 16).ldsn == 10,
              "counting runs take the 10-entry stack");
constexpr WfFramePlan kPlan = wf_frame_plan(WfFrameInputs{kBase, kModeRender, 1920u, 1080u, 1u, 4u, -1, -1, 0, false, 1, 256, 32, 16});
static_assert(kPlan.ok && !kPlan.empty && !kPlan.persist && kPlan.K == 3u && kPlan.trace_grid == 2730u &&
                  kPlan.shade_grid == 1024u && kPlan.persist_grid == 0u,
              "the 1080p plan");
static_assert(kPlan.pipe[2].paths == 691200u && kPlan.pipe[2].init_grid == 2700u && kPlan.pipe[2].geo == 3 &&
                  kPlan.pipe[2].iters == 5u,
              "its third pipeline");
static_assert(wf_variant_code(wf_pipe_variant(kPlan, kBase, 0)) < kWfVariantCodes, "the cache's index");
static_assert(!wf_frame_continues(kPlan, kModeRender, 1, WfPending{}) &&
                  wf_frame_continues(kPlan, kModeRender, 1, WfPending{true, 3u, 1920u, 1080u, false}),
              "the continuation predicate");
