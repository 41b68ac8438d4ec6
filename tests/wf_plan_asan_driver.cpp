// CPU test driver for tests/test_wf_plan_sanitizers.py: the wavefront launch rules (wc-path-tracer_amd/csrc/wf_plan.h,
// what launch_wavefront evaluates on every render) under AddressSanitizer and UndefinedBehaviorSanitizer -- the frames at
// the edges of 32 bits and a sweep over frames, modes, options, occupancies and CU counts, with the plan's own
// invariants checked on each: the pipelines' shares partition the tiles, nothing is written past the K pipelines, every
// grid is at least 1, whatever a pipeline launches is built. A signed overflow, an out-of-range shift or an index past
// pipe[kWfMaxPipes] is a sanitizer report, which aborts the process; the checks below return 1.
// The launch record's model (tests/wf_plan_shim.cpp wfp_record_expect and wfp_record_continues, what tests/wf_record.py
// holds a GPU render's wcpt_wf_last_plan against) runs here too, on records filled the way launch_wavefront fills them:
// the shim's source is part of this program, nothing is loaded.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "wf_plan_shim.cpp" // includes include/wcpt.h and wc-path-tracer_amd/csrc/wf_plan.h

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

static WfFrameInputs inputs(int mode, uint32_t draws, bool fast, int stack, uint32_t W, uint32_t rows)
{
    return WfFrameInputs{wf_variant_select(mode, draws, fast, stack), mode, W, rows, 1u, 4u, -1, -1, 0, false, 1, 256, 32, 16};
}

/* the record launch_wavefront makes of a plan it carried out whole (pt_wavefront.hip wf_record, pipe_iterate) */
static wcpt_wf_plan_info record_of(const WfFrameInputs& in, const WfFramePlan& p)
{
    wcpt_wf_plan_info r = {};
    r.launches = 1;
    r.mode = in.mode;
    r.ok = p.ok;
    r.empty = p.empty;
    r.persist = p.persist;
    r.K = p.K;
    r.trace_grid = p.trace_grid;
    r.shade_grid = p.shade_grid;
    r.persist_grid = p.persist_grid;
    r.sort = in.sort;
    for (uint32_t j = 0; j < (uint32_t)kWfMaxPipes; j++) {
        r.pipe[j].variant_code = WCPT_WF_NO_VARIANT;
        if (j >= p.K) continue;
        r.pipe[j].variant_code = wf_variant_code(wf_pipe_variant(p, in.base, j));
        r.pipe[j].dispatches = p.persist ? 1u : p.pipe[j].iters;
        r.pipe[j].tiles = p.pipe[j].tiles;
        r.pipe[j].paths = p.pipe[j].paths;
        r.pipe[j].iters = p.pipe[j].iters;
    }
    r.base_code = wf_variant_code(in.base);
    r.width = in.W;
    r.rows = in.rows;
    r.samples = in.samples;
    r.max_bounce = in.max_bounce;
    r.wf_fetch = in.wf_fetch;
    r.wf_persist = in.wf_persist;
    r.pipes = in.pipes;
    r.overlap = in.overlap;
    r.cus = in.cus;
    r.trace_bpc = in.trace_bpc;
    r.persist_bpc = in.persist_bpc;
    return r;
}

/* the record's model gives back a true record, tells a wrong instance, and continues where wf_frame_continues does */
static void record_model(const WfFrameInputs& in, const WfFramePlan& p)
{
    static_assert(sizeof(wcpt_wf_plan_info) == 176, "no padding: the records are compared as bytes");
    wcpt_wf_plan_info r = record_of(in, p), want;
    CHECK(wfp_record_expect(&r, &want) == 1);
    CHECK(std::memcmp(&r, &want, sizeof(r)) == 0);
    if (p.ok && !p.empty) {
        wcpt_wf_plan_info bad = r;
        bad.pipe[p.K - 1u].variant_code ^= 1u; /* the counting twin of the instance */
        CHECK(wfp_record_expect(&bad, &want) == 1 && std::memcmp(&bad, &want, sizeof(bad)) != 0);
        CHECK(want.pipe[p.K - 1u].variant_code == r.pipe[p.K - 1u].variant_code);
    }
    CHECK(!wfp_record_continues(&r, nullptr));
    CHECK((wfp_record_continues(&r, &r) != 0) == (p.ok && !p.empty && in.overlap != 0 && p.K > 1u && in.mode == kModeRender));
    wcpt_wf_plan_info off = r;
    off.base_code = kWfVariantCodes; /* no instance: refused, the output zeroed */
    CHECK(wfp_record_expect(&off, &want) == 0 && want.launches == 0u && want.K == 0u);
}

/* what holds of every plan */
static void invariants(const WfFrameInputs& in, const WfFramePlan& p)
{
    const uint64_t pixels = (uint64_t)in.W * in.rows;
    const uint64_t tiles = (((uint64_t)in.W + 7u) / 8u) * (((uint64_t)in.rows + 7u) / 8u);
    CHECK(p.W == in.W && p.rows == in.rows);
    CHECK(p.empty == (pixels == 0u));
    CHECK(p.ok == (pixels <= 0xFFFFFFFFull && tiles * 64u <= 0xFFFFFFC0ull));
    if (!p.ok || p.empty) {
        CHECK(p.K == 0u && !p.persist && p.persist_grid == 0u);
        return;
    }
    CHECK(p.K >= 1u && p.K <= (uint32_t)kWfMaxPipes && p.K <= tiles);
    CHECK(p.trace_grid >= 1u && p.shade_grid >= 1u && (p.persist_grid != 0u) == p.persist);
    CHECK(!p.persist || wf_persist_eligible(in.base, in.samples, in.sort, in.wf_persist));
    uint64_t sum = 0;
    for (uint32_t j = 0; j < (uint32_t)kWfMaxPipes; j++) {
        const WfPipePlan& q = p.pipe[j];
        if (j >= p.K) {
            CHECK(q.tiles == 0u && q.total == 0u && q.paths == 0u && q.init_grid == 0u && q.iters == 0u);
            continue;
        }
        const WfShare s = wf_pipe_share(in.W, in.rows, j, p.K);
        CHECK(s.tiles == q.tiles && s.total == q.total && s.paths == q.paths);
        CHECK(q.tiles >= 1u && q.total == q.tiles * 64u && q.paths <= q.total && q.paths <= pixels && q.init_grid >= 1u);
        CHECK(q.iters == wf_iterations(in.mode, in.samples, in.max_bounce) && q.iters <= kWfMaxIters);
        const WfVariant v = wf_pipe_variant(p, in.base, j);
        CHECK(wf_variant_built(v) && wf_variant_code(v) < kWfVariantCodes && v.geo == q.geo && v.persist == p.persist);
        sum += q.tiles;
    }
    CHECK(sum == tiles);
    const WfPending same = {true, p.K, p.W, p.rows, p.persist};
    CHECK(wf_frame_continues(p, in.mode, in.overlap, same) == (in.overlap != 0 && p.K > 1u && in.mode == kModeRender));
    CHECK(!wf_frame_continues(p, in.mode, in.overlap, WfPending{}));
}

static void edges()
{
    const uint32_t big[] = {0u, 1u, 7u, 8u, 9u, 65529u, 65535u, 65536u, 65537u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFC0u / 8u,
                            8u * ((1u << 26) - 1u), 8u * ((1u << 26) - 1u) + 1u, 0xFFFFFFF8u, 0xFFFFFFF9u, 0xFFFFFFFFu};
    for (uint32_t W : big)
        for (uint32_t rows : big)
            for (int pipes : {0, 1, 4}) {
                WfFrameInputs in = inputs(kModeRender, 1u, true, 0, W, rows);
                in.pipes = pipes;
                invariants(in, wf_frame_plan(in));
                record_model(in, wf_frame_plan(in));
            }
    /* the last frame accepted, and the first refused by its lanes alone */
    CHECK(wf_frame_plan(inputs(kModeRender, 1u, true, 0, 8u, 8u * ((1u << 26) - 1u))).ok);
    CHECK(wf_frame_plan(inputs(kModeRender, 1u, true, 0, 8u, 8u * ((1u << 26) - 1u))).pipe[0].paths == 0x80000000u);
    CHECK(!wf_frame_plan(inputs(kModeRender, 1u, true, 0, 65529u, 65529u)).ok);
    CHECK(!wf_frame_plan(inputs(kModeRender, 1u, true, 0, 65536u, 65536u)).ok);
    /* iteration counts at the ends of their inputs */
    for (int mode : {kModeRender, kModeCount, kModeDiag})
        for (uint32_t s : {0u, 1u, 2u, 0xFFFFFFFFu})
            for (uint32_t b : {0u, 1u, (1u << 20) - 1u, 1u << 20, 0xFFFFFFFFu}) CHECK(wf_iterations(mode, s, b) <= kWfMaxIters);
    CHECK(wf_iterations(kModeRender, 1u, (1u << 20) - 1u) == kWfMaxIters && wf_iterations(kModeRender, 1u, (1u << 20) - 2u) == kWfMaxIters - 1u);
    /* the numbering */
    uint32_t built = 0;
    for (uint32_t c = 0; c < kWfVariantCodes; c++) {
        const WfVariant v = wf_variant_decode(c);
        CHECK(wf_variant_code(v) == c);
        built += wf_variant_built(v) ? 1u : 0u;
    }
    CHECK(built == 12u);
}

static void sweep(std::mt19937& rng)
{
    const uint32_t dims[] = {1u, 5u, 8u, 9u, 17u, 64u, 100u, 135u, 136u, 216u, 360u, 640u, 1080u, 1920u, 2160u, 3840u};
    const int nd = (int)(sizeof(dims) / sizeof(dims[0]));
    auto pick = [&](std::initializer_list<int> l) { return l.begin()[rng() % l.size()]; };
    for (int it = 0; it < 200000; it++) {
        const int mode = pick({kModeRender, kModeRender, kModeCount, kModeDiag});
        WfFrameInputs in = inputs(mode, (uint32_t)pick({0, 1, 1, 2}), pick({0, 1, 1}) != 0, pick({0, 10, 16, 24, 7}),
                                  dims[rng() % nd], dims[rng() % nd]);
        in.samples = (uint32_t)pick({0, 1, 1, 1, 2, 5});
        in.max_bounce = (uint32_t)pick({0, 1, 4, 8, 1 << 20});
        in.wf_fetch = pick({-1, -1, 0, 1});
        in.wf_persist = pick({-1, -1, 0, 1});
        in.pipes = pick({-1, 0, 0, 1, 2, 3, 4, 5, 1 << 30});
        in.sort = pick({0, 0, 1}) != 0;
        in.overlap = pick({0, 1, 2});
        in.cus = pick({1, 64, 256, 304});
        in.trace_bpc = pick({1, 8, 20, 32});
        in.persist_bpc = pick({1, 4, 16});
        invariants(in, wf_frame_plan(in));
        if (it % 8 == 0) record_model(in, wf_frame_plan(in));
    }
}

int main()
{
    std::mt19937 rng(20240917u);
    edges();
    sweep(rng);
    std::printf("%d failed checks\n", failures);
    return failures ? 1 : 0;
}
