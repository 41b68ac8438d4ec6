/* wf_plan.h — the wavefront renderer's launch rules as values: which wf_trace instances are compiled (WfVariant,
 * wf_variant_built), which of them a launch takes (wf_variant_select, wf_persist_eligible), and everything
 * launch_wavefront decides about a frame before it touches the device (wf_frame_plan): whether the path-persistent trace
 * runs, the pipeline count, the grids, and each pipeline's tiles, paths, fetch rounds and iterations. Plain C++17, no
 * HIP: tests/wf_plan_shim.cpp compiles it with g++, and pt_wavefront.hip turns a runtime WfVariant into wf_trace's
 * template arguments (wf_dispatch), so this file is the list of instances. Everything is constexpr on fixed-size
 * arrays: the plan is computed on every render.
 *
 * The instances (a device code object holds 12 wf_trace):
 *    6 render    per-bounce launches: any draws (GEO 0); one draw (GEO 1) on an LDS stack of 10, 16 or 24 entries; one
 *                draw on the fast layout with two fetch rounds per iteration (GEO 2) or one (GEO 3)
 *    2 count     the counting build, GEO 0 and 1
 *    2 diag      ... with the SIMD step counters and the phase timers, GEO 0 and 1
 *    2 persist   the path-persistent render, GEO 2 and 3
 * All but render GEO 1 take the 10-entry stack.
 * Eleven of the twelve can be launched. wf_persist_variant() fixes the persistent trace's GEO when the library is compiled
 * (WCPT_WF_PERSIST_GEO, 3), so the persistent instance of the other GEO (2) is in the code object and no launch selects
 * it: it is there for a build with the macro set the other way, which then leaves GEO 3 unreachable.
 * tests/test_gpu_wf_variants.py launches the eleven, each asserted from the launch record (wcpt_wf_last_plan), and
 * asserts that the twelfth is exactly the built set's remainder. */
#ifndef WCPT_WF_PLAN_H
#define WCPT_WF_PLAN_H

#include <stdint.h>

#include "mk_variant.h"

namespace wcpt {

/* Concurrent wavefront pipelines (WCPT_OPTION_WF_PIPES): at most this many (pt_kernels.h WfPipes). */
constexpr int kWfMaxPipes = 4;
constexpr uint32_t kWfShadeBlock = 256; /* threads of a wf_init and of a wf_shade block */

/* The five values an instance is specialised on, in the order of wf_trace's template parameters. */
struct WfVariant {
    bool count;   /* counts the reference's work instead of rendering */
    bool diag;    /* ... and the SIMD lane / wave steps and the loop's phase timers */
    int geo;      /* 0 any draws; 1 one draw; 2 one draw on the fast layout; 3 the same with one fetch round per iteration */
    int ldsn;     /* LDS traversal-stack entries per lane: 10, 16 or 24 */
    bool persist; /* the path-persistent trace: one launch runs every segment of its paths */
};

/* Which combinations are compiled: the single statement of it (the dispatcher instantiates exactly these). */
constexpr bool wf_variant_built(const WfVariant& v)
{
    if (v.geo < 0 || v.geo > 3 || (v.ldsn != 10 && v.ldsn != 16 && v.ldsn != 24)) return false;
    if (v.geo != 1 && v.ldsn != 10) return false; /* the deeper stacks exist for the one-draw render only */
    if (v.persist) return !v.count && !v.diag && v.geo >= 2; /* render, fast layout */
    if (v.diag && !v.count) return false; /* the diagnostics are counters */
    if (v.count) return v.geo <= 1 && v.ldsn == 10; /* the counting builds walk the reference's layout */
    return true;
}

/* Dense numbering of the field combinations, for enumerating them and for the occupancy cache (pt_kernels.h
 * WfState::bpc): wf_variant_decode(c) for c < kWfVariantCodes is every combination once. */
constexpr uint32_t kWfVariantCodes = 2u * 2u * 4u * 3u * 2u;
constexpr WfVariant wf_variant_decode(uint32_t c)
{
    WfVariant v = {};
    v.count = c % 2u != 0u;   c /= 2u;
    v.diag = c % 2u != 0u;    c /= 2u;
    v.geo = (int)(c % 4u);    c /= 4u;
    v.ldsn = c % 3u == 0u ? 10 : (c % 3u == 1u ? 16 : 24); c /= 3u;
    v.persist = c % 2u != 0u;
    return v;
}
/* of a combination whose fields are in range (every built one is) */
constexpr uint32_t wf_variant_code(const WfVariant& v)
{
    uint32_t c = v.persist ? 1u : 0u;
    c = c * 3u + (v.ldsn == 10 ? 0u : (v.ldsn == 16 ? 1u : 2u));
    c = c * 4u + (uint32_t)v.geo;
    c = c * 2u + (v.diag ? 1u : 0u);
    c = c * 2u + (v.count ? 1u : 0u);
    return c;
}

/* The selection: the base variant of a launch, whose occupancy sizes the trace grid. mode: kModeRender / Count / Diag;
 * draws: drawCommandCount; wf_fast: LaunchArgs::wf_fast; lds_stack: WCPT_OPTION_WF_STACK. Every variant returned is
 * built.
 *   - geo: 0 any draws, 1 one draw (the reference's case, PathTracingRenderer.jai:251), 2 one draw on the fast layout
 *     (render build, the default LDS stack). A pipeline may trace GEO 3 instead of 2 (wf_pipe_geo), at GEO 2's
 *     occupancy: both run 8 waves/SIMD;
 *   - ldsn: the option normalised to 10, 16 or 24; only the one-draw render has the deeper stacks, so counting and
 *     diagnostics runs and renders of any other draw count take 10. */
constexpr WfVariant wf_variant_select(int mode, uint32_t draws, bool wf_fast, int lds_stack)
{
    const int ldsn = (lds_stack == 16 || lds_stack == 24) ? lds_stack : 10;
    WfVariant v = {};
    v.count = mode != kModeRender;
    v.diag = mode == kModeDiag;
    v.geo = draws != 1u ? 0 : ((wf_fast && mode == kModeRender && ldsn == 10) ? 2 : 1);
    v.ldsn = (mode == kModeRender && v.geo == 1) ? ldsn : 10;
    v.persist = false;
    return v;
}

/* The path-persistent trace (WCPT_OPTION_WF_PERSIST): one launch for every segment of a pipeline's paths. */
#ifndef WCPT_WF_PERSIST_GEO
#define WCPT_WF_PERSIST_GEO 3 /* the persistent trace's fetch rounds: 3 one per iteration, 2 two */
#endif
constexpr WfVariant wf_persist_variant() { return WfVariant{false, false, WCPT_WF_PERSIST_GEO, 10, true}; }

/* Whether a launch may run on the persistent trace at all -- known before its occupancy is queried: a render of one
 * sample per pixel on the fast layout, unsorted, and the option not 0. sort: the ray sort as it runs (the option, and
 * there are draws to sort by). */
constexpr bool wf_persist_eligible(const WfVariant& base, uint32_t samples, bool sort, int wf_persist)
{
    return !base.count && !base.diag && base.geo == 2 && samples == 1u && !sort && wf_persist != 0;
}

/* A queue is short when it holds at most WCPT_WF_FETCH_ONCE_RATIO rays per lane of the `trace_grid` resident waves
 * it is compared with. The one threshold has two uses, which compare different things (wf_pipe_geo, wf_frame_plan). */
#ifndef WCPT_WF_FETCH_ONCE_RATIO
#define WCPT_WF_FETCH_ONCE_RATIO 8
#endif
constexpr bool wf_short_queue(uint64_t paths, uint32_t trace_grid)
{
    return paths <= (uint64_t)WCPT_WF_FETCH_ONCE_RATIO * 64ull * trace_grid;
}

/* One fetch round per trace iteration (GEO 3) or two (GEO 2: a lane that descends into a leaf tests its first
 * triangle in the same iteration, after the interior lanes' fetch). One round overlaps the interior and leaf lanes'
 * fetches, which pays where fetch latency is exposed -- few queued rays per resident lane, so much of the launch is
 * its tail -- and costs an iteration per leaf descent, which loses where the chip is issue-bound on a long queue.
 * Measured (profiles/r05_fetch_once_ab.log): c3 (4.0 rays per lane per pipeline) 4.52 against 4.66 ms; c4 (15.8)
 * 203.6 against 199.6 ms. WCPT_OPTION_WF_FETCH: -1 (default) by that ratio, 0 two rounds, 1 one round.
 * This use of the threshold compares one pipeline's paths with that pipeline's trace grid, after the division by K. */
constexpr int wf_pipe_geo(const WfVariant& base, int wf_fetch, uint32_t paths, uint32_t trace_grid)
{
    if (base.geo != 2 || wf_fetch == 0) return base.geo;
    if (wf_fetch > 0) return 3;
    return wf_short_queue(paths, trace_grid) ? 3 : 2;
}

/* A pipeline's share of the frame: pipeline j of K owns the 8x8 tiles t with t % K == j. `total` is the lanes of its
 * ray generation (64 per tile) and `paths` its live paths at most -- its pixels, so the slot arrays are sized by its
 * share of the tiles, not the frame. Of a frame that wf_frame_plan accepts; a pipeline past the last tile has none. */
struct WfShare {
    uint32_t tiles, total, paths;
};
constexpr WfShare wf_pipe_share(uint32_t W, uint32_t rows, uint32_t j, uint32_t K)
{
    const uint32_t tiles = (uint32_t)((((uint64_t)W + 7u) / 8u) * (((uint64_t)rows + 7u) / 8u));
    if (K == 0u || j >= K || j >= tiles) return WfShare{0u, 0u, 0u};
    const uint32_t mine = (tiles - j + K - 1u) / K;
    const uint64_t pixels = (uint64_t)W * rows;
    return WfShare{mine, mine * 64u, (uint32_t)((uint64_t)mine * 64u < pixels ? (uint64_t)mine * 64u : pixels)};
}

/* Trace/shade iterations of a pipeline: each advances every live path by one traced segment; a path needs <=
 * samples*(maxBounce+1), or with the primary records reused (wf_shade: renders of more than one sample) maxBounce+1 for
 * sample 0 and maxBounce for each later sample. Bounded; WCPT documents the cap. */
constexpr uint32_t kWfMaxIters = 1u << 20;
constexpr uint32_t wf_iterations(int mode, uint32_t samples, uint32_t max_bounce)
{
    uint64_t iters = (uint64_t)samples * ((uint64_t)max_bounce + 1ull);
    if (mode == kModeRender && samples > 1u) iters = (uint64_t)max_bounce + 1ull + (uint64_t)(samples - 1u) * max_bounce;
    return iters > kWfMaxIters ? kWfMaxIters : (uint32_t)iters;
}

/* Shade blocks per CU (grid-stride over the queue). The continuing paths are appended in roughly the order
 * the blocks walk their chunks, so a small grid keeps the next queue close to the input order (coherent rays
 * for the next trace). Measured on c3: 4 -> 7.98 ms, 8 -> 8.13, 16 -> 8.56, 32 -> 8.98, one thread per slot ->
 * 8.97. */
#ifndef WCPT_SHADE_BLOCKS_PER_CU
#define WCPT_SHADE_BLOCKS_PER_CU 4
#endif

/* What launch_wavefront is asked. */
struct WfFrameInputs {
    WfVariant base;      /* wf_variant_select's */
    int mode;            /* kModeRender / Count / Diag */
    uint32_t W, rows;    /* the context's rows of the frame */
    uint32_t samples, max_bounce;
    int wf_fetch;        /* LaunchArgs::wf_fetch: -1 auto, 0 two rounds, 1 one */
    int wf_persist;      /* LaunchArgs::wf_persist: -1 auto, 0 off, 1 wherever eligible */
    int pipes;           /* WCPT_OPTION_WF_PIPES: below 1 by queue length */
    bool sort;           /* the ray sort as it runs: the option, and drawCommandCount > 0 */
    int overlap;         /* WCPT_OPTION_FRAME_OVERLAP as the runtime allows it for this render */
    int cus;             /* compute units of the device */
    int trace_bpc;       /* blocks per CU of the base variant (>= 1) */
    int persist_bpc;     /* ... of wf_persist_variant() (>= 1); read only where wf_persist_eligible */
};

struct WfPipePlan {
    uint32_t tiles, total, paths; /* wf_pipe_share */
    uint32_t init_grid;           /* wf_init's blocks */
    int geo;                      /* the GEO this pipeline traces: the base's, 3 for a short queue on the fast layout
                                     (wf_pipe_geo), WCPT_WF_PERSIST_GEO on the persistent trace */
    uint32_t iters;               /* trace/shade iterations (the per-bounce launches; the persistent trace is one launch) */
};
struct WfFramePlan {
    bool ok;               /* false: the frame's lanes or pixels do not fit 32 bits (hipErrorInvalidValue) */
    bool empty;            /* no pixels: success, nothing to launch */
    bool persist;          /* the pipelines run the persistent trace */
    uint32_t W, rows;      /* the frame the plan is of */
    uint32_t K;            /* pipelines */
    uint32_t trace_grid;   /* waves of one pipeline's wf_trace (the resident waves / K) */
    uint32_t shade_grid;   /* blocks of wf_shade */
    uint32_t persist_grid; /* waves of one pipeline's persistent trace, 0 without it */
    WfPipePlan pipe[kWfMaxPipes]; /* [0, K) */
};

/* the instance pipeline j launches */
constexpr WfVariant wf_pipe_variant(const WfFramePlan& p, const WfVariant& base, uint32_t j)
{
    return p.persist ? wf_persist_variant() : WfVariant{base.count, base.diag, p.pipe[j].geo, base.ldsn, false};
}

constexpr WfFramePlan wf_frame_plan(const WfFrameInputs& in)
{
    WfFramePlan p = {};
    p.W = in.W;
    p.rows = in.rows;
    const uint64_t pixels = (uint64_t)in.W * in.rows;
    if (pixels == 0u) {
        p.ok = p.empty = true;
        return p;
    }
    if (pixels > 0xFFFFFFFFull) return p; /* first, so that the tile product below cannot wrap */
    const uint64_t tiles64 = (((uint64_t)in.W + 7u) / 8u) * (((uint64_t)in.rows + 7u) / 8u);
    if (tiles64 * 64ull > 0xFFFFFFC0ull) return p;
    p.ok = true;
    const uint32_t tiles = (uint32_t)tiles64;
    const uint32_t trace_full = (uint32_t)(in.trace_bpc * in.cus);
    /* 0: one thread per path slot (no grid-stride loop) */
    p.shade_grid = WCPT_SHADE_BLOCKS_PER_CU > 0 ? (uint32_t)(in.cus * WCPT_SHADE_BLOCKS_PER_CU)
                                                : (uint32_t)((pixels + kWfShadeBlock - 1u) / kWfShadeBlock);
    /* the path-persistent trace (WCPT_OPTION_WF_PERSIST): one sample per pixel on the fast layout, and by default only
     * where the frame's paths about fit its resident lanes (row blocks): there the per-bounce
     * launches each last as long as their slowest ray, and one launch that lets each path run on lasts as long as its
     * slowest path (c3 135-row blocks 1.30 against 1.85 ms; the full c3 frame 6.64 against 4.55 ms,
     * profiles/r05_persist_ab.log) */
    const bool persist_ok = wf_persist_eligible(in.base, in.samples, in.sort, in.wf_persist);
    const uint32_t persist_full = persist_ok ? (uint32_t)(in.persist_bpc * in.cus) : 0u;
    /* at most 1.4 paths per resident lane: the lanes freed by the first paths take the rest (7- / 6-way c3 splits at
     * 1.13 / 1.32 paths per lane gain 7 % / 3 %, 5-way at 1.58 is flat, 4-way at 2.0 loses) */
    p.persist = persist_ok && (in.wf_persist > 0 || pixels * 5ull <= 64ull * 7ull * persist_full);
    /* pipelines: the option's count, or (0, the default) for the path-persistent trace one when each frame joins its
     * pipelines (its blocks measured 1.30 / 1.40 / 1.40 ms with 1 / 2 / 3) and two under the frame overlap, where a
     * pipeline's persistent launch runs on into its next frame (c3 8-way shares, slowest of 8, region-timed: 8-row
     * stripes 1.254 / 1.246 ms with one, 1.219 / 1.218 with two, 1.218 / 1.214 with three -- a third stream would sit
     * past the four hardware queues beside a group's communication stream; profiles/r06_c3_persist_pipes.log); else 3
     * when the frame holds at most 8 paths per resident trace lane -- the launches are short and their tails weigh, so
     * a third chain overlaps them (c3 4.41-4.46 against 4.50-4.55 ms with two) -- and 2 on longer queues (c4 199.5
     * against 197.9 ms with two; profiles/r05_pipes_ab.log).
     * This use of the threshold compares the whole frame's paths with the whole trace grid, before the division by K. */
    uint32_t K = (uint32_t)(in.pipes > kWfMaxPipes ? kWfMaxPipes : in.pipes);
    if (in.pipes < 1)
        K = p.persist ? (in.overlap != 0 && in.mode == kModeRender ? 2u : 1u) : (wf_short_queue(pixels, trace_full) ? 3u : 2u);
    if (in.sort || in.mode == kModeDiag) K = 1u; /* one sort scratch and one diagnostics block */
    if (K > tiles) K = tiles;
    p.K = K;
    /* each pipeline's persistent trace grid holds 1/K of the resident-wave slots, so the K traces run side by side
     * instead of the first one taking every slot and the others only filling its tail (c3 6.58 -> 6.16 ms with two
     * pipelines; 5/8 or 3/4 of the slots per pipeline measured equal, 7/16 slower) */
    p.trace_grid = trace_full / K > 0u ? trace_full / K : 1u;
    p.persist_grid = p.persist ? (persist_full / K > 0u ? persist_full / K : 1u) : 0u;
    const uint32_t iters = wf_iterations(in.mode, in.samples, in.max_bounce);
    for (uint32_t j = 0; j < K; j++) {
        const WfShare s = wf_pipe_share(in.W, in.rows, j, K);
        const uint32_t blocks = (uint32_t)(((uint64_t)s.total + kWfShadeBlock - 1u) / kWfShadeBlock);
        const uint32_t cap = (uint32_t)in.cus * 16u;
        p.pipe[j].tiles = s.tiles;
        p.pipe[j].total = s.total;
        p.pipe[j].paths = s.paths;
        p.pipe[j].init_grid = blocks < cap ? blocks : cap;
        p.pipe[j].geo = p.persist ? WCPT_WF_PERSIST_GEO : wf_pipe_geo(in.base, in.wf_fetch, s.paths, p.trace_grid);
        p.pipe[j].iters = iters;
    }
    return p;
}

/* Frame overlap (WCPT_OPTION_FRAME_OVERLAP; the megakernel's in pt_kernels.hip launch_megakernel): pipeline j
 * owns the tiles t % K == j, so while K and the frame's tiles stay, this render's pipelines need not wait for the
 * previous render's other pipelines -- each continues on its own stream, and the context's stream is joined to
 * them only when another entry point needs it (wf_join). On the per-bounce launches that recovers the frame's
 * ragged end (c3: its three pipelines end 0.3-0.5 ms apart, profiles/r06_c3_frame_timeline.log).
 * WfPending: the frames that pipelines 1..pipes-1 hold and the context's stream has not been joined to. */
struct WfPending {
    bool pending = false;
    uint32_t pipes = 0, W = 0, rows = 0;
    bool persist = false;
};
constexpr bool wf_frame_continues(const WfFramePlan& p, int mode, int overlap, const WfPending& q)
{
    return overlap != 0 && p.K > 1u && mode == kModeRender && q.pending && q.pipes == p.K && q.W == p.W &&
           q.rows == p.rows && q.persist == p.persist;
}

} // namespace wcpt

#endif
