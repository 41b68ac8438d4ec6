/*
 * wcpt_render.hip — C-ABI runtime, a frame: its preparation (the triangle records of every draw command, their table,
 * what the frame runs), the render dispatch with its counting and diagnostics runs, the primary-hit pass and the pick
 * (which share that preparation), the validation a group makes of all its ranks first, and the device self-tests.
 * render_common and everything it calls per frame are here.
 */
#include <algorithm>
#include <cstddef>

#include "primary_hit.h"
#include "wcpt_context.h"

using namespace wcpt::rt;

namespace {

/* ---- frame preparation: what it decides is stated in frame_prep.h; what it does to the device is below ---------------- */

/* One copy of a draw's primary-ray records (`copy` of the bytes at `dst`) brought to the camera position `origin` (bit
 * patterns) and the records build `build`, on the stream that owns the copy; nothing is queued when it is there. */
hipError_t bring_primary_copy(const TriRecords& t, TriRecords::PrimCopy& copy, void* dst, const uint32_t origin[3],
                              uint64_t build, hipStream_t stream)
{
    if (copy.valid && copy.build == build && std::memcmp(copy.origin, origin, sizeof(copy.origin)) == 0) return hipSuccess;
    float o[3];
    std::memcpy(o, origin, sizeof(o));
    const hipError_t e = wcpt::launch_build_primary_pairs(static_cast<const char*>(t.mem) + t.pair_offset,
                                                          (uint32_t)wcpt::record_layout(t.ntri).prim_pairs, o[0], o[1], o[2],
                                                          dst, stream);
    if (e != hipSuccess) return e;
    copy.valid = true;
    copy.build = build;
    std::memcpy(copy.origin, origin, sizeof(copy.origin));
    return hipSuccess;
}

/* Frame overlap, pipe 1 (pt_kernels.hip launch_megakernel): before its launch, on its own stream, the pipe-1 copy of
 * each draw's primary-ray records is derived again when it is not of the frame's camera position and records build.
 * Only pipe 1's stream ever writes that copy and the context's stream the other, so a moving camera needs no join. */
hipError_t prep_pipe1(void* user, hipStream_t stream)
{
    wcpt_context* ctx = static_cast<wcpt_context*>(user);
    for (TriRecords& t : ctx->tri) {
        if (!t.prim.valid || t.ntri == 0) continue;
        const hipError_t e = bring_primary_copy(t, t.prim1, t.pmem1(), t.prim.origin, t.prim.build, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

/* A frame's plan into its launch arguments and the context: the one exit of prepare_tri_records. With primary-ray
 * records pipe 1 reads a table of its own and derives its copy before its launch; else both pipes read the one table. */
void apply_plan(wcpt_context* ctx, const wcpt::FramePlan& p, uint32_t n, wcpt::LaunchArgs& a)
{
    a.pair_records = p.pair_records;
    a.wf_fast = p.wf_fast;
    a.tiny_tree = p.tiny_tree;
    a.triangles = p.triangles;
    ctx->kernel_run = p.kernel_run;
    const bool pipe1 = p.want_primary && n != 0;
    a.tri_records = n ? ctx->d_tri_table : nullptr;
    a.tri_records_pipe1 = pipe1 ? ctx->d_tri_table + (uint64_t)wcpt::kTriTableWords * ctx->tri_table_cap : nullptr;
    a.pipe1_prepare = pipe1 ? prep_pipe1 : nullptr;
    a.pipe1_user = pipe1 ? ctx : nullptr;
}

/* The frame's n draw commands into dc: from the host copy of their buffer when every byte of them was written through
 * wcpt_buffer_upload and the triangle cache is on (from_host); otherwise from the device, behind the pending frames (a
 * synchronous copy of 32 B per draw), so that draw commands written by other means (hipMemcpy, the application's own
 * kernels) are honoured with WCPT_OPTION_TRIANGLE_CACHE = 0. */
int read_draw_commands(wcpt_context* ctx, uint64_t draws, uint32_t n, std::vector<wcpt_draw_command>& dc, bool& from_host)
{
    const uint64_t dbytes = (uint64_t)n * sizeof(wcpt_draw_command);
    uint64_t off = 0;
    Buffer* db = buffer_at(ctx, draws, off);
    from_host = ctx->tri_cache && db && shadow_known(*db, off, dbytes);
    dc.resize(n);
    if (from_host) {
        std::memcpy(dc.data(), db->shadow.data() + off, dbytes);
        return WCPT_SUCCESS;
    }
    const int rc = join_pending(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dc.data(), reinterpret_cast<const void*>(draws), dbytes, hipMemcpyDeviceToHost, ctx->stream),
            "hipMemcpyAsync(draw commands)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(draw commands)");
    return WCPT_SUCCESS;
}

/* The argument checks of draw command d (frame_prep.h check_draw_args; bi: its index buffer at offset oi, or null when
 * the context does not know it), for the render and for render_validate alike. */
int check_draw(wcpt_context* ctx, uint32_t d, const wcpt_draw_command& c, const Buffer* bi, uint64_t oi)
{
    const uint64_t left = bi ? bi->bytes - oi : 0;
    switch (wcpt::check_draw_args(c.indexCount, c.vertexBuffer, c.indexBuffer, bi != nullptr, left)) {
    case wcpt::kDrawIndexCountPastBuffer:
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT,
                         "draw command %u: indexCount %u exceeds its index buffer (%llu bytes from offset %llu)", d,
                         c.indexCount, (unsigned long long)left, (unsigned long long)oi);
    case wcpt::kDrawNullBuffer:
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "draw command %u: null vertex/index buffer", d);
    default: return WCPT_SUCCESS;
    }
}

/* Word `word` of draw d in the host image of the table; true when that changed it. */
bool set_table_word(wcpt_context* ctx, uint32_t d, uint32_t word, uint64_t value)
{
    uint64_t& w = ctx->tri_table[(uint64_t)wcpt::kTriTableWords * d + word];
    if (w == value) return false;
    w = value;
    return true;
}

/* what the per-draw steps add up for frame_plan */
struct PrepSums { uint64_t tris_all = 0, leaves_all = 0, tris_max = 0; };

/* Draw d of a preparation miss: its argument checks, its triangle records (rebuilt unless the triangle cache holds
 * them), the leaf scan of its BVH (once per BVH buffer generation; the one step that blocks the host) and its table
 * words but the primary-ray records'. */
int prepare_draw(wcpt_context* ctx, uint32_t d, const wcpt_draw_command& c, PrepSums& sums, bool& table_dirty)
{
    TriRecords& t = ctx->tri[d];
    const uint64_t vb = c.vertexBuffer, ib = c.indexBuffer;
    uint64_t ov = 0, oi = 0, ob = 0;
    const Buffer* bv = buffer_at(ctx, vb, ov);
    const Buffer* bi = buffer_at(ctx, ib, oi);
    const Buffer* bb = buffer_at(ctx, c.bvhBuffer, ob);
    const int rc = check_draw(ctx, d, c, bi, oi);
    if (rc) return rc;
    const uint64_t gv = bv ? bv->generation : kUnknownGeneration;
    const uint64_t gi = bi ? bi->generation : kUnknownGeneration;
    const uint32_t ntri = c.indexCount / 3u;
    const uint32_t nvert = wcpt::vertex_bound(bv != nullptr, bv ? bv->bytes - ov : 0);
    const bool reuse = ctx->tri_cache && t.valid && t.vb == vb && t.ib == ib && t.ntri == ntri && t.gen_vb == gv &&
                       t.gen_ib == gi && gv != kUnknownGeneration && gi != kUnknownGeneration;
    if (!reuse) {
        const wcpt::RecordLayout l = wcpt::record_layout(ntri);
        if (t.cap < l.bytes) {
            const int grc = grow(ctx, t.mem, t.cap, l.bytes, l.bytes, "hipMalloc(triangle records)");
            if (grc) return grc;
        }
        t.pair_offset = l.pair_offset;
        HIP_TRY(ctx, wcpt::launch_build_tri_records(reinterpret_cast<const uint32_t*>(ib), reinterpret_cast<const float*>(vb),
                                                    ntri, nvert, t.mem, static_cast<char*>(t.mem) + l.pair_offset,
                                                    ctx->stream), "build_tri_records");
        t.vb = vb;
        t.ib = ib;
        t.gen_vb = gv;
        t.gen_ib = gi;
        t.ntri = ntri;
        t.valid = true;
        t.build_id++;
    }
    const uint64_t nodes = wcpt::bvh_node_count(bb != nullptr, bb ? bb->bytes - ob : 0);
    if (wcpt::draw_needs_scan(ctx->packed_refs, ctx->tri_cache != 0, nodes, c.indexCount) &&
        !(t.leaves_valid && t.bvh == c.bvhBuffer && t.gen_bvh == bb->generation && t.bvh_nodes == nodes && t.bvh_ntri == ntri)) {
        if (!ctx->d_scan) HIP_TRY(ctx, hipMalloc(&ctx->d_scan, sizeof(uint32_t)), "hipMalloc(leaf scan flag)");
        HIP_TRY(ctx, wcpt::launch_scan_leaf_counts(reinterpret_cast<const void*>(c.bvhBuffer), (uint32_t)nodes, ntri,
                                                   ctx->d_scan, ctx->stream), "scan_leaf_counts");
        uint32_t lf = wcpt::kLeafScanUnknown;
        HIP_TRY(ctx, hipMemcpyAsync(&lf, ctx->d_scan, sizeof(lf), hipMemcpyDeviceToHost, ctx->stream),
                "hipMemcpyAsync(leaf scan flag)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(leaf scan flag)");
        t.bvh = c.bvhBuffer;
        t.gen_bvh = bb->generation;
        t.bvh_nodes = nodes;
        t.bvh_ntri = ntri;
        t.leaf_flags = lf;
        t.leaves_valid = true;
    }
    const wcpt::DrawWords w = wcpt::draw_words(ctx->packed_refs, ctx->tri_cache != 0, nodes, c.indexCount, t.leaf_flags,
                                               ctx->mk_tiny_tree, nvert);
    const uint64_t addr = reinterpret_cast<uint64_t>(t.mem);
    table_dirty |= set_table_word(ctx, d, wcpt::kTriWordSingles, addr);
    table_dirty |= set_table_word(ctx, d, wcpt::kTriWordPairs, addr + t.pair_offset);
    table_dirty |= set_table_word(ctx, d, wcpt::kTriWordCount, w.word2);
    table_dirty |= set_table_word(ctx, d, wcpt::kTriWordFlags, w.flags);
    sums.tris_all += ntri;
    sums.tris_max = std::max<uint64_t>(sums.tris_max, ntri);
    sums.leaves_all += wcpt::leaf_estimate(bb != nullptr, bb ? bb->bytes : 0, ntri);
    return WCPT_SUCCESS;
}

/* Draw d's primary-ray records for the camera position `origin`, where the plan wants them: grown to the draw's pair
 * records, the context stream's copy derived (once per camera position and records build), table word kTriWordPrimary. */
int prepare_primary(wcpt_context* ctx, uint32_t d, bool want_primary, const uint32_t origin[3], bool& table_dirty)
{
    TriRecords& t = ctx->tri[d];
    uint64_t paddr = 0;
    if (want_primary && t.ntri > 0) {
        const uint64_t bytes = wcpt::record_layout(t.ntri).prim_bytes;
        if (t.pcap < bytes) {
            t.prim.valid = false;
            t.prim1.valid = false;
            const int rc = grow(ctx, t.pmem, t.pcap, bytes, 2 * bytes, "hipMalloc(primary-ray pair records)");
            if (rc) return rc;
        }
        HIP_TRY(ctx, bring_primary_copy(t, t.prim, t.pmem, origin, t.build_id, ctx->stream), "build_primary_pairs");
        paddr = reinterpret_cast<uint64_t>(t.pmem);
    }
    table_dirty |= set_table_word(ctx, d, wcpt::kTriWordPrimary, paddr);
    return WCPT_SUCCESS;
}

/* The host image of n draws' table to the device, grown to n draws: two tables, the second for pipe 1, which differs
 * only in kTriWordPrimary, pipe 1's copy of the primary-ray records. Blocks the host (the image is host memory). */
int upload_table(wcpt_context* ctx, uint32_t n, bool table_dirty)
{
    constexpr uint64_t W = wcpt::kTriTableWords;
    if (ctx->tri_table_cap < n) {
        const int rc = grow(ctx, ctx->d_tri_table, ctx->tri_table_cap, n, 2 * W * n * sizeof(uint64_t),
                            "hipMalloc(triangle record table)");
        if (rc) return rc;
        table_dirty = true;
    }
    if (!table_dirty) return WCPT_SUCCESS;
    const uint64_t second = W * ctx->tri_table_cap;
    std::vector<uint64_t> both(2 * second, 0);
    std::copy(ctx->tri_table.begin(), ctx->tri_table.begin() + W * n, both.begin());
    std::copy(ctx->tri_table.begin(), ctx->tri_table.begin() + W * n, both.begin() + second);
    for (uint32_t d = 0; d < n; d++)
        if (ctx->tri_table[W * d + wcpt::kTriWordPrimary])
            both[second + W * d + wcpt::kTriWordPrimary] = reinterpret_cast<uint64_t>(ctx->tri[d].pmem1());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tri_table, both.data(), both.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                                ctx->stream), "hipMemcpyAsync(triangle record table)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(triangle record table)");
    return WCPT_SUCCESS;
}

/* Derive (or reuse) the triangle records of every draw command, point a.tri_records at their table and choose what
 * the frame runs (frame_prep.h frame_plan). */
int prepare_tri_records(wcpt_context* ctx, const wcpt_scene_data& sd, uint64_t draws, wcpt::LaunchArgs& a)
{
    const uint32_t n = sd.drawCommandCount;
    if (n == 0) {
        apply_plan(ctx, wcpt::frame_plan(0, 0, 0, 0, 0, 0, ctx->pair_records, ctx->kernel), 0, a);
        return WCPT_SUCCESS;
    }
    uint32_t origin[3];
    std::memcpy(origin, sd.position, sizeof(origin));
    const bool handoff = ctx->handoff_valid && ctx->handoff_draws == draws && ctx->handoff.size() == n;
    ctx->handoff_valid = false;
    wcpt_context::PrepCache& pc = ctx->prep;
    if (!handoff && pc.valid && pc.gen == ctx->generation && pc.draws == draws && pc.n == n) {
        /* Only the camera moved (an editor drag, bench.py --camera orbit): the primary-ray records are derived again
         * for the new position -- the context stream's copy here, behind that stream's frames; pipe 1's copy on its own
         * stream before its launch (prep_pipe1) -- and nothing else changes, so the frame overlap goes on. */
        if (std::memcmp(pc.origin, origin, sizeof(origin)) != 0) {
            if (pc.plan.want_primary) {
                for (uint32_t d = 0; d < n; d++) {
                    TriRecords& t = ctx->tri[d];
                    if (!t.prim.valid || t.ntri == 0) continue;
                    HIP_TRY(ctx, bring_primary_copy(t, t.prim, t.pmem, origin, t.build_id, ctx->stream), "build_primary_pairs");
                }
            }
            std::memcpy(pc.origin, origin, sizeof(origin));
        }
        apply_plan(ctx, pc.plan, n, a);
        ctx->prep_missed = false;
        return WCPT_SUCCESS;
    }
    pc.valid = false;
    /* the preparation below may rebuild records that pending frames read, and queues its work on the stream; the
     * frame that follows runs on the stream itself (render_common): a camera that moves every frame rebuilds the
     * primary-ray records every frame, and a fork and a join per frame would cost more than the overlap returns */
    ctx->prep_missed = true;
    int rc = join_pending(ctx);
    if (rc) return rc;
    std::vector<wcpt_draw_command> dc;
    bool from_host = false; /* a frame handed over by render_validate was read from the device: never cached */
    if (handoff) {
        dc.swap(ctx->handoff);
    } else {
        rc = read_draw_commands(ctx, draws, n, dc, from_host);
        if (rc) return rc;
    }
    if (ctx->tri.size() < n) ctx->tri.resize(n);
    bool table_dirty = ctx->tri_table.size() < (uint64_t)wcpt::kTriTableWords * n;
    if (table_dirty) ctx->tri_table.resize((uint64_t)wcpt::kTriTableWords * n, 0);
    PrepSums sums;
    for (uint32_t d = 0; d < n; d++) {
        rc = prepare_draw(ctx, d, dc[d], sums, table_dirty);
        if (rc) return rc;
    }
    const wcpt::FramePlan plan =
        wcpt::frame_plan(n, ctx->tri_table[wcpt::kTriWordCount], ctx->tri_table[wcpt::kTriWordFlags], sums.tris_all,
                         sums.leaves_all, sums.tris_max, ctx->pair_records, ctx->kernel);
    for (uint32_t d = 0; d < n; d++) {
        rc = prepare_primary(ctx, d, plan.want_primary, origin, table_dirty);
        if (rc) return rc;
    }
    rc = upload_table(ctx, n, table_dirty);
    if (rc) return rc;
    apply_plan(ctx, plan, n, a);
    if (from_host) pc = {true, ctx->generation, draws, n, {origin[0], origin[1], origin[2]}, plan};
    return WCPT_SUCCESS;
}

/* The argument checks of wcpt_render that need no device work (render_common, wcpt::render_validate). */
int check_render_args(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
                      uint64_t draws, int mode)
{
    if (!scene) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: null SceneData");
    if (!ctx->image || ctx->layout.width == 0 || ctx->layout.rows == 0)
        return set_error(ctx, WCPT_ERROR_NO_SCREEN, "wcpt_render: no output image (call wcpt_create_screen)");
    if (!wcpt::layout_renderable(ctx->layout))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT,
                         "wcpt_render: the context's %u rows of width %u cover %llu 8x8 tiles, more than 2^26 - 1 "
                         "(name fewer rows with wcpt_set_row_range or wcpt_set_row_stripes)", ctx->layout.rows,
                         ctx->layout.width, (unsigned long long)wcpt::layout_tiles(ctx->layout));
    if (scene->sphereCount > 0 && spheres == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: sphereCount > 0 with a null sphere buffer");
    if (scene->drawCommandCount > 0 && draws == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: drawCommandCount > 0 with null draw commands");
    if (materials == 0 && (scene->sphereCount > 0 || scene->drawCommandCount > 0))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: null material buffer");
    /* the output's rows: the context's rows back to back, or (WCPT_OPTION_GATHER_FRAME_ROWS) frame rows up to its last */
    const uint64_t wire_rows = ctx->gather_frame_rows ? wcpt::layout_last_row(ctx->layout) + 1u : ctx->layout.rows;
    if (ctx->wire && mode == wcpt::kModeRender &&
        (uint64_t)ctx->layout.width * wire_rows * wcpt::payload_pixel_bytes(ctx->wire_ch) > ctx->wire_bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "gather output of %llu bytes too small for %ux%llu x %u B",
                         (unsigned long long)ctx->wire_bytes, ctx->layout.width, (unsigned long long)wire_rows,
                         (unsigned)wcpt::payload_pixel_bytes(ctx->wire_ch));
    return WCPT_SUCCESS;
}

/* Profiling events time the launches only: no system-scope fence when they are recorded (hip_runtime_api.h,
 * hipEventDisableSystemFence), so the timed frames pay no cache writeback between launches (c2 0.538 -> 0.534
 * ms/frame against hipEventReleaseToDevice and hipEventDefault, which measured alike). */
#ifndef WCPT_PROFILE_EVENT_FLAGS
#define WCPT_PROFILE_EVENT_FLAGS hipEventDisableSystemFence
#endif

/* Region timing (WCPT_OPTION_PROFILE_REGION) of a render or a primary-hit pass about to be queued: one event before the
 * first launch since wcpt_profile_begin; wcpt_profile_end records the closing one. */
int region_launch(wcpt_context* ctx)
{
    if (ctx->events.empty()) {
        hipEvent_t b, c;
        HIP_TRY(ctx, hipEventCreateWithFlags(&b, WCPT_PROFILE_EVENT_FLAGS), "hipEventCreate");
        HIP_TRY(ctx, hipEventCreateWithFlags(&c, WCPT_PROFILE_EVENT_FLAGS), "hipEventCreate");
        ctx->events.emplace_back(b, c);
    }
    if (ctx->region_renders++ == 0) {
        HIP_TRY(ctx, hipEventRecord(ctx->events[0].first, ctx->stream), "hipEventRecord");
        ctx->events_used = 1;
    }
    return WCPT_SUCCESS;
}

int render_common(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
                  uint64_t draws, int mode)
{
    int rc = bind_device(ctx);
    if (rc) return rc;
    /* frame overlap (WCPT_OPTION_FRAME_OVERLAP, pt_kernels.hip launch_megakernel): renders only, on the context's own
     * stream (work the application queues on a stream of its own could not be ordered behind the pipes), and not
     * under per-render timing events (they bracket each frame on the stream) */
    int overlap = (mode == wcpt::kModeRender && ctx->stream == ctx->own_stream && !ctx->overlap_suppressed &&
                   !(ctx->profiling && !ctx->profile_region)) ? ctx->frame_overlap : 0;
    if (!overlap) {
        rc = join_pending(ctx);
        if (rc) return rc;
    }
    rc = check_render_args(ctx, scene, materials, spheres, draws, mode);
    if (rc) return rc;
    wcpt::LaunchArgs a;
    a.sd = *scene;
    a.materials = reinterpret_cast<const wcpt_material*>(materials);
    a.spheres = reinterpret_cast<const wcpt_sphere*>(spheres);
    a.draws = reinterpret_cast<const wcpt_draw_command*>(draws);
    a.image = ctx->image;
    a.wire = nullptr;
    a.wire_ch = ctx->wire_ch;
    if (ctx->wire && mode == wcpt::kModeRender) a.wire = ctx->wire;
    a.W = ctx->layout.width;
    a.H = ctx->layout.height;
    a.y0 = ctx->layout.y0;
    a.rows = ctx->layout.rows;
    {
        const wcpt::RowMap m = wcpt::layout_row_map(ctx->layout);
        a.row_shift = m.shift;
        a.row_gap = m.gap;
        a.wire_rows = ctx->gather_frame_rows ? m : wcpt::RowMap{0u, wcpt::kContiguousShift, 0u};
    }
    a.status = ctx->d_status;
    a.counters = ctx->d_counters;
    a.tri_records = nullptr;
    a.pair_records = false;
    a.wf_fast = false;
    a.wf_refill = (uint32_t)ctx->wf_refill;
    a.wf_refill_persist = (uint32_t)ctx->wf_refill_persist;
    a.wf_fetch = ctx->wf_fetch;
    a.wf_persist = ctx->wf_persist;
    a.mk_tile_order = (uint32_t)ctx->mk_tile_order;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->profiling && mode == wcpt::kModeRender && ctx->profile_region) {
        rc = region_launch(ctx);
        if (rc) return rc;
    } else if (ctx->profiling && mode == wcpt::kModeRender) {
        if (ctx->events_used == ctx->events.size()) {
            hipEvent_t b, c;
            HIP_TRY(ctx, hipEventCreateWithFlags(&b, WCPT_PROFILE_EVENT_FLAGS), "hipEventCreate");
            HIP_TRY(ctx, hipEventCreateWithFlags(&c, WCPT_PROFILE_EVENT_FLAGS), "hipEventCreate");
            ctx->events.emplace_back(b, c);
        }
        e0 = ctx->events[ctx->events_used].first;
        e1 = ctx->events[ctx->events_used].second;
        ctx->events_used++;
        HIP_TRY(ctx, hipEventRecord(e0, ctx->stream), "hipEventRecord");
    }
    ctx->prep_missed = false;
    rc = prepare_tri_records(ctx, *scene, draws, a);
    if (rc) return rc;
    if (ctx->prep_missed) overlap = 0;
    /* WCPT_OPTION_ARITH: only the megakernel's render instances have fast twins; the wavefront kernels (also as
     * WCPT_KERNEL_AUTO's choice), the counting and the diagnostics runs are exact */
    a.arith = (mode == wcpt::kModeRender && ctx->kernel_run == WCPT_KERNEL_MEGAKERNEL) ? ctx->arith : WCPT_ARITH_EXACT;
    ctx->arith_run = a.arith;
    a.mk_split = ctx->mk_split;
    /* the other kernel's pending frames (the same image) first */
    if (ctx->kernel_run != WCPT_KERNEL_MEGAKERNEL && ctx->mk.pending)
        HIP_TRY(ctx, wcpt::mk_join(ctx->mk, ctx->stream), "frame overlap join");
    if (ctx->kernel_run != WCPT_KERNEL_WAVEFRONT && ctx->wf.pending)
        HIP_TRY(ctx, wcpt::wf_join(ctx->wf, ctx->stream), "frame overlap join (wavefront)");
#if WCPT_MK_TIMERS
    /* tools-only build: the render's megakernel adds its phase timers to the counters (wcpt_read_diagnostics) */
    rc = join_pending(ctx);
    if (rc) return rc;
    if (mode == wcpt::kModeRender && ctx->kernel_run == WCPT_KERNEL_MEGAKERNEL)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, kNumCounters * sizeof(unsigned long long), ctx->stream),
                "hipMemsetAsync(timers)");
#endif
    hipError_t e = hipSuccess;
    /* primary cache (primary_cache_key.h): the key of this render; launch_megakernel applies the rule. Under the
     * triangle cache's promise only -- scene buffers change through wcpt_buffer_upload (which bumps the generation) or
     * the application restarts accumulation at frame 0 -- so never with WCPT_OPTION_TRIANGLE_CACHE = 0. */
    wcpt::PrimaryCacheKey pkey;
    if (mode == wcpt::kModeRender && ctx->prim_cache && ctx->tri_cache) {
        pkey = wcpt::primary_cache_key(*scene, a.W, a.H, a.y0, a.rows, a.row_shift, a.row_gap, spheres, draws,
                                       reinterpret_cast<uint64_t>(a.tri_records), a.pair_records, ctx->generation);
        a.prim_key = &pkey;
    }
    switch (ctx->kernel_run) {
    case WCPT_KERNEL_MEGAKERNEL: e = wcpt::launch_megakernel(a, mode, ctx->stack_kind, ctx->mk, ctx->stream, overlap); break;
    case WCPT_KERNEL_WAVEFRONT:
        if (mode == wcpt::kModeRender) ctx->mk.prim_valid = false; /* a frame the megakernel did not render */
        e = wcpt::launch_wavefront(a, mode, ctx->wf, ctx->wf_pipes, ctx->sort_rays != 0, ctx->wf_stack, ctx->stream, overlap);
        break;
    default: return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "kernel variant %d not available", ctx->kernel_run);
    }
    if (e != hipSuccess) return hip_fail(ctx, e, "kernel launch");
    if (e1) HIP_TRY(ctx, hipEventRecord(e1, ctx->stream), "hipEventRecord");
    return WCPT_SUCCESS;
}

/* the self-tests' scratch (their inputs, then their outputs) and the pick's one record */
int ensure_scratch(wcpt_context* ctx, uint64_t bytes)
{
    if (ctx->scratch_bytes >= bytes) return WCPT_SUCCESS;
    return grow(ctx, ctx->d_scratch, ctx->scratch_bytes, bytes, bytes, "hipMalloc(selftest scratch)");
}

/* ---- the primary-hit pass (pt_primary.hip, primary_hit.h) -------------------------------------------------------------- */

/* What wcpt_trace_primary and wcpt_pick (`who`) refuse about the scene and the screen before any device work: a render's
 * checks without the material buffer and the gather output. */
int check_primary_args(wcpt_context* ctx, const char* who, const wcpt_scene_data* scene, uint64_t spheres, uint64_t draws)
{
    if (!scene) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s: null SceneData", who);
    if (ctx->layout.width == 0 || ctx->layout.height == 0 || ctx->layout.rows == 0)
        return set_error(ctx, WCPT_ERROR_NO_SCREEN, "%s: no screen (call wcpt_create_screen)", who);
    if (!wcpt::layout_renderable(ctx->layout))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s: the context's %u rows of width %u cover %llu 8x8 tiles, more "
                         "than 2^26 - 1", who, ctx->layout.rows, ctx->layout.width,
                         (unsigned long long)wcpt::layout_tiles(ctx->layout));
    if (scene->sphereCount > 0 && spheres == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s: sphereCount > 0 with a null sphere buffer", who);
    if (scene->drawCommandCount > 0 && draws == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s: drawCommandCount > 0 with null draw commands", who);
    return WCPT_SUCCESS;
}

/* The pass over one window (PrimaryPass: x0, width, rows, rm, dst), behind both frame-overlap pipes and a render's frame
 * preparation, which it shares: a prepared scene is not prepared again and the next render's preparation still hits. The
 * plan the preparation makes is a render's business: what the last render ran (wcpt_last_kernel) stays. `timed`: the pass
 * counts in a profiled region (WCPT_OPTION_PROFILE_REGION). */
int primary_pass(wcpt_context* ctx, const wcpt_scene_data& scene, uint64_t spheres, uint64_t draws, wcpt::PrimaryPass& p,
                 bool timed)
{
    int rc = join_pending(ctx);
    if (rc) return rc;
    wcpt::LaunchArgs a;
    a.tri_records = nullptr;
    const int kernel_run = ctx->kernel_run;
    rc = prepare_tri_records(ctx, scene, draws, a);
    ctx->kernel_run = kernel_run;
    if (rc) return rc;
    p.sd = scene;
    p.spheres = reinterpret_cast<const wcpt_sphere*>(spheres);
    p.draws = reinterpret_cast<const wcpt_draw_command*>(draws);
    p.tri_records = a.tri_records;
    p.pair_records = a.pair_records;
    p.W = ctx->layout.width;
    p.H = ctx->layout.height;
    p.status = ctx->d_status;
    /* region timing counts the pass once nothing can refuse it any more: a pass the preparation refused was no launch */
    if (timed && ctx->profiling && ctx->profile_region) {
        rc = region_launch(ctx);
        if (rc) return rc;
    }
    HIP_TRY(ctx, wcpt::launch_primary(p, ctx->stream), "primary-hit launch");
    return WCPT_SUCCESS;
}

} // namespace

/* Every check wcpt_render would make before it launches anything, with no launch: the argument checks and, per draw
 * command, the checks of the record build (check_draw). A group validates all its ranks first, so
 * that an argument error cannot leave some ranks a frame ahead of the others. */
int wcpt::render_validate(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
                          uint64_t draws)
{
    int rc = bind_device(ctx); /* a validation that reads nothing from the device leaves pending frames running */
    if (rc) return rc;
    rc = check_render_args(ctx, scene, materials, spheres, draws, kModeRender);
    if (rc) return rc;
    const uint32_t n = scene->drawCommandCount;
    ctx->handoff_valid = false;
    if (n == 0) return WCPT_SUCCESS;
    wcpt_context::ValidCache& vc = ctx->validated;
    if (vc.valid && vc.gen == ctx->generation && vc.draws == draws && vc.n == n) return WCPT_SUCCESS;
    vc.valid = false;
    /* draw commands read from the device (the application may write them behind the runtime) are handed to the render
     * that follows (prepare_tri_records), so a frame reads them once */
    std::vector<wcpt_draw_command>& dc = ctx->handoff;
    bool from_host = false;
    rc = read_draw_commands(ctx, draws, n, dc, from_host);
    if (rc) return rc;
    for (uint32_t d = 0; d < n; d++) {
        uint64_t oi = 0;
        const Buffer* bi = buffer_at(ctx, dc[d].indexBuffer, oi);
        rc = check_draw(ctx, d, dc[d], bi, oi);
        if (rc) return rc;
    }
    if (from_host) {
        vc.valid = true;
        vc.gen = ctx->generation;
        vc.draws = draws;
        vc.n = n;
    } else {
        ctx->handoff_draws = draws;
        ctx->handoff_valid = true;
    }
    return WCPT_SUCCESS;
}

/* A validated frame that will not be rendered (another rank's validation failed): drop its hand-off. */
void wcpt::render_abandon(wcpt_context* ctx)
{
    if (ctx) ctx->handoff_valid = false;
}

extern "C" {

/* ---- dispatch ------------------------------------------------------------------------------------ */
int wcpt_render(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
                uint64_t draw_commands)
{
    return render_common(ctx, scene, materials, spheres, draw_commands, wcpt::kModeRender);
}

int wcpt_render_counters(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
                         uint64_t draw_commands, wcpt_counters* out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null counters");
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, kNumCounters * sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
    rc = render_common(ctx, scene, materials, spheres, draw_commands,
                       ctx->diagnostics ? wcpt::kModeDiag : wcpt::kModeCount);
    if (rc) return rc;
    unsigned long long h[kNumCounters];
    HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_counters, sizeof(h), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    /* the device's counters are wcpt_counters' fields in their order, but for the deepest stack's "too deep to track" */
    static_assert(sizeof(wcpt_counters) == sizeof(h) && offsetof(wcpt_counters, ref_stack_max) == 15 * sizeof(uint64_t),
                  "wcpt_counters: kNumCounters fields of 64 bits");
    std::memcpy(out, h, sizeof(h));
    if (h[15] == 0xFFFFFFFFull) out->ref_stack_max = UINT64_MAX;
    return read_status(ctx);
}

/* ---- the primary-hit buffer and the pick ---------------------------------------------------------- */
int wcpt_trace_primary(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t spheres, uint64_t draw_commands,
                       uint64_t dst, uint64_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = check_primary_args(ctx, "wcpt_trace_primary", scene, spheres, draw_commands);
    if (rc) return rc;
    const uint64_t need = wcpt::primary_hit_bytes(ctx->layout.width, ctx->layout.rows);
    if (dst == 0 || dst % 16u != 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_trace_primary: output address 0x%llx (16-byte aligned, not null)",
                         (unsigned long long)dst);
    if (bytes < need)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_trace_primary: output of %llu bytes too small for %ux%u x %u B",
                         (unsigned long long)bytes, ctx->layout.width, ctx->layout.rows, wcpt::kPrimHitBytes);
    wcpt::PrimaryPass p;
    p.dst = reinterpret_cast<void*>(dst);
    p.x0 = 0;
    p.width = ctx->layout.width;
    p.rows = ctx->layout.rows;
    p.rm = wcpt::layout_row_map(ctx->layout);
    return primary_pass(ctx, *scene, spheres, draw_commands, p, true);
}

int wcpt_pick(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t spheres, uint64_t draw_commands, uint32_t x,
              uint32_t y, wcpt_primary_hit* out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = check_primary_args(ctx, "wcpt_pick", scene, spheres, draw_commands);
    if (rc) return rc;
    if (!out) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_pick: null output");
    if (x >= ctx->layout.width || y >= ctx->layout.height)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_pick: pixel (%u, %u) outside the %ux%u frame", x, y,
                         ctx->layout.width, ctx->layout.height);
    rc = ensure_scratch(ctx, wcpt::kPrimHitBytes);
    if (rc) return rc;
    /* the one-pixel window at (x, y): a block of one row from frame row y, whichever rows the context holds */
    wcpt::PrimaryPass p;
    p.dst = ctx->d_scratch;
    p.x0 = x;
    p.width = 1;
    p.rows = 1;
    p.rm = wcpt::RowMap{y, wcpt::kContiguousShift, 0u};
    rc = primary_pass(ctx, *scene, spheres, draw_commands, p, false); /* a pick is not a timed pass */
    if (rc) return rc;
    static_assert(sizeof(wcpt_primary_hit) == wcpt::kPrimHitBytes, "wcpt_primary_hit is primary_hit.h's record");
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_scratch, sizeof(*out), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(pick)");
    return read_status(ctx); /* synchronises: *out is filled */
}

int wcpt_read_diagnostics(wcpt_context* ctx, uint64_t* out, uint32_t n)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out || n > 8) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_read_diagnostics: bad output");
    memset(out, 0, sizeof(uint64_t) * n);
#if WCPT_MK_TIMERS
    if (ctx->kernel_run == WCPT_KERNEL_MEGAKERNEL && n) { /* megakernel phase timers of the last render */
        HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_counters, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, ctx->stream),
                "hipMemcpyAsync(timers)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        return WCPT_SUCCESS;
    }
#endif
    if (!ctx->wf.pipe[0].diag || n == 0) return WCPT_SUCCESS;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->wf.pipe[0].diag, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, ctx->stream),
            "hipMemcpyAsync(diag)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return WCPT_SUCCESS;
}

/* ---- self-test -------------------------------------------------------------------------------------- */
int wcpt_selftest_device(wcpt_context* ctx, int fn, const uint32_t* in, const uint32_t* in2, uint32_t* out, uint32_t n)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!in || !out || ((fn == 6 || fn == 14 || fn == 16 || fn == 17) && !in2))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null selftest arrays");
    if (fn < 0 || fn > 22) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "unknown selftest fn %d", fn);
    const uint64_t outw = (fn == 1) ? 4ull * n : ((fn == 7 || fn == 22) ? 3ull * n : (uint64_t)n);
    rc = ensure_scratch(ctx, (2ull * n + outw) * 4ull + 16);
    if (rc) return rc;
    uint32_t* d_in = ctx->d_scratch;
    uint32_t* d_in2 = d_in + n;
    uint32_t* d_out = d_in2 + n;
    HIP_TRY(ctx, hipMemcpyAsync(d_in, in, 4ull * n, hipMemcpyHostToDevice, ctx->stream), "selftest upload");
    if (in2) HIP_TRY(ctx, hipMemcpyAsync(d_in2, in2, 4ull * n, hipMemcpyHostToDevice, ctx->stream), "selftest upload");
    HIP_TRY(ctx, wcpt::launch_selftest(fn, d_in, d_in2, d_out, n, ctx->stream), "selftest launch");
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, 4ull * outw, hipMemcpyDeviceToHost, ctx->stream), "selftest download");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return WCPT_SUCCESS;
}

int wcpt_selftest_geometry(wcpt_context* ctx, int fn, int arith, const uint32_t* in, uint32_t in_words, uint32_t* out,
                           uint32_t out_words, uint32_t n)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!in || !out) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null selftest arrays");
    if (arith != WCPT_ARITH_EXACT && arith != WCPT_ARITH_FAST)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "unknown arithmetic mode %d", arith);
    uint32_t iw = 0, ow = 0;
    if (!wcpt::selftest_geometry_words(fn, iw, ow))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "unknown geometry selftest fn %d", fn);
    if (in_words != iw || out_words != ow)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "geometry selftest fn %d takes %u words and gives %u per item", fn,
                         iw, ow);
    const uint64_t inw = (uint64_t)n * iw, outw = (uint64_t)n * ow;
    rc = ensure_scratch(ctx, (inw + outw) * 4ull + 16);
    if (rc) return rc;
    uint32_t* d_in = ctx->d_scratch;
    uint32_t* d_out = d_in + inw;
    HIP_TRY(ctx, hipMemcpyAsync(d_in, in, 4ull * inw, hipMemcpyHostToDevice, ctx->stream), "selftest upload");
    HIP_TRY(ctx, wcpt::launch_selftest_geometry(fn, arith, d_in, iw, d_out, ow, n, ctx->stream), "selftest launch");
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, 4ull * outw, hipMemcpyDeviceToHost, ctx->stream), "selftest download");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return WCPT_SUCCESS;
}

} /* extern "C" */
