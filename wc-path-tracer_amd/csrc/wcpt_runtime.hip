/*
 * wcpt_runtime.hip — C-ABI runtime: device context, device buffers, output image, dispatch, timing.
 *
 * Replaces the Vulkan plumbing of the reference's renderer host (src/PathTracingRenderer.jai,
 * src/BufferManager.jai, modules/VKUtils/{Buffer,Synchronization}.jai); see include/wcpt.h for the
 * line-by-line mapping. HIP device memory replaces VMA GPU-only buffers; a device pointer IS the buffer
 * device address (VK_KHR_buffer_device_address, pathTracer.comp:74-95).
 */
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/wcpt.h"
#include "pt_kernels.h"
#include "wcpt_bloom.h"
#include "bvh_midpoint.h"

namespace {

constexpr int kNumCounters = 16; /* wcpt_counters: 8 reference counters + 6 diagnostics + 2 reference-stack fields */
std::mutex g_err_mutex;
std::string g_last_error;

/* Device buffers are handed out at base address = 32 (mod 64) (a 64-byte-aligned allocation + 32). A BVH
 * node is 32 bytes and the two children of an interior node sit at indices (2k+1, 2k+2) (the builder appends
 * them as a pair after the root, PathTracingRenderer.jai:196-202), so with this base every child pair the
 * traversal fetches together occupies exactly one 64-byte cache line instead of straddling two. Scattered
 * line visits are what bounds traversal (tools/gather_bench.hip). 32-byte alignment is enough for every
 * other buffer type (largest access: 16 bytes). */
constexpr uint64_t kBufferSkew = 32;

struct Buffer {
    void* raw = nullptr;   /* hipMalloc result */
    void* ptr = nullptr;   /* raw + kBufferSkew: the device address handed out */
    uint64_t bytes = 0;
    uint64_t generation = 0;      /* context-wide counter value of the last alloc / upload / grow */
    std::vector<uint8_t> shadow;  /* host copy of the uploaded contents (buffers <= kShadowMax bytes) */
    std::vector<uint8_t> known;   /* per kShadowChunk bytes: 1 when `shadow` holds what wcpt_buffer_upload wrote */
};

/* Small buffers (draw commands, materials, spheres) keep a host copy of what was uploaded, so that the render
 * call can read the draw commands without a device round trip. */
constexpr uint64_t kShadowMax = 1ull << 20;
/* Granularity of the host copy's validity map. hipMalloc contents are undefined, so a byte range of the host copy is
 * trusted only where wcpt_buffer_upload wrote it; any other range is read from the device. */
constexpr uint64_t kShadowChunk = 32;

/* Mark the chunks of [offset, end) that the upload covers entirely as known (partially covered chunks keep their
 * state: the host copy is updated byte-exactly either way). */
void shadow_mark(Buffer& b, uint64_t offset, uint64_t end)
{
    if (b.known.empty()) return;
    const uint64_t c0 = (offset + kShadowChunk - 1) / kShadowChunk, c1 = end / kShadowChunk;
    for (uint64_t c = c0; c < c1 && c < b.known.size(); c++) b.known[c] = 1;
}

/* The chunks that [offset, end) touches no longer hold what the device holds (a kernel wrote the range). */
void shadow_forget(Buffer& b, uint64_t offset, uint64_t end)
{
    for (uint64_t c = offset / kShadowChunk; c < (end + kShadowChunk - 1) / kShadowChunk && c < b.known.size(); c++) b.known[c] = 0;
}

/* True when the host copy holds every byte of [offset, offset + bytes). */
bool shadow_known(const Buffer& b, uint64_t offset, uint64_t bytes)
{
    if (b.shadow.size() != b.bytes || bytes == 0 || offset + bytes > b.bytes) return false;
    for (uint64_t c = offset / kShadowChunk; c < (offset + bytes + kShadowChunk - 1) / kShadowChunk; c++)
        if (c >= b.known.size() || !b.known[c]) return false;
    return true;
}

/* Derived triangle records of one draw command (pt_device.h): rebuilt when the draw's vertex/index buffers,
 * their generations or its index count change (or on every render with WCPT_OPTION_TRIANGLE_CACHE = 0). */
constexpr uint64_t kUnknownGeneration = ~0ull;
struct TriRecords {
    uint64_t vb = 0, ib = 0, gen_vb = kUnknownGeneration, gen_ib = kUnknownGeneration;
    uint32_t ntri = 0;
    bool valid = false;
    void* mem = nullptr;    /* single records, then pair records */
    uint64_t cap = 0;
    uint64_t pair_offset = 0;
    uint64_t build_id = 0;  /* incremented on every rebuild of the records */
    /* whether every node of the draw's BVH (address bvh, `bvh_nodes` nodes, buffer generation gen_bvh) has
     * triangleCount < 255 (frame_prep.h kTriFlagSmallLeaves) */
    uint64_t bvh = 0, gen_bvh = kUnknownGeneration;
    uint64_t bvh_nodes = 0;
    uint32_t bvh_ntri = 0;
    uint32_t leaf_flags = 0;   /* launch_scan_leaf_counts: frame_prep.h kLeafScan* */
    bool leaves_valid = false;
    /* primary-ray pair records (pt_device.h TriPairP): two copies of pcap bytes in pmem, the context stream's (state
     * `prim`), then the overlap's pipe 1's (pmem1, state `prim1`). Pipe 1's copy is rebuilt on pipe 1's stream only, so
     * neither copy is ever written while the other stream's frames read it (prep_pipe1). */
    void* pmem = nullptr;
    uint64_t pcap = 0;
    struct PrimCopy {
        bool valid = false;
        uint32_t origin[3] = {0, 0, 0}; /* the camera position the copy is derived for (bit patterns) */
        uint64_t build = 0;             /* ... from the pair records of this build_id */
    } prim, prim1;
    void* pmem1() const { return pmem ? static_cast<char*>(pmem) + pcap : nullptr; }
};

/* Bytes per pixel of a gather payload format (wcpt.h WCPT_PAYLOAD_*) */
uint64_t payload_pixel_bytes(uint32_t format) { return format == WCPT_PAYLOAD_DISPLAY_RGBA8 ? 4u : 4ull * format; }

hipError_t skewed_alloc(Buffer& b, uint64_t bytes)
{
    b.raw = nullptr;
    b.ptr = nullptr;
    b.bytes = bytes;
    if (!bytes) return hipSuccess;
    hipError_t e = hipMalloc(&b.raw, bytes + 2 * kBufferSkew);
    if (e != hipSuccess) return e;
    b.ptr = static_cast<char*>(b.raw) + kBufferSkew;
    return hipSuccess;
}

} // namespace

struct wcpt_context {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::unordered_map<uint64_t, Buffer> buffers;
    uint64_t next_handle = 1;
    float4* image = nullptr;           /* the image kernels write: own_image or an external buffer */
    float4* own_image = nullptr;
    uint64_t image_bytes_cap = 0;
    uint64_t external_bytes = 0;       /* != 0 while an external image is attached */
    float* wire = nullptr;             /* wcpt_set_gather_output */
    uint64_t wire_bytes = 0;
    uint32_t wire_ch = 3;
    uint32_t width = 0, height = 0, y0 = 0, rows = 0; /* rows == height when not sharded */
    uint32_t stripe = 0, period = 0;   /* wcpt_set_row_stripes (0: a contiguous block [y0, y0 + rows)) */
    bool sharded = false;
    int gather_frame_rows = 0;         /* WCPT_OPTION_GATHER_FRAME_ROWS */
    uint32_t* d_status = nullptr;
    unsigned long long* d_counters = nullptr;
    wcpt::WfPipes wf;                  /* path state + streams of the wavefront pipelines (allocated on first use) */
    wcpt::MkState mk;                  /* megakernel launch state (CU count, cost-ordered tiles) */
    uint32_t* d_scratch = nullptr;
    uint32_t* d_scan = nullptr;        /* leaf-count scan flag (prepare_tri_records) */
    float4* d_bloom = nullptr;         /* wcpt_composite_bloom: the down pyramid, then the up pyramid (on first use) */
    uint64_t bloom_bytes = 0;
    void* d_bvh = nullptr;             /* wcpt_bvh_build_device: its scratch (on first use, grown on demand) */
    uint64_t bvh_bytes = 0;
    uint64_t scratch_bytes = 0;
    int kernel = WCPT_KERNEL_MEGAKERNEL;
    int kernel_run = WCPT_KERNEL_MEGAKERNEL; /* the variant the current/last render runs (WCPT_KERNEL_AUTO resolved) */
    int arith = WCPT_ARITH_EXACT;      /* WCPT_OPTION_ARITH: a permission for megakernel render launches */
    int arith_run = WCPT_ARITH_EXACT;  /* the arithmetic the current/last render runs (wcpt_last_arith) */
    int stack_kind = 1;                /* WCPT_OPTION_STACK: 0 scratch, 1 LDS + spill (default; c2 -2%, 135-row blocks -8%) */
    int diagnostics = 0;               /* WCPT_OPTION_DIAGNOSTICS */
    int sort_rays = 0;                 /* WCPT_OPTION_SORT_RAYS (wavefront only; measured a net loss on c3) */
    int wf_stack = 10;                 /* WCPT_OPTION_WF_STACK: LDS stack entries of the wavefront trace kernel */
    int tri_cache = 1;                 /* WCPT_OPTION_TRIANGLE_CACHE */
    int prim_cache = 1;                /* WCPT_OPTION_PRIMARY_CACHE (active only with tri_cache) */
    int mk_split = wcpt::kMkSplitAuto; /* WCPT_OPTION_MK_SPLIT */
    int mk_tiny_tree = wcpt::kMkTinyAuto; /* WCPT_OPTION_MK_TINY_TREE */
    int packed_refs = 1;               /* WCPT_OPTION_PACKED_REFS */
    int wf_fetch = -1;                 /* WCPT_OPTION_WF_FETCH */
    int wf_persist = -1;               /* WCPT_OPTION_WF_PERSIST */
    int wf_refill = 20;                /* WCPT_OPTION_WF_REFILL (round 5 with the deferred hit stores, c4: 8 / 12 / 16 / 20 / 24 / 32 -> 203.5 / 199.6 / 198.9 / 198.0 / 198.6 / 201.4 ms; c3 flat; profiles/r05_fetch_once_ab.log) */
    /* the path-persistent trace's threshold while the option is unset (round 6, c3 8-way slowest share over 3 rounds,
     * refill 8 / 12 / 16 / 20: 8-row stripes 1.265 / 1.250 / 1.249 / 1.262 ms, row blocks 1.314 / 1.280 / 1.293 / 1.287
     * ms; profiles/r06_persist_refill_sweep_c3.log) */
    int wf_refill_persist = 12;
#ifndef WCPT_WF_PIPES_DEFAULT
#define WCPT_WF_PIPES_DEFAULT 0
#endif
    int wf_pipes = WCPT_WF_PIPES_DEFAULT; /* WCPT_OPTION_WF_PIPES (0 = by queue length, pt_wavefront.hip launch_wavefront) */
    int pair_records = -1;             /* WCPT_OPTION_PAIR_RECORDS: -1 auto, 0 singles, 1 pairs (megakernel) */
    int mk_tile_order = 2;             /* WCPT_OPTION_MK_TILE_ORDER: auto */
    int frame_overlap = 1;             /* WCPT_OPTION_FRAME_OVERLAP: auto */
    bool overlap_suppressed = false;   /* set by a group (wcpt::set_overlap_suppressed) */
    bool prep_missed = false;          /* the last render's preparation missed its cache (prepare_tri_records) */
    uint64_t generation = 0;           /* bumped by every buffer alloc / upload / free and every option change */
    /* Frame preparation of the last render (prepare_tri_records) and the last validation (render_validate), reused
     * while nothing they read can have changed: the same draw-command address and count, no buffer allocated,
     * uploaded or freed and no option changed since (ctx->generation), the draw commands read from the host copy of
     * wcpt_buffer_upload (never from the device, which the application may write behind the runtime), and for the
     * primary-ray records the same camera position. An unchanged frame -- progressive accumulation, a group's every
     * rank every frame -- then does no draw-command copy, lookup, allocation or table compare. */
    struct PrepCache {
        bool valid = false;
        uint64_t gen = 0, draws = 0;
        uint32_t n = 0;
        uint32_t origin[3] = {0, 0, 0};
        wcpt::FramePlan plan;
    } prep;
    struct ValidCache {
        bool valid = false;
        uint64_t gen = 0, draws = 0;
        uint32_t n = 0;
    } validated;
    /* draw commands render_validate had to read from the device, handed to the render that follows it (one read, one
     * host-blocking sync per frame instead of two) */
    std::vector<wcpt_draw_command> handoff;
    uint64_t handoff_draws = 0;
    bool handoff_valid = false;
    std::vector<TriRecords> tri;       /* per draw command index */
    std::vector<uint64_t> tri_table;   /* host image of d_tri_table: kTriTableWords per draw (frame_prep.h) */
    uint64_t* d_tri_table = nullptr;   /* two tables of tri_table_cap draws: the context stream's, then pipe 1's, whose
                                        * kTriWordPrimary points at the pipe-1 copy of the primary-ray records */
    uint32_t tri_table_cap = 0;        /* draws d_tri_table can hold */
    std::string last_error;
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    int profile_region = 0;     /* WCPT_OPTION_PROFILE_REGION */
    uint32_t region_renders = 0; /* renders since wcpt_profile_begin (region timing) */
};

namespace {

int set_error(wcpt_context* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->last_error = buf;
    std::lock_guard<std::mutex> lk(g_err_mutex);
    g_last_error = buf;
    return code;
}

int hip_fail(wcpt_context* ctx, hipError_t e, const char* what)
{
    const int code = (e == hipErrorOutOfMemory) ? WCPT_ERROR_OUT_OF_DEVICE_MEMORY : WCPT_ERROR_DEVICE_LOST;
    return set_error(ctx, code, "%s: %s", what, hipGetErrorString(e));
}

#define HIP_TRY(ctx, expr, what)                                  \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return hip_fail((ctx), _e, (what)); \
    } while (0)

/* the context's device current, without touching its stream (render_common: a render may continue the overlap) */
int bind_device(wcpt_context* ctx)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    HIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    return WCPT_SUCCESS;
}

/* Frames the frame-overlap pipes hold (MkState::pending) are joined into the context's stream before anything else
 * is queued there or waited for: every entry point but a render binds through here, and so does the group's access
 * to the stream (context_stream), so stream order is as if each render had run on the stream itself. */
int join_pending(wcpt_context* ctx)
{
    if (ctx->mk.pending) HIP_TRY(ctx, wcpt::mk_join(ctx->mk, ctx->stream), "frame overlap join");
    if (ctx->wf.pending) HIP_TRY(ctx, wcpt::wf_join(ctx->wf, ctx->stream), "frame overlap join (wavefront)");
    return WCPT_SUCCESS;
}

int bind(wcpt_context* ctx)
{
    const int rc = bind_device(ctx);
    return rc ? rc : join_pending(ctx);
}

Buffer* find_buffer(wcpt_context* ctx, wcpt_buffer h)
{
    auto it = ctx->buffers.find(h);
    return it == ctx->buffers.end() ? nullptr : &it->second;
}

int ensure_scratch(wcpt_context* ctx, uint64_t bytes)
{
    if (ctx->scratch_bytes >= bytes) return WCPT_SUCCESS;
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    ctx->d_scratch = nullptr;
    ctx->scratch_bytes = 0;
    HIP_TRY(ctx, hipMalloc(&ctx->d_scratch, bytes), "hipMalloc(selftest scratch)");
    ctx->scratch_bytes = bytes;
    return WCPT_SUCCESS;
}

int alloc_image(wcpt_context* ctx, uint32_t w, uint32_t h, uint32_t y0, uint32_t rows)
{
    const uint64_t bytes = (uint64_t)w * rows * 16ull;
    if (ctx->external_bytes) {
        if (bytes > ctx->external_bytes)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image of %llu bytes < %llu needed",
                             (unsigned long long)ctx->external_bytes, (unsigned long long)bytes);
    } else if (bytes > ctx->image_bytes_cap) {
        if (ctx->own_image) (void)hipFree(ctx->own_image);
        ctx->own_image = nullptr;
        ctx->image = nullptr;
        ctx->image_bytes_cap = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->own_image, bytes), "hipMalloc(image)");
        ctx->image_bytes_cap = bytes;
        ctx->image = ctx->own_image;
    }
    ctx->width = w;
    ctx->height = h;
    ctx->y0 = y0;
    ctx->rows = rows;
    return WCPT_SUCCESS;
}

/* The context's row map (row_map.h): frame row of each local row. */
wcpt::RowMap row_map(const wcpt_context* ctx)
{
    if (!ctx->stripe) return {ctx->y0, wcpt::kContiguousShift, 0u};
    return {ctx->y0, (uint32_t)__builtin_ctz(ctx->stripe), ctx->period - ctx->stripe};
}

/* The frame row of the context's last local row (its rows must be > 0). */
uint64_t last_frame_row(const wcpt_context* ctx) { return wcpt::frame_row64(row_map(ctx), ctx->rows - 1u); }

/* The buffer whose [ptr, ptr + bytes) contains device address `addr`, or null. */
Buffer* buffer_at(wcpt_context* ctx, uint64_t addr, uint64_t& offset)
{
    for (auto& kv : ctx->buffers) {
        const uint64_t base = reinterpret_cast<uint64_t>(kv.second.ptr);
        if (kv.second.ptr && addr >= base && addr < base + kv.second.bytes) {
            offset = addr - base;
            return &kv.second;
        }
    }
    return nullptr;
}

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

/* A device allocation that work queued on the context's stream may still read, replaced by one of `bytes`: that work
 * is waited for only when there is an old allocation. */
template <class T, class C>
int grow(wcpt_context* ctx, T*& mem, C& cap, C new_cap, uint64_t bytes, const char* what)
{
    if (mem) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        (void)hipFree(mem);
    }
    mem = nullptr;
    cap = 0;
    HIP_TRY(ctx, hipMalloc(&mem, bytes), what);
    cap = new_cap;
    return WCPT_SUCCESS;
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
    if (!ctx->image || ctx->width == 0 || ctx->rows == 0)
        return set_error(ctx, WCPT_ERROR_NO_SCREEN, "wcpt_render: no output image (call wcpt_create_screen)");
    if (scene->sphereCount > 0 && spheres == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: sphereCount > 0 with a null sphere buffer");
    if (scene->drawCommandCount > 0 && draws == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: drawCommandCount > 0 with null draw commands");
    if (materials == 0 && (scene->sphereCount > 0 || scene->drawCommandCount > 0))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wcpt_render: null material buffer");
    /* the output's rows: the context's rows back to back, or (WCPT_OPTION_GATHER_FRAME_ROWS) frame rows up to its last */
    const uint64_t wire_rows = ctx->gather_frame_rows ? last_frame_row(ctx) + 1u : ctx->rows;
    if (ctx->wire && mode == wcpt::kModeRender &&
        (uint64_t)ctx->width * wire_rows * payload_pixel_bytes(ctx->wire_ch) > ctx->wire_bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "gather output of %llu bytes too small for %ux%llu x %u B",
                         (unsigned long long)ctx->wire_bytes, ctx->width, (unsigned long long)wire_rows,
                         (unsigned)payload_pixel_bytes(ctx->wire_ch));
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
    a.W = ctx->width;
    a.H = ctx->height;
    a.y0 = ctx->y0;
    a.rows = ctx->rows;
    {
        const wcpt::RowMap m = row_map(ctx);
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
/* Profiling events time the launches only: no system-scope fence when they are recorded (hip_runtime_api.h,
 * hipEventDisableSystemFence), so the timed frames pay no cache writeback between launches (c2 0.538 -> 0.534
 * ms/frame against hipEventReleaseToDevice and hipEventDefault, which measured alike). */
#ifndef WCPT_PROFILE_EVENT_FLAGS
#define WCPT_PROFILE_EVENT_FLAGS hipEventDisableSystemFence
#endif
    if (ctx->profiling && mode == wcpt::kModeRender && ctx->profile_region) {
        /* region timing: one event before the first render; wcpt_profile_end records the closing one */
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

int read_status(wcpt_context* ctx)
{
    uint32_t st = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&st, ctx->d_status, 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(status)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (st) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, 4, ctx->stream), "hipMemsetAsync(status)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        return set_error(ctx, WCPT_ERROR_STACK_OVERFLOW,
                         "BVH traversal stack overflow (tree deeper than %d levels); image is incomplete",
                         wcpt::kStackDepth);
    }
    return WCPT_SUCCESS;
}

} // namespace

/* Internal hooks for the multi-device group (wcpt_group.hip): a context's current stream, and error reporting
 * through the same last-error strings as the C entry points. */
namespace wcpt {
hipStream_t context_stream(wcpt_context* ctx)
{
    if (!ctx) return nullptr;
    /* the group queues waits, copies and events here: pending overlap frames first (a failed join surfaces at the
     * group's next stream operation or sync) */
    (void)join_pending(ctx);
    return ctx->stream;
}
int context_device(wcpt_context* ctx) { return ctx ? ctx->device : -1; }
int context_error(wcpt_context* ctx, int code, const char* msg) { return set_error(ctx, code, "%s", msg); }
/* A validated frame that will not be rendered (another rank's validation failed): drop its hand-off. */
void render_abandon(wcpt_context* ctx)
{
    if (ctx) ctx->handoff_valid = false;
}

void set_overlap_suppressed(wcpt_context* ctx, bool on)
{
    if (ctx) ctx->overlap_suppressed = on;
}

int context_frame_streams(wcpt_context* ctx, hipStream_t* out, int cap)
{
    if (!ctx || cap < 1) return 0;
    int n = 0;
    out[n++] = ctx->stream;
    if (ctx->mk.pending)
        for (uint32_t p = 1; p < wcpt::kMkPipes && n < cap; p++) out[n++] = ctx->mk.pipe[p];
    if (ctx->wf.pending)
        for (uint32_t j = 1; j < ctx->wf.pending_pipes && n < cap; j++) out[n++] = ctx->wf.aux[j];
    return n;
}

/* Every check wcpt_render would make before it launches anything, with no launch: the argument checks and, per draw
 * command, the checks of the record build (check_draw). A group validates all its ranks first, so
 * that an argument error cannot leave some ranks a frame ahead of the others. */
int render_validate(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
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

/* CreateScreen of one row block in one step: the frame's size and the context's block [y0, y0 + rows) are set
 * together, so only the block is allocated (and zeroed), whatever the previous frame's size was. */
int set_frame_block(wcpt_context* ctx, uint32_t width, uint32_t height, uint32_t y0, uint32_t rows, uint32_t stripe,
                    uint32_t period)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (stripe && (stripe & (stripe - 1u) || stripe > 32768u || period < stripe))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row stripes of %u rows every %u rows", stripe, period);
    const uint64_t last = rows == 0 ? 0 : frame_row64(wcpt::RowMap{y0, stripe ? (uint32_t)__builtin_ctz(stripe) : kContiguousShift,
                                                                 stripe ? period - stripe : 0u}, rows - 1u);
    if (width == 0 || rows == 0 || last >= height)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%u rows from row %u (stripes %u / %u) in a %ux%u frame", rows,
                         y0, stripe, period, width, height);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->sharded = true;
    ctx->stripe = stripe;
    ctx->period = stripe ? period : 0u;
    rc = alloc_image(ctx, width, height, y0, rows);
    if (rc) return rc;
    if (!ctx->external_bytes) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->image, 0, (uint64_t)width * rows * 16ull, ctx->stream), "hipMemsetAsync(image)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    return WCPT_SUCCESS;
}
} // namespace wcpt

extern "C" {

int wcpt_abi_version(void) { return WCPT_ABI_VERSION; }

#ifndef WCPT_BUILD_ID
#define WCPT_BUILD_ID "unknown"
#endif
const char* wcpt_build_id(void) { return WCPT_BUILD_ID; }

int wcpt_runtime_version(int* version)
{
    if (!version) return set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "null version");
    hipError_t e = hipRuntimeGetVersion(version);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipRuntimeGetVersion");
    return WCPT_SUCCESS;
}

const char* wcpt_last_error(const wcpt_context* ctx)
{
    if (ctx) return ctx->last_error.c_str();
    std::lock_guard<std::mutex> lk(g_err_mutex);
    return g_last_error.c_str();
}

int wcpt_device_count(int* count)
{
    if (!count) return set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        (void)hipGetLastError();
        return WCPT_SUCCESS; /* no device is not an error for the query */
    }
    *count = n;
    return WCPT_SUCCESS;
}

int wcpt_device_pci_bus_id(int device, char* out, int len)
{
    if (!out || len < 13) return set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "pci bus id buffer of %d bytes", len);
    const hipError_t e = hipDeviceGetPCIBusId(out, len, device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        out[0] = 0;
        return set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "hipDeviceGetPCIBusId(%d): %s", device, hipGetErrorString(e));
    }
    return WCPT_SUCCESS;
}

int wcpt_create(int device, wcpt_context** out_ctx)
{
    if (!out_ctx) return set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "null out_ctx");
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return set_error(nullptr, WCPT_ERROR_INITIALIZATION_FAILED, "no HIP device available");
    }
    if (device < 0 || device >= n)
        return set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, n);
    wcpt_context* ctx = new (std::nothrow) wcpt_context();
    if (!ctx) return set_error(nullptr, WCPT_ERROR_OUT_OF_HOST_MEMORY, "out of host memory");
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_status, 4);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_counters, kNumCounters * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(ctx->d_status, 0, 4);
    if (e != hipSuccess) {
        int rc = hip_fail(nullptr, e, "wcpt_create");
        wcpt_destroy(ctx);
        return rc;
    }
    ctx->stream = ctx->own_stream;
    *out_ctx = ctx;
    return WCPT_SUCCESS;
}

int wcpt_destroy(wcpt_context* ctx)
{
    if (!ctx) return WCPT_SUCCESS;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)join_pending(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->buffers)
        if (kv.second.raw) (void)hipFree(kv.second.raw);
    if (ctx->own_image) (void)hipFree(ctx->own_image);
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    wcpt::wf_release(ctx->wf);
    wcpt::mk_release(ctx->mk);
    for (auto& t : ctx->tri) {
        if (t.mem) (void)hipFree(t.mem);
        if (t.pmem) (void)hipFree(t.pmem);
    }
    if (ctx->d_tri_table) (void)hipFree(ctx->d_tri_table);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    if (ctx->d_scan) (void)hipFree(ctx->d_scan);
    if (ctx->d_bloom) (void)hipFree(ctx->d_bloom);
    if (ctx->d_bvh) (void)hipFree(ctx->d_bvh);
    for (auto& p : ctx->events) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return WCPT_SUCCESS;
}

int wcpt_set_stream(wcpt_context* ctx, void* hip_stream)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return WCPT_SUCCESS;
}

int wcpt_set_kernel(wcpt_context* ctx, int variant)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (variant != WCPT_KERNEL_MEGAKERNEL && variant != WCPT_KERNEL_WAVEFRONT && variant != WCPT_KERNEL_AUTO)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "kernel variant %d not available", variant);
    if (ctx->kernel != variant) ctx->generation++; /* the cached frame preparation resolved the variant */
    ctx->kernel = variant;
    return WCPT_SUCCESS;
}

int wcpt_last_kernel(wcpt_context* ctx, int* variant)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (!variant) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null variant");
    *variant = ctx->kernel_run;
    return WCPT_SUCCESS;
}

int wcpt_last_arith(wcpt_context* ctx, int* arith)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (!arith) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null arith");
    *arith = ctx->arith_run;
    return WCPT_SUCCESS;
}

int wcpt_set_option(wcpt_context* ctx, int option, int value)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    /* The options that prepare_tri_records / render_validate read (record formats, stack-entry layout, the cache
     * itself) invalidate their cached frame preparation once accepted: ctx->generation++ there only, so a host that
     * sets the other options every frame keeps the cache. */
    switch (option) {
    case WCPT_OPTION_SORT_RAYS:
        ctx->sort_rays = value ? 1 : 0;
        return WCPT_SUCCESS;
    case WCPT_OPTION_WF_REFILL:
        if (value < 1 || value > 64) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "refill threshold %d", value);
        ctx->wf_refill = value;
        ctx->wf_refill_persist = value; /* an explicit value governs both traces */
        return WCPT_SUCCESS;
    case WCPT_OPTION_WF_PIPES:
        if (value < 0 || value > wcpt::kWfMaxPipes) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "pipelines %d", value);
        ctx->wf_pipes = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_MK_TILE_ORDER:
        if (value < 0 || value > 6) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "tile order %d", value);
        ctx->mk_tile_order = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_FRAME_OVERLAP:
        if (value < 0 || value > 2) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "frame overlap %d", value);
        ctx->frame_overlap = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_PACKED_REFS:
        ctx->packed_refs = value ? 1 : 0;
        ctx->generation++;
        return WCPT_SUCCESS;
    case WCPT_OPTION_PAIR_RECORDS:
        if (value < -1 || value > 1) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "pair records %d", value);
        ctx->pair_records = value;
        ctx->generation++;
        return WCPT_SUCCESS;
    case WCPT_OPTION_TRIANGLE_CACHE:
        ctx->tri_cache = value ? 1 : 0;
        ctx->generation++;
        return WCPT_SUCCESS;
    case WCPT_OPTION_PRIMARY_CACHE:
        if (value < 0 || value > 1) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "primary cache %d", value);
        ctx->prim_cache = value;
        ctx->generation++;
        return WCPT_SUCCESS;
    case WCPT_OPTION_MK_SPLIT:
        if (value < wcpt::kMkSplitAuto || value > wcpt::kMkSplitMaxCut)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "megakernel split %d", value);
        ctx->mk_split = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_MK_TINY_TREE:
        if (value < wcpt::kMkTinyAuto || value > 1)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "megakernel tiny tree %d", value);
        if (ctx->mk_tiny_tree != value) ctx->generation++; /* the draw's table flag is part of the cached frame preparation */
        ctx->mk_tiny_tree = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_ARITH:
        if (value != WCPT_ARITH_EXACT && value != WCPT_ARITH_FAST)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "arithmetic mode %d", value);
        ctx->arith = value;
        ctx->generation++; /* the primary cache's key holds the generation: a record belongs to the arithmetic that found it */
        return WCPT_SUCCESS;
    case WCPT_OPTION_WF_STACK:
        if (value != 10 && value != 16 && value != 24)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wavefront LDS stack %d (10, 16 or 24)", value);
        ctx->wf_stack = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_DIAGNOSTICS:
        ctx->diagnostics = value ? 1 : 0;
        return WCPT_SUCCESS;
    case WCPT_OPTION_WF_PERSIST:
        if (value < -1 || value > 1) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wavefront persist %d", value);
        ctx->wf_persist = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_WF_FETCH:
        if (value < -1 || value > 1) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wavefront fetch rounds %d", value);
        ctx->wf_fetch = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_PROFILE_REGION:
        if (ctx->profiling) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "profile region: set outside profiling");
        ctx->profile_region = value ? 1 : 0;
        return WCPT_SUCCESS;
    case WCPT_OPTION_STACK:
        if (value < 0 || value > 1) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "stack kind %d", value);
        ctx->stack_kind = value;
        return WCPT_SUCCESS;
    case WCPT_OPTION_GATHER_FRAME_ROWS:
        if (value < 0 || value > 1) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "gather frame rows %d", value);
        ctx->gather_frame_rows = value;
        return WCPT_SUCCESS;
    default: return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "unknown option %d", option);
    }
}

/* ---- buffers ------------------------------------------------------------------------------------ */
int wcpt_buffer_alloc(wcpt_context* ctx, uint64_t bytes, wcpt_buffer* out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null out handle");
    Buffer b;
    HIP_TRY(ctx, skewed_alloc(b, bytes), "hipMalloc(buffer)");
    b.generation = ++ctx->generation;
    if (bytes <= kShadowMax) b.shadow.assign(bytes, 0); /* hipMalloc contents are undefined; see upload */
    if (bytes <= kShadowMax) b.known.assign((bytes + kShadowChunk - 1) / kShadowChunk, 0);
    const uint64_t h = ctx->next_handle++;
    ctx->buffers[h] = b;
    *out = h;
    return WCPT_SUCCESS;
}

int wcpt_buffer_upload(wcpt_context* ctx, wcpt_buffer buf, const void* src, uint64_t bytes, uint64_t offset)
{
    int rc = bind(ctx);
    if (rc) return rc;
    Buffer* b = find_buffer(ctx, buf);
    if (!b) return set_error(ctx, WCPT_ERROR_INVALID_HANDLE, "unknown buffer handle %llu", (unsigned long long)buf);
    if (bytes && !src) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null upload source");
    uint64_t end = 0;
    if (__builtin_add_overflow(offset, bytes, &end) || end > (1ull << 48))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "upload range offset %llu + %llu bytes overflows",
                         (unsigned long long)offset, (unsigned long long)bytes);
    if (end > b->bytes) {
        /* grow, keeping the old contents (BufferManager.jai:53-54 reallocates on growth) */
        Buffer nb;
        HIP_TRY(ctx, skewed_alloc(nb, end), "hipMalloc(buffer grow)");
        if (b->ptr && b->bytes) {
            hipError_t e = hipMemcpyAsync(nb.ptr, b->ptr, b->bytes, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) {
                (void)hipFree(nb.raw);
                return hip_fail(ctx, e, "buffer grow copy");
            }
        }
        if (b->raw) (void)hipFree(b->raw);
        nb.shadow = std::move(b->shadow);
        nb.known = std::move(b->known);
        *b = std::move(nb);
        if (b->bytes <= kShadowMax) {
            b->shadow.resize(b->bytes, 0);
            b->known.resize((b->bytes + kShadowChunk - 1) / kShadowChunk, 0); /* the grown tail is undefined */
        } else {
            b->shadow.clear();
            b->known.clear();
        }
    }
    if (bytes) {
        HIP_TRY(ctx, hipMemcpyAsync(static_cast<char*>(b->ptr) + offset, src, bytes, hipMemcpyHostToDevice, ctx->stream),
                "hipMemcpyAsync(upload)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(upload)"); /* blocking, like :98-112 */
        if (b->shadow.size() == b->bytes && b->bytes) {
            std::memcpy(b->shadow.data() + offset, src, bytes);
            shadow_mark(*b, offset, end);
        }
    }
    b->generation = ++ctx->generation;
    return WCPT_SUCCESS;
}

int wcpt_buffer_download(wcpt_context* ctx, wcpt_buffer buf, void* dst, uint64_t bytes, uint64_t offset)
{
    int rc = bind(ctx);
    if (rc) return rc;
    Buffer* b = find_buffer(ctx, buf);
    if (!b) return set_error(ctx, WCPT_ERROR_INVALID_HANDLE, "unknown buffer handle %llu", (unsigned long long)buf);
    if (bytes > b->bytes || offset > b->bytes - bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "download out of range");
    if (bytes && !dst) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null download destination");
    if (bytes) {
        HIP_TRY(ctx, hipMemcpyAsync(dst, static_cast<char*>(b->ptr) + offset, bytes, hipMemcpyDeviceToHost, ctx->stream),
                "hipMemcpyAsync(download)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(download)");
    }
    return WCPT_SUCCESS;
}

int wcpt_buffer_size(wcpt_context* ctx, wcpt_buffer buf, uint64_t* out_bytes)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    Buffer* b = find_buffer(ctx, buf);
    if (!b) return set_error(ctx, WCPT_ERROR_INVALID_HANDLE, "unknown buffer handle");
    if (!out_bytes) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null out_bytes");
    *out_bytes = b->bytes;
    return WCPT_SUCCESS;
}

uint64_t wcpt_buffer_device_address(wcpt_context* ctx, wcpt_buffer buf)
{
    if (!ctx) return 0;
    Buffer* b = find_buffer(ctx, buf);
    if (!b) {
        set_error(ctx, WCPT_ERROR_INVALID_HANDLE, "unknown buffer handle");
        return 0;
    }
    return reinterpret_cast<uint64_t>(b->ptr);
}

int wcpt_buffer_free(wcpt_context* ctx, wcpt_buffer buf)
{
    int rc = bind(ctx);
    if (rc) return rc;
    auto it = ctx->buffers.find(buf);
    if (it == ctx->buffers.end()) return set_error(ctx, WCPT_ERROR_INVALID_HANDLE, "unknown buffer handle");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(free)");
    if (it->second.raw) HIP_TRY(ctx, hipFree(it->second.raw), "hipFree");
    ctx->buffers.erase(it);
    ctx->generation++;
    return WCPT_SUCCESS;
}

/* ---- BVH build on the device (pt_bvh_build.hip) --------------------------------------------------- */
int wcpt_bvh_build_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                          uint32_t index_count, wcpt_buffer nodes, uint32_t* nodes_used)
{
    int rc = bind(ctx);
    if (rc) return rc;
    Buffer* bv = find_buffer(ctx, vertices);
    Buffer* bi = find_buffer(ctx, indices);
    Buffer* bn = find_buffer(ctx, nodes);
    if (!bv || !bi || !bn) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: unknown buffer handle");
    if (bv == bi || bv == bn || bi == bn) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: the three buffers must differ");
    if (!nodes_used) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: null nodes_used");
    if (index_count == 0 || index_count % 3 != 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: index_count %u is zero or no multiple of 3", index_count);
    if ((uint64_t)vertex_count * 12ull > bv->bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: %u vertices exceed the vertex buffer (%llu bytes)",
                         vertex_count, (unsigned long long)bv->bytes);
    if ((uint64_t)index_count * 4ull > bi->bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: %u indices exceed the index buffer (%llu bytes)",
                         index_count, (unsigned long long)bi->bytes);
    const uint64_t node_bound = 2ull * index_count / 3ull;
    if (bn->bytes / sizeof(wcpt_node) < node_bound)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: the node buffer holds %llu nodes, %llu needed",
                         (unsigned long long)(bn->bytes / sizeof(wcpt_node)), (unsigned long long)node_bound);
    const uint64_t need = wcpt::bvh_build_scratch_bytes(index_count);
    if (ctx->bvh_bytes < need) {
        rc = grow(ctx, ctx->d_bvh, ctx->bvh_bytes, need, need, "hipMalloc(bvh build scratch)");
        if (rc) return rc;
    }
    uint32_t status = 0, used = 0;
    HIP_TRY(ctx, wcpt::bvh_build_device(static_cast<const float*>(bv->ptr), vertex_count, static_cast<uint32_t*>(bi->ptr),
                                        index_count, bn->ptr, ctx->d_bvh, &status, &used, ctx->stream), "bvh build");
    if (status & wcpt::kBvhBadIndex)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: an index is not below vertex_count %u", vertex_count);
    if (status & wcpt::kBvhNotFinite)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: a referenced coordinate is not finite");
    /* a write of both buffers, as wcpt_buffer_upload's: the host copies no longer know the range, and everything keyed
     * on the generations (triangle records, leaf scan, tiny-tree flag, frame preparation, primary cache) is re-learned */
    shadow_forget(*bi, 0, (uint64_t)index_count * 4ull);
    shadow_forget(*bn, 0, (uint64_t)used * sizeof(wcpt_node));
    bi->generation = ++ctx->generation;
    bn->generation = ++ctx->generation;
    *nodes_used = used;
    return WCPT_SUCCESS;
}

/* ---- image -------------------------------------------------------------------------------------- */
int wcpt_create_screen(wcpt_context* ctx, uint32_t width, uint32_t height)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (width == 0 || height == 0) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "zero-sized screen");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    uint32_t y0 = 0, rows = height;
    if (ctx->sharded && ctx->stripe) {
        /* interleaved stripes: kept while every row still lies in the new frame, else the full frame */
        if (ctx->rows && last_frame_row(ctx) < height) {
            y0 = ctx->y0;
            rows = ctx->rows;
        } else {
            ctx->sharded = false;
            ctx->stripe = ctx->period = 0;
        }
    } else if (ctx->sharded && ctx->y0 < height) {
        y0 = ctx->y0;
        rows = (ctx->y0 + ctx->rows <= height) ? ctx->rows : height - ctx->y0;
    } else {
        ctx->sharded = false;
    }
    rc = alloc_image(ctx, width, height, y0, rows);
    if (rc) return rc;
    /* The reference's storage image starts undefined (PathTracingRenderer.jai:345-385) and its editor's first
     * frame already blends with it (renderedFramesCount 1, editor.jai:149-152): define it as zero. */
    if (!ctx->external_bytes) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->image, 0, (uint64_t)width * rows * 16ull, ctx->stream), "hipMemsetAsync(image)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    return WCPT_SUCCESS;
}

int wcpt_resize(wcpt_context* ctx, uint32_t width, uint32_t height)
{
    return wcpt_create_screen(ctx, width, height); /* Resize = DestroyScreen + CreateScreen (:393-397) */
}

int wcpt_set_row_range(wcpt_context* ctx, uint32_t y0, uint32_t rows)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (rows == 0) {
        ctx->sharded = false;
        ctx->stripe = ctx->period = 0;
        if (ctx->height) return alloc_image(ctx, ctx->width, ctx->height, 0, ctx->height);
        return WCPT_SUCCESS;
    }
    if (ctx->height && (uint64_t)y0 + rows > ctx->height)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row range [%u,%u) outside frame height %u", y0, y0 + rows,
                         ctx->height);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->sharded = true;
    ctx->stripe = ctx->period = 0;
    ctx->y0 = y0;
    ctx->rows = rows;
    if (ctx->height) return alloc_image(ctx, ctx->width, ctx->height, y0, rows);
    return WCPT_SUCCESS;
}

int wcpt_set_row_stripes(wcpt_context* ctx, uint32_t y_first, uint32_t rows, uint32_t stripe, uint32_t period)
{
    if (stripe == 0) return wcpt_set_row_range(ctx, y_first, rows);
    int rc = bind(ctx);
    if (rc) return rc;
    if (rows == 0 || stripe & (stripe - 1u) || stripe > 32768u || period < stripe)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%u rows in stripes of %u rows every %u rows", rows, stripe,
                         period);
    const uint64_t last = wcpt::frame_row64(wcpt::RowMap{y_first, (uint32_t)__builtin_ctz(stripe), period - stripe}, rows - 1u);
    if (ctx->height && last >= ctx->height)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row stripes reach row %llu of a frame of height %u",
                         (unsigned long long)last, ctx->height);
    if (last > 0xFFFFFFFFull)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row stripes past row 2^32");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->sharded = true;
    ctx->stripe = stripe;
    ctx->period = period;
    ctx->y0 = y_first;
    ctx->rows = rows;
    if (ctx->height) return alloc_image(ctx, ctx->width, ctx->height, y_first, rows);
    return WCPT_SUCCESS;
}

uint64_t wcpt_image_device_ptr(wcpt_context* ctx) { return ctx ? reinterpret_cast<uint64_t>(ctx->image) : 0; }

int wcpt_set_external_image(wcpt_context* ctx, uint64_t device_ptr, uint64_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (device_ptr == 0) {
        ctx->external_bytes = 0;
        ctx->image = ctx->own_image;
        if (ctx->width && ctx->rows) return alloc_image(ctx, ctx->width, ctx->height, ctx->y0, ctx->rows);
        return WCPT_SUCCESS;
    }
    if (bytes == 0) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image of 0 bytes");
    if (ctx->width && (uint64_t)ctx->width * ctx->rows * 16ull > bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image too small for %ux%u", ctx->width, ctx->rows);
    ctx->external_bytes = bytes;
    ctx->image = reinterpret_cast<float4*>(device_ptr);
    return WCPT_SUCCESS;
}

int wcpt_set_gather_output(wcpt_context* ctx, uint64_t device_ptr, uint64_t bytes, uint32_t channels)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (device_ptr == 0) {
        ctx->wire = nullptr;
        ctx->wire_bytes = 0;
        return WCPT_SUCCESS;
    }
    if (channels != WCPT_PAYLOAD_RGB32F && channels != WCPT_PAYLOAD_RGBA32F && channels != WCPT_PAYLOAD_DISPLAY_RGBA8)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "gather output format %u (3, 4 or 8)", channels);
    if (bytes == 0 || (device_ptr & 3u))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "gather output: %llu bytes at a misaligned or empty buffer",
                         (unsigned long long)bytes);
    if (channels == WCPT_PAYLOAD_RGBA32F && (device_ptr & 15u))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "gather output: RGBA needs 16-byte alignment");
    ctx->wire = reinterpret_cast<float*>(device_ptr);
    ctx->wire_bytes = bytes;
    ctx->wire_ch = channels;
    return WCPT_SUCCESS;
}

int wcpt_readback(wcpt_context* ctx, float* dst, uint64_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const uint64_t have = (uint64_t)ctx->width * ctx->rows * 16ull;
    if (!ctx->image) return set_error(ctx, WCPT_ERROR_NO_SCREEN, "no output image");
    if (!dst || bytes > have) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "readback of %llu bytes, image holds %llu",
                                               (unsigned long long)bytes, (unsigned long long)have);
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->image, bytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(readback)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(readback)");
    return read_status(ctx);
}

namespace {

/* What wcpt_composite and wcpt_composite_bloom check about their output: the image exists, the format is one of the
 * two, and a destination inside a context buffer holds the frame's bytes. */
int check_composite_target(wcpt_context* ctx, uint64_t dst, int format)
{
    if (!ctx->image) return set_error(ctx, WCPT_ERROR_NO_SCREEN, "no output image");
    if (format != WCPT_COMPOSITE_RGBA32F && format != WCPT_COMPOSITE_RGBA8)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "composite format %d", format);
    if (!dst) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null composite destination");
    const uint64_t pixels = (uint64_t)ctx->width * ctx->rows;
    const uint64_t need = pixels * (format == WCPT_COMPOSITE_RGBA8 ? 4ull : 16ull);
    uint64_t off = 0;
    Buffer* b = buffer_at(ctx, dst, off);
    if (b && off + need > b->bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "composite destination holds %llu bytes, %llu needed",
                         (unsigned long long)(b->bytes - off), (unsigned long long)need);
    return WCPT_SUCCESS;
}

} // namespace

int wcpt_composite(wcpt_context* ctx, uint64_t dst, int format)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = check_composite_target(ctx, dst, format);
    if (rc) return rc;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->rows;
    int dev = 0, cus = 0;
    HIP_TRY(ctx, hipGetDevice(&dev), "hipGetDevice");
    HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "hipDeviceGetAttribute");
    HIP_TRY(ctx, wcpt::launch_composite(ctx->image, pixels, reinterpret_cast<void*>(dst), format == WCPT_COMPOSITE_RGBA8,
                                        cus, ctx->stream), "composite launch");
    return WCPT_SUCCESS;
}

int wcpt_composite_bloom(wcpt_context* ctx, uint64_t dst, int format, const wcpt_bloom_params* p)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = check_composite_target(ctx, dst, format);
    if (rc) return rc;
    if (!p) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null bloom parameters");
    if (!wcpt_bloom_curve_ok(p->threshold, p->knee))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bloom threshold %g, knee %g (finite, knee > 0)", (double)p->threshold,
                         (double)p->knee);
    if (ctx->sharded)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bloom needs the whole frame: the context holds %u of %u rows",
                         ctx->rows, ctx->height);
    uint32_t lw[WCPT_BLOOM_MAX_LEVELS], lh[WCPT_BLOOM_MAX_LEVELS];
    const uint32_t levels = wcpt_bloom_plan(ctx->width, ctx->height, p->levels, lw, lh);
    if (levels == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bloom of %u levels (2..12) on a %ux%u frame (2 levels need 4x4)",
                         p->levels, ctx->width, ctx->height);
    /* both pyramids in one allocation, the down levels first; every level is written before it is read in each call, so
     * a new screen size only moves the levels */
    const uint64_t texels = wcpt::bloom_pyramid_texels(levels, lw, lh);
    if (2ull * texels * sizeof(float4) > ctx->bloom_bytes) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(bloom pyramids)");
        if (ctx->d_bloom) (void)hipFree(ctx->d_bloom);
        ctx->d_bloom = nullptr;
        ctx->bloom_bytes = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->d_bloom, 2ull * texels * sizeof(float4)), "hipMalloc(bloom pyramids)");
        ctx->bloom_bytes = 2ull * texels * sizeof(float4);
    }
    HIP_TRY(ctx, wcpt::launch_composite_bloom(ctx->image, ctx->width, ctx->height, p->threshold, p->knee, levels, lw, lh,
                                              ctx->d_bloom, ctx->d_bloom + texels, reinterpret_cast<void*>(dst),
                                              format == WCPT_COMPOSITE_RGBA8, ctx->stream), "bloom composite launch");
    return WCPT_SUCCESS;
}

int wcpt_image_upload(wcpt_context* ctx, const float* src, uint64_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const uint64_t have = (uint64_t)ctx->width * ctx->rows * 16ull;
    if (!ctx->image) return set_error(ctx, WCPT_ERROR_NO_SCREEN, "no output image");
    if (!src || bytes > have) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "image upload size");
    HIP_TRY(ctx, hipMemcpyAsync(ctx->image, src, bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(image)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return WCPT_SUCCESS;
}

/* ---- dispatch ------------------------------------------------------------------------------------ */
int wcpt_render(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials, uint64_t spheres,
                uint64_t draw_commands)
{
    return render_common(ctx, scene, materials, spheres, draw_commands, wcpt::kModeRender);
}

int wcpt_primary_cache_stats(wcpt_context* ctx, uint64_t* writes, uint64_t* reads)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (writes) *writes = ctx->mk.prim_writes;
    if (reads) *reads = ctx->mk.prim_reads;
    return WCPT_SUCCESS;
}

int wcpt_mk_split_stats(wcpt_context* ctx, uint64_t* renders)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (renders) *renders = ctx->mk.split_renders;
    return WCPT_SUCCESS;
}

int wcpt_mk_tiny_tree_stats(wcpt_context* ctx, uint64_t* renders)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (renders) *renders = ctx->mk.tiny_renders;
    return WCPT_SUCCESS;
}

int wcpt_sync(wcpt_context* ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return read_status(ctx);
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
    out->pixels = h[0];
    out->segments = h[1];
    out->sphere_tests = h[2];
    out->node_pops = h[3];
    out->interior_visits = h[4];
    out->triangle_tests = h[5];
    out->hits = h[6];
    out->draw_fetches = h[7];
    out->wave_interior_steps = h[8];
    out->lane_interior_steps = h[9];
    out->wave_triangle_steps = h[10];
    out->lane_triangle_steps = h[11];
    out->wave_segment_steps = h[12];
    out->lane_segment_steps = h[13];
    out->ref_stack_overflow_segments = h[14];
    out->ref_stack_max = h[15] == 0xFFFFFFFFull ? UINT64_MAX : h[15];
    return read_status(ctx);
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

/* ---- timing --------------------------------------------------------------------------------------- */
int wcpt_profile_begin(wcpt_context* ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    ctx->profiling = true;
    ctx->events_used = 0;
    ctx->region_renders = 0;
    return WCPT_SUCCESS;
}

int wcpt_profile_end(wcpt_context* ctx, double* kernel_ms_total, uint32_t* launches)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const bool region = ctx->profile_region && ctx->region_renders > 0;
    if (region) HIP_TRY(ctx, hipEventRecord(ctx->events[0].second, ctx->stream), "hipEventRecord");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    double total = 0.0;
    for (size_t i = 0; i < ctx->events_used; i++) {
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->events[i].first, ctx->events[i].second), "hipEventElapsedTime");
        total += ms;
    }
    if (kernel_ms_total) *kernel_ms_total = total;
    if (launches) *launches = region ? ctx->region_renders : (uint32_t)ctx->events_used;
    ctx->profiling = false;
    ctx->events_used = 0;
    ctx->region_renders = 0;
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
