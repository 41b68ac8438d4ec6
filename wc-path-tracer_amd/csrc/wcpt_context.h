/* wcpt_context.h — what every part of the C-ABI runtime shares: the context, its buffer table, error reporting, binding
 * a call to the context's device and stream, and the one on-demand device allocation. Internal: not installed, not part
 * of the ABI. The parts:
 *   wcpt_runtime.hip  the context itself: create / destroy, options, queries, sync, profiling, the group's hooks
 *   wcpt_buffers.hip  device buffers and their host copies, the device BVH builds' and refit's entry points
 *   wcpt_screen.hip   the image and which rows of the frame it holds (screen_layout.h), readback, the display step
 *   wcpt_render.hip   frame preparation (frame_prep.h), the render dispatch, the self-tests
 */
#ifndef WCPT_CONTEXT_H
#define WCPT_CONTEXT_H

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/wcpt.h"
#include "pt_kernels.h"
#include "screen_layout.h"

/* wcpt::rt is the runtime's own: none of it, nor a template instantiated over its types, is exported from the library */
#define WCPT_INTERNAL __attribute__((visibility("hidden")))

static_assert(wcpt::kPayloadRgb32f == WCPT_PAYLOAD_RGB32F && wcpt::kPayloadRgba32f == WCPT_PAYLOAD_RGBA32F &&
                  wcpt::kPayloadDisplayRgba8 == WCPT_PAYLOAD_DISPLAY_RGBA8, "screen_layout.h PayloadFormat");

namespace wcpt {
namespace rt WCPT_INTERNAL {

constexpr int kNumCounters = 16; /* wcpt_counters: 8 reference counters + 6 diagnostics + 2 reference-stack fields */

struct Buffer {
    void* raw = nullptr;   /* hipMalloc result */
    void* ptr = nullptr;   /* raw + the skew of wcpt_buffers.hip: the device address handed out */
    uint64_t bytes = 0;
    uint64_t generation = 0;      /* context-wide counter value of the last alloc / upload / grow */
    std::vector<uint8_t> shadow;  /* host copy of the uploaded contents (small buffers, wcpt_buffers.hip) */
    std::vector<uint8_t> known;   /* per chunk of it: 1 when `shadow` holds what wcpt_buffer_upload wrote */
};

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

} // namespace rt
} // namespace wcpt

struct wcpt_context {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::unordered_map<uint64_t, wcpt::rt::Buffer> buffers;
    uint64_t next_handle = 1;
    float4* image = nullptr;           /* the image kernels write: own_image or an external buffer */
    float4* own_image = nullptr;
    uint64_t image_bytes_cap = 0;
    uint64_t external_bytes = 0;       /* != 0 while an external image is attached */
    float* wire = nullptr;             /* wcpt_set_gather_output */
    uint64_t wire_bytes = 0;
    uint32_t wire_ch = 3;
    wcpt::ScreenLayout layout;         /* the frame's size and the rows of it the image holds (screen_layout.h) */
    int gather_frame_rows = 0;         /* WCPT_OPTION_GATHER_FRAME_ROWS */
    uint32_t* d_status = nullptr;
    unsigned long long* d_counters = nullptr;
    wcpt::WfPipes wf;                  /* path state + streams of the wavefront pipelines (allocated on first use) */
    wcpt::MkState mk;                  /* megakernel launch state (CU count, cost-ordered tiles) */
    uint32_t* d_scratch = nullptr;
    uint32_t* d_scan = nullptr;        /* leaf-count scan flag (prepare_tri_records) */
    float4* d_bloom = nullptr;         /* wcpt_composite_bloom: the down pyramid, then the up pyramid (on first use) */
    uint64_t bloom_bytes = 0;
    void* d_denoise = nullptr;         /* wcpt_composite_denoise: two float4 images, then the packed guide (on first use) */
    uint64_t denoise_bytes = 0;
    void* d_temporal = nullptr;        /* wcpt_composite_temporal: the sequence's state in two sides (pt_temporal.hip; on first use) */
    uint64_t temporal_bytes = 0;
    /* the history wcpt_composite_temporal carries: dropped by wcpt_temporal_reset and by every new layout of the screen */
    struct TemporalState {
        bool valid = false;
        uint32_t side = 0;             /* the side of d_temporal that holds the last output */
        float F[9] = {};               /* the camera that side's guide belongs to (wcpt_temporal.h wcpt_temporal_camera) */
        float position[3] = {};
    } temporal;
    void* d_bvh = nullptr;             /* wcpt_bvh_build_device / _sah_device / wcpt_bvh_refit_device: their scratch (on first use, grown on demand) */
    uint64_t bvh_bytes = 0;
    void* d_bvh_bins = nullptr;        /* wcpt_bvh_build_sah_device: the bins of a level's open nodes (grown on demand) */
    uint64_t bvh_bins_bytes = 0;
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
    std::vector<wcpt::rt::TriRecords> tri; /* per draw command index */
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

namespace wcpt {
namespace rt WCPT_INTERNAL {

/* the call's error code, with its message as the context's and the process's last error (wcpt_runtime.hip) */
int set_error(wcpt_context* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int hip_fail(wcpt_context* ctx, hipError_t e, const char* what);

#define HIP_TRY(ctx, expr, what)                                                \
    do {                                                                        \
        hipError_t _e = (expr);                                                 \
        if (_e != hipSuccess) return ::wcpt::rt::hip_fail((ctx), _e, (what));   \
    } while (0)

/* the context's device current, without touching its stream (render_common: a render may continue the overlap) */
inline int bind_device(wcpt_context* ctx)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    HIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    return WCPT_SUCCESS;
}

/* Frames the frame-overlap pipes hold (MkState::pending) are joined into the context's stream before anything else
 * is queued there or waited for: every entry point but a render binds through here, and so does the group's access
 * to the stream (context_stream), so stream order is as if each render had run on the stream itself. */
inline int join_pending(wcpt_context* ctx)
{
    if (ctx->mk.pending) HIP_TRY(ctx, wcpt::mk_join(ctx->mk, ctx->stream), "frame overlap join");
    if (ctx->wf.pending) HIP_TRY(ctx, wcpt::wf_join(ctx->wf, ctx->stream), "frame overlap join (wavefront)");
    return WCPT_SUCCESS;
}

inline int bind(wcpt_context* ctx)
{
    const int rc = bind_device(ctx);
    return rc ? rc : join_pending(ctx);
}

inline Buffer* find_buffer(wcpt_context* ctx, wcpt_buffer h)
{
    auto it = ctx->buffers.find(h);
    return it == ctx->buffers.end() ? nullptr : &it->second;
}

/* The buffer whose [ptr, ptr + bytes) contains device address `addr`, or null. */
inline Buffer* buffer_at(wcpt_context* ctx, uint64_t addr, uint64_t& offset)
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

/* True when the buffer's host copy holds every byte of [offset, offset + bytes) (wcpt_buffers.hip). */
bool shadow_known(const Buffer& b, uint64_t offset, uint64_t bytes);

/* The one on-demand device allocation: `mem`, which work queued on the context's stream may still read, replaced by
 * `bytes` new bytes, its recorded capacity `cap` by `new_cap`. That work is waited for only when there is an old
 * allocation; after a failure there is none (mem null, cap 0). */
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

/* the kernels' status word, read and cleared: a traversal stack overflow is the call's error (wcpt_runtime.hip) */
int read_status(wcpt_context* ctx);

} // namespace rt
} // namespace wcpt

#endif
