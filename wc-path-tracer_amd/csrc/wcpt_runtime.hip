/*
 * wcpt_runtime.hip — C-ABI runtime, the context itself: create / destroy, versions, errors, device queries, stream,
 * kernel and option setters, what the last render ran, sync and timing. Its buffers, its image and its renders are
 * wcpt_buffers.hip, wcpt_screen.hip and wcpt_render.hip; wcpt_context.h holds what they share.
 *
 * Replaces the Vulkan plumbing of the reference's renderer host (src/PathTracingRenderer.jai,
 * src/BufferManager.jai, modules/VKUtils/{Buffer,Synchronization}.jai); see include/wcpt.h for the
 * line-by-line mapping. HIP device memory replaces VMA GPU-only buffers; a device pointer IS the buffer
 * device address (VK_KHR_buffer_device_address, pathTracer.comp:74-95).
 */
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <new>

#include "wcpt_context.h"

using namespace wcpt::rt;

namespace {
std::mutex g_err_mutex;
std::string g_last_error;
} // namespace

namespace wcpt {
namespace rt WCPT_INTERNAL {

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

} // namespace rt

/* Internal hooks for the multi-device group (wcpt_group.hip, declared in pt_kernels.h): a context's current stream, and
 * error reporting through the same last-error strings as the C entry points. */
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

/* host/wcpt_host.cpp: a host utility's refusal becomes the process's last error (not part of the ABI) */
void wcpt_internal_note_error(const char* text) { set_error(nullptr, WCPT_ERROR_INVALID_ARGUMENT, "%s", text ? text : ""); }

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
    if (ctx->d_denoise) (void)hipFree(ctx->d_denoise);
    if (ctx->d_temporal) (void)hipFree(ctx->d_temporal);
    if (ctx->d_bvh) (void)hipFree(ctx->d_bvh);
    if (ctx->d_bvh_bins) (void)hipFree(ctx->d_bvh_bins);
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

namespace {

/* One WCPT_OPTION_*: the field it sets, the values it accepts, what acceptance does to the cached frame preparation
 * and the noun of its refusal ("<noun> <value>"). The options that prepare_tri_records / render_validate read (record
 * formats, stack-entry layout, the cache itself) invalidate their cached frame preparation once accepted:
 * ctx->generation++ there only, so a host that sets the other options every frame keeps the cache. */
enum Bump { kBumpNever, kBumpOnChange, kBumpAlways };
struct OptionRow {
    int option;
    int wcpt_context::*field;
    int lo, hi;       /* the accepted range; lo > hi: a boolean, any value, normalised to 0 / 1 */
    Bump bump;
    const char* noun;
};
constexpr int kBool = 1; /* lo of a boolean row (hi 0) */
const OptionRow kOptions[] = {
    {WCPT_OPTION_SORT_RAYS, &wcpt_context::sort_rays, kBool, 0, kBumpNever, ""},
    {WCPT_OPTION_WF_REFILL, &wcpt_context::wf_refill, 1, 64, kBumpNever, "refill threshold"},
    {WCPT_OPTION_WF_PIPES, &wcpt_context::wf_pipes, 0, wcpt::kWfMaxPipes, kBumpNever, "pipelines"},
    {WCPT_OPTION_MK_TILE_ORDER, &wcpt_context::mk_tile_order, 0, 6, kBumpNever, "tile order"},
    {WCPT_OPTION_FRAME_OVERLAP, &wcpt_context::frame_overlap, 0, 2, kBumpNever, "frame overlap"},
    {WCPT_OPTION_PACKED_REFS, &wcpt_context::packed_refs, kBool, 0, kBumpAlways, ""},
    {WCPT_OPTION_PAIR_RECORDS, &wcpt_context::pair_records, -1, 1, kBumpAlways, "pair records"},
    {WCPT_OPTION_TRIANGLE_CACHE, &wcpt_context::tri_cache, kBool, 0, kBumpAlways, ""},
    {WCPT_OPTION_PRIMARY_CACHE, &wcpt_context::prim_cache, 0, 1, kBumpAlways, "primary cache"},
    {WCPT_OPTION_MK_SPLIT, &wcpt_context::mk_split, wcpt::kMkSplitAuto, wcpt::kMkSplitMaxCut, kBumpNever, "megakernel split"},
    /* the draw's table flag is part of the cached frame preparation */
    {WCPT_OPTION_MK_TINY_TREE, &wcpt_context::mk_tiny_tree, wcpt::kMkTinyAuto, 1, kBumpOnChange, "megakernel tiny tree"},
    /* the primary cache's key holds the generation: a record belongs to the arithmetic that found it */
    {WCPT_OPTION_ARITH, &wcpt_context::arith, WCPT_ARITH_EXACT, WCPT_ARITH_FAST, kBumpAlways, "arithmetic mode"},
    {WCPT_OPTION_DIAGNOSTICS, &wcpt_context::diagnostics, kBool, 0, kBumpNever, ""},
    {WCPT_OPTION_WF_PERSIST, &wcpt_context::wf_persist, -1, 1, kBumpNever, "wavefront persist"},
    {WCPT_OPTION_WF_FETCH, &wcpt_context::wf_fetch, -1, 1, kBumpNever, "wavefront fetch rounds"},
    {WCPT_OPTION_PROFILE_REGION, &wcpt_context::profile_region, kBool, 0, kBumpNever, ""},
    {WCPT_OPTION_STACK, &wcpt_context::stack_kind, 0, 1, kBumpNever, "stack kind"},
    {WCPT_OPTION_GATHER_FRAME_ROWS, &wcpt_context::gather_frame_rows, 0, 1, kBumpNever, "gather frame rows"},
};

} // namespace

int wcpt_set_option(wcpt_context* ctx, int option, int value)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    /* the options the table does not describe whole */
    if (option == WCPT_OPTION_WF_STACK) { /* three values, no range */
        if (value != 10 && value != 16 && value != 24)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "wavefront LDS stack %d (10, 16 or 24)", value);
        ctx->wf_stack = value;
        return WCPT_SUCCESS;
    }
    if (option == WCPT_OPTION_PROFILE_REGION && ctx->profiling)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "profile region: set outside profiling");
    for (const OptionRow& o : kOptions) {
        if (o.option != option) continue;
        const bool boolean = o.lo > o.hi;
        if (!boolean && (value < o.lo || value > o.hi)) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s %d", o.noun, value);
        const int v = boolean ? (value ? 1 : 0) : value;
        if (o.bump == kBumpAlways || (o.bump == kBumpOnChange && ctx->*o.field != v)) ctx->generation++;
        ctx->*o.field = v;
        if (option == WCPT_OPTION_WF_REFILL) ctx->wf_refill_persist = v; /* an explicit value governs both traces */
        return WCPT_SUCCESS;
    }
    return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "unknown option %d", option);
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

/* no bind: reading the record must not join the pipelines it describes */
int wcpt_wf_last_plan(wcpt_context* ctx, wcpt_wf_plan_info* out)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    if (!out) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null plan record");
    *out = ctx->wf.last;
    return WCPT_SUCCESS;
}

int wcpt_sync(wcpt_context* ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return read_status(ctx);
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

} /* extern "C" */
