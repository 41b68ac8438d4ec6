/*
 * wcpt_screen.hip — C-ABI runtime, the output image (CreateScreen / Resize): the frame's size and the rows of it the
 * context holds (screen_layout.h states every rule; here are their messages and the device's part), an external image,
 * the gather output, readback and upload, and the display step (wcpt_composite, wcpt_composite_bloom,
 * wcpt_composite_denoise, wcpt_composite_temporal).
 */
#include "wcpt_context.h"
#include "wcpt_bloom.h"
#include "wcpt_denoise.h"
#include "wcpt_temporal.h"

using namespace wcpt::rt;

namespace {

/* An image of `bytes` bytes: the external one must hold them, the context's own is grown to them. */
int alloc_image(wcpt_context* ctx, uint64_t bytes)
{
    if (ctx->external_bytes) {
        if (bytes > ctx->external_bytes)
            return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image of %llu bytes < %llu needed",
                             (unsigned long long)ctx->external_bytes, (unsigned long long)bytes);
    } else if (bytes > ctx->image_bytes_cap) {
        ctx->image = nullptr;
        const int rc = grow(ctx, ctx->own_image, ctx->image_bytes_cap, bytes, bytes, "hipMalloc(image)");
        if (rc) return rc;
        ctx->image = ctx->own_image;
    }
    return WCPT_SUCCESS;
}

uint64_t layout_bytes(const wcpt::ScreenLayout& l) { return (uint64_t)l.width * l.rows * 16ull; }

/* The context brought to the layout `next`, after the caller's sync. What kind of rows it holds changes at once; the
 * frame's size and the rows change when the image holds them (with no screen yet there is no image: the rows are held
 * for the first screen's resize rule). `zero`: the context's own image then starts as zeros -- the reference's storage
 * image starts undefined (PathTracingRenderer.jai:345-385) and its editor's first frame already blends with it
 * (renderedFramesCount 1, editor.jai:149-152). */
int apply_layout(wcpt_context* ctx, const wcpt::ScreenLayout& next, bool zero)
{
    wcpt::ScreenLayout& l = ctx->layout;
    ctx->temporal.valid = false; /* wcpt_composite_temporal's history belongs to the layout it was made in */
    l.sharded = next.sharded;
    l.stripe = next.stripe;
    l.period = next.period;
    if (next.height) {
        const int rc = alloc_image(ctx, layout_bytes(next));
        if (rc) return rc;
    }
    l = next;
    if (zero && !ctx->external_bytes) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->image, 0, layout_bytes(next), ctx->stream), "hipMemsetAsync(image)");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    return WCPT_SUCCESS;
}

/* wcpt_set_row_range and wcpt_set_row_stripes name the context's rows: they are its rows from the call on, also when
 * the image then cannot be brought to hold them and the call fails. An external image is the exception: the context
 * cannot grow it, and a render of rows it does not hold would write past the caller's memory, so rows it cannot hold
 * are refused before anything changes. */
int apply_named_rows(wcpt_context* ctx, const wcpt::ScreenLayout& next)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (ctx->external_bytes && next.height) {
        const int rc = alloc_image(ctx, layout_bytes(next));
        if (rc) return rc;
    }
    ctx->layout.y0 = next.y0;
    ctx->layout.rows = next.rows;
    return apply_layout(ctx, next, false);
}

} // namespace

/* CreateScreen of one row block in one step: the frame's size and the context's block [y0, y0 + rows) are set
 * together, so only the block is allocated (and zeroed), whatever the previous frame's size was. */
int wcpt::set_frame_block(wcpt_context* ctx, uint32_t width, uint32_t height, uint32_t y0, uint32_t rows, uint32_t stripe,
                          uint32_t period)
{
    const int rc = bind(ctx);
    if (rc) return rc;
    wcpt::ScreenLayout next;
    switch (wcpt::layout_frame_block(ctx->layout, width, height, y0, rows, stripe, period, next)) {
    case wcpt::kLayoutOk: break;
    case wcpt::kLayoutBadStripes:
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row stripes of %u rows every %u rows", stripe, period);
    default:
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%u rows from row %u (stripes %u / %u) in a %ux%u frame", rows,
                         y0, stripe, period, width, height);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return apply_layout(ctx, next, true);
}

extern "C" {

/* ---- image -------------------------------------------------------------------------------------- */
int wcpt_create_screen(wcpt_context* ctx, uint32_t width, uint32_t height)
{
    const int rc = bind(ctx);
    if (rc) return rc;
    wcpt::ScreenLayout next;
    if (wcpt::layout_resize(ctx->layout, width, height, next) != wcpt::kLayoutOk)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "zero-sized screen");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return apply_layout(ctx, next, true);
}

int wcpt_resize(wcpt_context* ctx, uint32_t width, uint32_t height)
{
    return wcpt_create_screen(ctx, width, height); /* Resize = DestroyScreen + CreateScreen (:393-397) */
}

int wcpt_set_row_range(wcpt_context* ctx, uint32_t y0, uint32_t rows)
{
    const int rc = bind(ctx);
    if (rc) return rc;
    wcpt::ScreenLayout next;
    if (wcpt::layout_set_range(ctx->layout, y0, rows, next) != wcpt::kLayoutOk)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row range [%u,%u) outside frame height %u", y0, y0 + rows,
                         ctx->layout.height);
    return rows ? apply_named_rows(ctx, next) : apply_layout(ctx, next, false);
}

int wcpt_set_row_stripes(wcpt_context* ctx, uint32_t y_first, uint32_t rows, uint32_t stripe, uint32_t period)
{
    if (stripe == 0) return wcpt_set_row_range(ctx, y_first, rows);
    const int rc = bind(ctx);
    if (rc) return rc;
    wcpt::ScreenLayout next;
    switch (wcpt::layout_set_stripes(ctx->layout, y_first, rows, stripe, period, next)) {
    case wcpt::kLayoutOk: break;
    case wcpt::kLayoutPastFrame:
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row stripes reach row %llu of a frame of height %u",
                         (unsigned long long)wcpt::layout_last_row(next), ctx->layout.height);
    case wcpt::kLayoutPastRow32: return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "row stripes past row 2^32");
    default:
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%u rows in stripes of %u rows every %u rows", rows, stripe,
                         period);
    }
    return apply_named_rows(ctx, next);
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
        if (ctx->layout.width && ctx->layout.rows) return alloc_image(ctx, layout_bytes(ctx->layout));
        return WCPT_SUCCESS;
    }
    if (bytes == 0) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image of 0 bytes");
    if (device_ptr & 15u) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image needs 16-byte alignment");
    if (ctx->layout.width && layout_bytes(ctx->layout) > bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "external image too small for %ux%u", ctx->layout.width,
                         ctx->layout.rows);
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
    if (!wcpt::payload_format_valid(channels))
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
    const uint64_t have = layout_bytes(ctx->layout);
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
    const uint64_t pixels = (uint64_t)ctx->layout.width * ctx->layout.rows;
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
    const uint64_t pixels = (uint64_t)ctx->layout.width * ctx->layout.rows;
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
    if (ctx->layout.sharded)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bloom needs the whole frame: the context holds %u of %u rows",
                         ctx->layout.rows, ctx->layout.height);
    uint32_t lw[WCPT_BLOOM_MAX_LEVELS], lh[WCPT_BLOOM_MAX_LEVELS];
    const uint32_t levels = wcpt_bloom_plan(ctx->layout.width, ctx->layout.height, p->levels, lw, lh);
    if (levels == 0)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bloom of %u levels (2..12) on a %ux%u frame (2 levels need 4x4)",
                         p->levels, ctx->layout.width, ctx->layout.height);
    /* both pyramids in one allocation, the down levels first; every level is written before it is read in each call, so
     * a new screen size only moves the levels */
    const uint64_t texels = wcpt::bloom_pyramid_texels(levels, lw, lh);
    const uint64_t bytes = 2ull * texels * sizeof(float4);
    if (bytes > ctx->bloom_bytes) {
        rc = grow(ctx, ctx->d_bloom, ctx->bloom_bytes, bytes, bytes, "hipMalloc(bloom pyramids)");
        if (rc) return rc;
    }
    HIP_TRY(ctx, wcpt::launch_composite_bloom(ctx->image, ctx->layout.width, ctx->layout.height, p->threshold, p->knee,
                                              levels, lw, lh, ctx->d_bloom, ctx->d_bloom + texels,
                                              reinterpret_cast<void*>(dst), format == WCPT_COMPOSITE_RGBA8, ctx->stream),
            "bloom composite launch");
    return WCPT_SUCCESS;
}

namespace {

/* What wcpt_composite_denoise and wcpt_composite_temporal check about the denoise parameters and the guide: the context
 * holds the whole frame, and the guide's memory holds a record per pixel. */
int check_denoise_params(wcpt_context* ctx, const wcpt_denoise_params* p)
{
    if (!p) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null denoise parameters");
    if (!wcpt_denoise_params_ok(p->iterations, p->sigma_color, p->sigma_normal, p->sigma_depth))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT,
                         "denoise of %u iterations (1..6), sigma colour %g (> 0), normal %g, depth %g (finite, > 0)",
                         p->iterations, (double)p->sigma_color, (double)p->sigma_normal, (double)p->sigma_depth);
    return WCPT_SUCCESS;
}

int check_guide(wcpt_context* ctx, uint64_t guide, uint64_t guide_bytes, const char* who)
{
    if (ctx->layout.sharded)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s needs the whole frame: the context holds %u of %u rows", who,
                         ctx->layout.rows, ctx->layout.height);
    const uint64_t need = (uint64_t)ctx->layout.width * ctx->layout.height * WCPT_DENOISE_RECORD_BYTES;
    if (!guide || (guide & 15u) || guide_bytes < need)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s guide: %llu bytes at a null or misaligned address, %llu needed",
                         who, (unsigned long long)guide_bytes, (unsigned long long)need);
    uint64_t off = 0;
    Buffer* b = buffer_at(ctx, guide, off);
    if (b && off + need > b->bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "%s guide holds %llu bytes, %llu needed", who,
                         (unsigned long long)(b->bytes - off), (unsigned long long)need);
    return WCPT_SUCCESS;
}

/* two images and the packed guide in one allocation; every part is written before it is read in each call, so a new
 * screen size only moves the parts */
int grow_denoise_scratch(wcpt_context* ctx)
{
    const uint64_t bytes = wcpt::denoise_scratch_bytes(ctx->layout.width, ctx->layout.height);
    if (bytes > ctx->denoise_bytes) return grow(ctx, ctx->d_denoise, ctx->denoise_bytes, bytes, bytes, "hipMalloc(denoise scratch)");
    return WCPT_SUCCESS;
}

} // namespace

int wcpt_composite_denoise(wcpt_context* ctx, uint64_t guide, uint64_t guide_bytes, uint64_t dst, int format,
                           const wcpt_denoise_params* p)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = check_composite_target(ctx, dst, format);
    if (rc) return rc;
    rc = check_denoise_params(ctx, p);
    if (rc) return rc;
    rc = check_guide(ctx, guide, guide_bytes, "denoise");
    if (rc) return rc;
    rc = grow_denoise_scratch(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, wcpt::launch_composite_denoise(ctx->image, reinterpret_cast<const void*>(guide), ctx->layout.width,
                                                ctx->layout.height, p->iterations, p->sigma_color, p->sigma_normal,
                                                p->sigma_depth, ctx->d_denoise, reinterpret_cast<void*>(dst),
                                                format == WCPT_COMPOSITE_RGBA8, ctx->stream),
            "denoise composite launch");
    return WCPT_SUCCESS;
}

int wcpt_composite_temporal(wcpt_context* ctx, const wcpt_scene_data* scene, uint32_t frames, int restart, uint64_t guide,
                            uint64_t guide_bytes, uint64_t dst, int format, const wcpt_temporal_params* t,
                            const wcpt_denoise_params* d)
{
    static_assert(WCPT_TEMPORAL_RECORD_BYTES == WCPT_DENOISE_RECORD_BYTES, "one guide for both stages");
    int rc = bind(ctx);
    if (rc) return rc;
    rc = check_composite_target(ctx, dst, format);
    if (rc) return rc;
    if (!scene || !t) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "null temporal scene or parameters");
    if (!wcpt_temporal_params_ok(t->max_history, t->normal_min, t->depth_tol))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT,
                         "temporal history of %u samples (1..65536), normal_min %g (-1..1), depth_tol %g (finite, > 0)",
                         t->max_history, (double)t->normal_min, (double)t->depth_tol);
    if (frames == 0) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "temporal: an accumulation image of 0 frames");
    if (d) {
        rc = check_denoise_params(ctx, d);
        if (rc) return rc;
    }
    rc = check_guide(ctx, guide, guide_bytes, "temporal");
    if (rc) return rc;
    const uint32_t width = ctx->layout.width, height = ctx->layout.height;
    wcpt_temporal_camera cam;
    if (!wcpt_temporal_make_camera(scene->inverseProjection, scene->inverseView, scene->position, width, height, &cam))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT,
                         "temporal: a singular camera matrix, or not a plain perspective (a corner pixel misses its centre)");
    /* every part of a side is written before it is read, and the history does not outlive a layout (apply_layout) */
    const uint64_t bytes = wcpt::temporal_scratch_bytes(width, height);
    if (bytes > ctx->temporal_bytes) {
        ctx->temporal.valid = false;
        rc = grow(ctx, ctx->d_temporal, ctx->temporal_bytes, bytes, bytes, "hipMalloc(temporal scratch)");
        if (rc) return rc;
    }
    if (d) {
        rc = grow_denoise_scratch(ctx);
        if (rc) return rc;
    }
    wcpt_context::TemporalState& st = ctx->temporal;
    const wcpt_temporal_consts k = wcpt_temporal_make_consts(t->max_history, t->normal_min, t->depth_tol);
    const int store = d ? 0 : (format == WCPT_COMPOSITE_RGBA8 ? 2 : 1);
    void* const out = reinterpret_cast<void*>(dst);
    if (restart || !st.valid) {
        wcpt_temporal_camera hist_cam;
        memcpy(hist_cam.F, st.F, sizeof(st.F));
        memcpy(hist_cam.position, st.position, sizeof(st.position));
        HIP_TRY(ctx, wcpt::launch_temporal_reproject(ctx->image, reinterpret_cast<const void*>(guide), width, height,
                                                     cam.position, st.valid, hist_cam, st.side, (float)frames, k,
                                                     ctx->d_temporal, out, store, ctx->stream),
                "temporal reproject launch");
        st.side = st.valid ? (st.side ^ 1u) : ((st.side & 1u) ^ 1u);
        st.valid = true;
        memcpy(st.F, cam.F, sizeof(st.F));
        memcpy(st.position, cam.position, sizeof(st.position));
    } else {
        HIP_TRY(ctx, wcpt::launch_temporal_blend(ctx->image, width, height, st.side, (float)frames, k, ctx->d_temporal, out,
                                                 store, ctx->stream),
                "temporal blend launch");
    }
    if (d)
        HIP_TRY(ctx, wcpt::launch_composite_denoise(wcpt::temporal_hist_image(ctx->d_temporal, width, height, st.side),
                                                    reinterpret_cast<const void*>(guide), width, height, d->iterations,
                                                    d->sigma_color, d->sigma_normal, d->sigma_depth, ctx->d_denoise, out,
                                                    format == WCPT_COMPOSITE_RGBA8, ctx->stream),
                "temporal denoise launch");
    return WCPT_SUCCESS;
}

int wcpt_temporal_reset(wcpt_context* ctx)
{
    if (!ctx) return set_error(nullptr, WCPT_ERROR_INVALID_HANDLE, "null context");
    ctx->temporal.valid = false;
    return WCPT_SUCCESS;
}

int wcpt_image_upload(wcpt_context* ctx, const float* src, uint64_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const uint64_t have = layout_bytes(ctx->layout);
    if (!ctx->image) return set_error(ctx, WCPT_ERROR_NO_SCREEN, "no output image");
    if (!src || bytes > have) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "image upload size");
    HIP_TRY(ctx, hipMemcpyAsync(ctx->image, src, bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(image)");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return WCPT_SUCCESS;
}

} /* extern "C" */
