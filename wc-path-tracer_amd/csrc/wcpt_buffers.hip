/*
 * wcpt_buffers.hip — C-ABI runtime, device buffers (BufferManager.jai): alloc / upload / download / free, the host
 * copies that let a render read its draw commands without a device round trip, and the BVH builds and the refit on
 * the device, which write the context's buffers.
 */
#include "wcpt_context.h"
#include "bvh_sah.h"
#include "bvh_refit.h"

using namespace wcpt::rt;

namespace {

/* Device buffers are handed out at base address = 32 (mod 64) (a 64-byte-aligned allocation + 32). A BVH
 * node is 32 bytes and the two children of an interior node sit at indices (2k+1, 2k+2) (the builder appends
 * them as a pair after the root, PathTracingRenderer.jai:196-202), so with this base every child pair the
 * traversal fetches together occupies exactly one 64-byte cache line instead of straddling two. Scattered
 * line visits are what bounds traversal (tools/gather_bench.hip). 32-byte alignment is enough for every
 * other buffer type (largest access: 16 bytes). */
constexpr uint64_t kBufferSkew = 32;

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

/* wcpt_bvh_build_device and wcpt_bvh_build_sah_device: one set of argument checks, one scratch allocation (the two
 * builds are synchronous, so they take turns in it), one way of telling the runtime's caches what was written */
int bvh_build_on_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                        uint32_t index_count, wcpt_buffer nodes, uint32_t* nodes_used, bool sah)
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
    const uint64_t need = sah ? wcpt::bvh_sah_scratch_bytes(index_count) : wcpt::bvh_build_scratch_bytes(index_count);
    if (ctx->bvh_bytes < need) {
        rc = grow(ctx, ctx->d_bvh, ctx->bvh_bytes, need, need, "hipMalloc(bvh build scratch)");
        if (rc) return rc;
    }
    uint32_t status = 0, used = 0;
    if (sah) {
        HIP_TRY(ctx, wcpt::bvh_build_sah_device(static_cast<const float*>(bv->ptr), vertex_count, static_cast<uint32_t*>(bi->ptr),
                                                index_count, bn->ptr, ctx->d_bvh, &ctx->d_bvh_bins, &ctx->bvh_bins_bytes, &status,
                                                &used, ctx->stream), "bvh sah build");
    } else {
        HIP_TRY(ctx, wcpt::bvh_build_device(static_cast<const float*>(bv->ptr), vertex_count, static_cast<uint32_t*>(bi->ptr),
                                            index_count, bn->ptr, ctx->d_bvh, &status, &used, ctx->stream), "bvh build");
    }
    if (status & wcpt::kBvhBadIndex)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: an index is not below vertex_count %u", vertex_count);
    if (status & wcpt::kBvhNotFinite)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh build: a referenced coordinate is not finite");
    if (status & wcpt::kSahCentroidNotFinite)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh sah build: a triangle's centroid 0.5f * (lo + hi) is not finite");
    if (status & wcpt::kSahBadScale)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh sah build: a node's centroid extent, or 16 / extent, is not finite");
    if (status & wcpt::kSahNoFiniteCost)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT,
                         "bvh sah build: a node of more than 8 triangles has no finite split cost (its box overflows binary32)");
    /* a write of both buffers, as wcpt_buffer_upload's: the host copies no longer know the range, and everything keyed
     * on the generations (triangle records, leaf scan, tiny-tree flag, frame preparation, primary cache) is re-learned */
    shadow_forget(*bi, 0, (uint64_t)index_count * 4ull);
    shadow_forget(*bn, 0, (uint64_t)used * sizeof(wcpt_node));
    bi->generation = ++ctx->generation;
    bn->generation = ++ctx->generation;
    *nodes_used = used;
    return WCPT_SUCCESS;
}

} // namespace

/* True when the host copy holds every byte of [offset, offset + bytes). */
bool wcpt::rt::shadow_known(const Buffer& b, uint64_t offset, uint64_t bytes)
{
    if (b.shadow.size() != b.bytes || bytes == 0 || offset + bytes > b.bytes) return false;
    for (uint64_t c = offset / kShadowChunk; c < (offset + bytes + kShadowChunk - 1) / kShadowChunk; c++)
        if (c >= b.known.size() || !b.known[c]) return false;
    return true;
}

extern "C" {

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

/* ---- BVH build on the device (pt_bvh_build.hip, pt_bvh_sah.hip) ------------------------------------ */
int wcpt_bvh_build_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                          uint32_t index_count, wcpt_buffer nodes, uint32_t* nodes_used)
{
    return bvh_build_on_device(ctx, vertices, vertex_count, indices, index_count, nodes, nodes_used, false);
}

int wcpt_bvh_build_sah_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                              uint32_t index_count, wcpt_buffer nodes, uint32_t* nodes_used)
{
    return bvh_build_on_device(ctx, vertices, vertex_count, indices, index_count, nodes, nodes_used, true);
}

/* ---- BVH refit on the device (pt_bvh_refit.hip) ------------------------------------------------------ */
/* wcpt_bvh_refit_device: the builds' argument checks and scratch, what bvh_refit.h refuses, and the caches told of a
 * write of the nodes and -- the reason to refit -- of the vertices, however those got into their buffer */
int wcpt_bvh_refit_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                          uint32_t index_count, wcpt_buffer nodes, uint32_t nodes_used)
{
    int rc = bind(ctx);
    if (rc) return rc;
    Buffer* bv = find_buffer(ctx, vertices);
    Buffer* bi = find_buffer(ctx, indices);
    Buffer* bn = find_buffer(ctx, nodes);
    if (!bv || !bi || !bn) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh refit: unknown buffer handle");
    if (bv == bi || bv == bn || bi == bn) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh refit: the three buffers must differ");
    if ((uint64_t)vertex_count * 12ull > bv->bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh refit: %u vertices exceed the vertex buffer (%llu bytes)",
                         vertex_count, (unsigned long long)bv->bytes);
    if ((uint64_t)index_count * 4ull > bi->bytes)
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh refit: %u indices exceed the index buffer (%llu bytes)",
                         index_count, (unsigned long long)bi->bytes);
    if (nodes_used == 0u || nodes_used > bn->bytes / sizeof(wcpt_node))
        return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh refit: nodes_used %u is zero or exceeds the node buffer (%llu nodes)",
                         nodes_used, (unsigned long long)(bn->bytes / sizeof(wcpt_node)));
    const uint64_t need = wcpt::bvh_refit_scratch_bytes(nodes_used);
    if (ctx->bvh_bytes < need) {
        rc = grow(ctx, ctx->d_bvh, ctx->bvh_bytes, need, need, "hipMalloc(bvh refit scratch)");
        if (rc) return rc;
    }
    uint32_t status = 0;
    HIP_TRY(ctx, wcpt::bvh_refit_device(static_cast<const float*>(bv->ptr), vertex_count, static_cast<const uint32_t*>(bi->ptr),
                                        index_count, bn->ptr, nodes_used, ctx->d_bvh, &status, ctx->stream), "bvh refit");
    if (status) return set_error(ctx, WCPT_ERROR_INVALID_ARGUMENT, "bvh refit: %s", wcpt::refit_refusal(status));
    shadow_forget(*bv, 0, (uint64_t)vertex_count * 12ull);
    shadow_forget(*bn, 0, (uint64_t)nodes_used * sizeof(wcpt_node));
    bv->generation = ++ctx->generation;
    bn->generation = ++ctx->generation;
    return WCPT_SUCCESS;
}

} /* extern "C" */
