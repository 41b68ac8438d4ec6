/*
 * pt_denoise.hip — the guided a-trous denoise in front of the display step (the rule, the guide's packing and every
 * operation's order in wcpt_denoise.h): a pack pass that turns the caller's 48-byte primary-hit records into two planes of
 * 16-byte guide rows, then one launch per iteration over float4 images, the last of which applies gamma and the PBR
 * Neutral tonemap and stores rgba32f or RGBA8.
 *
 * 1 + iterations launches, all on the caller's stream; an iteration reads what the one before wrote, so stream order is
 * the only synchronisation. The first iteration reads the accumulation image, which is never written; the others
 * ping-pong between two images of the context's scratch. One pixel per lane, 32x8 pixels per 256-thread block as in
 * bloom_display_kernel, so a wave's loads of a tap are two contiguous row pieces of 512 bytes in each plane. A lane
 * reads the tap's first guide row and compares the key, then the second row and compares the kind, and only then
 * loads the colour: a skipped tap contributes nothing, so the order of the loads does not change the bits.
 *
 * The display step is fused into the last iteration. Built both ways and measured in alternating processes
 * (profiles/denoise_ab.log): with a display launch of its own (wcpt_composite's kernel after the last iteration) a call
 * is 19 to 22 us slower at 1920x1080 -- one more float4 image written and read, and one more launch -- at the same bits.
 *
 * Bound: the taps, not the streamed bytes. At 1920x1080 an iteration takes 170 to 181 us whatever its step (1 to 16)
 * against 25 to 29 us for the pack pass, which streams more bytes than an iteration's compulsory traffic (80 against 64
 * bytes per pixel): a pixel's 25 taps read 1200 bytes through the CU's L1 and each costs an exponential, two squared
 * distances and a plane distance, and since the time does not grow with the step it is not the L1 hit rate that bounds it
 * but the taps' issue: some 52 million of them per iteration. Five iterations are 0.89 ms per call on c2 beside 17.6 us for
 * wcpt_composite, 91 us for wcpt_composite_bloom and the 0.24-0.35 ms frame. As for the bloom pyramid
 * the taps read global memory, not an LDS tile; staging was not built here.
 */
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "wcpt_denoise.h"

namespace wcpt {
namespace dev {

struct DenoiseImage {
    const float4* __restrict__ texels;
    int w;
    __device__ void operator()(int x, int y, float rgba[4]) const
    {
        const float4 t = texels[(size_t)y * (size_t)w + (size_t)x];
        rgba[0] = t.x;
        rgba[1] = t.y;
        rgba[2] = t.z;
        rgba[3] = t.w;
    }
};

/* the packed guide: a plane of first rows, a plane of second rows */
struct DenoiseGuide {
    const uint4* __restrict__ row0;
    const uint4* __restrict__ row1;
    int w;
    __device__ static void get(const uint4* plane, size_t i, uint32_t r[4])
    {
        const uint4 v = plane[i];
        r[0] = v.x;
        r[1] = v.y;
        r[2] = v.z;
        r[3] = v.w;
    }
    __device__ void first(int x, int y, uint32_t r[4]) const { get(row0, (size_t)y * (size_t)w + (size_t)x, r); }
    __device__ void second(int x, int y, uint32_t r[4]) const { get(row1, (size_t)y * (size_t)w + (size_t)x, r); }
};

__global__ __launch_bounds__(256) void denoise_pack_kernel(const uint4* __restrict__ records, const uint64_t pixels,
                                                           const float sigma_depth, uint4* __restrict__ row0,
                                                           uint4* __restrict__ row1)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const uint4 a = records[3 * i], b = records[3 * i + 1], c = records[3 * i + 2];
    const uint32_t rec[WCPT_DENOISE_RECORD_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    uint32_t r0[4], r1[4];
    wcpt_denoise_pack(rec, sigma_depth, r0, r1);
    row0[i] = make_uint4(r0[0], r0[1], r0[2], r0[3]);
    row1[i] = make_uint4(r1[0], r1[1], r1[2], r1[3]);
}

enum DenoiseStore { kDenoiseImage, kDenoiseRgba32f, kDenoiseRgba8 };

template <int STORE>
__global__ __launch_bounds__(256) void denoise_iteration_kernel(const float4* __restrict__ src, const uint4* __restrict__ row0,
                                                                const uint4* __restrict__ row1, const int w, const int h,
                                                                const int step, const wcpt_denoise_consts k,
                                                                const uint32_t blocks_x, float4* __restrict__ out32,
                                                                uchar4* __restrict__ out8)
{
    const uint32_t bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
    const int x = (int)(bx * 32u + (threadIdx.x & 31u)), y = (int)(by * 8u + (threadIdx.x >> 5));
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    float f[4];
    wcpt_denoise_texel(DenoiseImage{src, w}, DenoiseGuide{row0, row1, w}, w, h, x, y, step, k, f);
    if (STORE == kDenoiseImage) {
        out32[i] = make_float4(f[0], f[1], f[2], f[3]);
        return;
    }
    float o[4];
    wcpt_composite_texel(f, o);
    if (STORE == kDenoiseRgba8)
        out8[i] = make_uchar4(wcpt_unorm8(o[0]), wcpt_unorm8(o[1]), wcpt_unorm8(o[2]), 255);
    else
        out32[i] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace dev

uint64_t denoise_scratch_bytes(uint32_t width, uint32_t height)
{
    return (uint64_t)width * height * WCPT_DENOISE_SCRATCH_BYTES;
}

hipError_t launch_composite_denoise(const float4* img, const void* records, uint32_t width, uint32_t height,
                                    uint32_t iterations, float sigma_color, float sigma_normal, float sigma_depth,
                                    void* scratch, void* dst, bool rgba8, hipStream_t stream)
{
    if (iterations < WCPT_DENOISE_MIN_ITERATIONS || iterations > WCPT_DENOISE_MAX_ITERATIONS || width > 0x7FFFFFFFu ||
        height > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    const uint64_t pixels = (uint64_t)width * height;
    const uint64_t nx = ((uint64_t)width + 31u) / 32u, ny = ((uint64_t)height + 7u) / 8u;
    const uint64_t pack_blocks = (pixels + 255u) / 256u;
    if (pixels == 0 || nx * ny > 0x7FFFFFFFull || pack_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const wcpt_denoise_consts k = wcpt_denoise_make_consts(sigma_color, sigma_normal, sigma_depth);
    /* the scratch: two float4 images, then the guide's two planes */
    float4* const image[2] = {static_cast<float4*>(scratch), static_cast<float4*>(scratch) + pixels};
    uint4* const row0 = reinterpret_cast<uint4*>(image[1] + pixels);
    uint4* const row1 = row0 + pixels;
    hipLaunchKernelGGL(dev::denoise_pack_kernel, dim3((uint32_t)pack_blocks), dim3(256), 0, stream,
                       static_cast<const uint4*>(records), pixels, sigma_depth, row0, row1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((uint32_t)(nx * ny)), block(256);
    const int w = (int)width, h = (int)height;
    const float4* src = img;
    for (uint32_t it = 0; it < iterations; it++) {
        const int step = 1 << it;
        if (it + 1 < iterations) {
            float4* const out = image[it & 1u];
            hipLaunchKernelGGL(dev::denoise_iteration_kernel<dev::kDenoiseImage>, grid, block, 0, stream, src, row0, row1, w, h,
                               step, k, (uint32_t)nx, out, nullptr);
            src = out;
        } else if (rgba8) {
            hipLaunchKernelGGL(dev::denoise_iteration_kernel<dev::kDenoiseRgba8>, grid, block, 0, stream, src, row0, row1, w, h,
                               step, k, (uint32_t)nx, nullptr, static_cast<uchar4*>(dst));
        } else {
            hipLaunchKernelGGL(dev::denoise_iteration_kernel<dev::kDenoiseRgba32f>, grid, block, 0, stream, src, row0, row1, w,
                               h, step, k, (uint32_t)nx, static_cast<float4*>(dst), nullptr);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace wcpt
