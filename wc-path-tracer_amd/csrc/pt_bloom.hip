/*
 * pt_bloom.hip — the bloom pyramid of the display step (bloom.comp, composite.comp:44-45; arithmetic and chain in
 * wcpt_bloom.h): prefilter, downsample and upsample passes over float4 levels, and the display store that adds the
 * sampled pyramid to the accumulation image before gamma and the PBR Neutral tonemap (rgba32f or RGBA8).
 *
 * One launch per step, 2L launches for L levels, all on the caller's stream; a step reads what the step before wrote,
 * so stream order is the only synchronisation. One output texel per thread, 16x16 texels per 256-thread block (32x8
 * pixels in the display store, whose rows are 16 B per pixel wide): the 13 (box) or 9 (tent) bilinear taps of
 * neighbouring texels overlap almost entirely, so the block's source footprint (about 36x36 texels of a level twice
 * the size, 20 KB) is fetched from memory once and the taps' 16-byte texel loads are served by the CU's L1.
 *
 * Bound: streaming for the two full-size passes (the image is read by the prefilter and by the display store), latency
 * for the rest: of the twelve launches of a 1920x1080 frame with six levels, the eight from D[2] down to D[5] and back up
 * to U[1] take 4.5 to 5 us each whatever their level's size (30x16 to 480x270). Measured (profiles/bloom_ab.log): 91 us
 * per call against 17 us for wcpt_composite alone. Staging each block's footprint in LDS and running the small levels
 * in one launch of one workgroup were both built, gave the same bits and were slower ("Tried and
 * rejected"), so the taps read global memory through L1 and every step is its own launch.
 */
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "wcpt_bloom.h"

namespace wcpt {
namespace dev {

/* A level (or the accumulation image) in global memory */
struct GlobalTexture {
    const float4* __restrict__ texels;
    int w;
    __device__ void operator()(int x, int y, float rgb[3]) const
    {
        const float4 t = texels[(size_t)y * (size_t)w + (size_t)x];
        rgb[0] = t.x;
        rgb[1] = t.y;
        rgb[2] = t.z;
    }
};

enum BloomMode { kBloomPrefilter, kBloomDownsample, kBloomUpsample };

struct BloomStep {
    const float4* src;      /* the texture the taps read: the image, D[l-1], or the level below (D[L-1] or U[l+1]) */
    const float4* existing; /* kBloomUpsample: D[l], same size as dst */
    float4* dst;
    wcpt_bloom_size ss, ds; /* sizes of src and dst */
    wcpt_bloom_curve curve; /* kBloomPrefilter */
    uint32_t blocks_x;      /* blocks per row of blocks */
};

template <int MODE>
__global__ __launch_bounds__(256) void bloom_step_kernel(const BloomStep s)
{
    const uint32_t bx = blockIdx.x % s.blocks_x, by = blockIdx.x / s.blocks_x;
    const int x = (int)(bx * 16u + (threadIdx.x & 15u)), y = (int)(by * 16u + (threadIdx.x >> 4));
    if (x >= s.ds.w || y >= s.ds.h) return;
    const GlobalTexture tex{s.src, s.ss.w};
    const size_t i = (size_t)y * (size_t)s.ds.w + (size_t)x;
    float o[3];
    if (MODE == kBloomPrefilter) {
        wcpt_bloom_prefilter_texel(tex, s.ss, s.ds, x, y, s.curve, o);
    } else if (MODE == kBloomDownsample) {
        wcpt_bloom_downsample_texel(tex, s.ss, s.ds, x, y, o);
    } else {
        const float4 e = s.existing[i];
        const float ex[3] = {e.x, e.y, e.z};
        wcpt_bloom_upsample_texel(tex, s.ss, s.ds, x, y, ex, o);
    }
    s.dst[i] = make_float4(o[0], o[1], o[2], 1.0f); /* bloom.comp:147 */
}

template <bool RGBA8>
__global__ __launch_bounds__(256) void bloom_display_kernel(const float4* __restrict__ img, const float4* __restrict__ bloom,
                                                            const wcpt_bloom_size bs, const wcpt_bloom_size frame,
                                                            const uint32_t blocks_x, float4* __restrict__ out32,
                                                            uchar4* __restrict__ out8)
{
    const uint32_t bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
    const int x = (int)(bx * 32u + (threadIdx.x & 31u)), y = (int)(by * 8u + (threadIdx.x >> 5));
    if (x >= frame.w || y >= frame.h) return;
    const size_t i = (size_t)y * (size_t)frame.w + (size_t)x;
    const float4 v = img[i];
    const float in[4] = {v.x, v.y, v.z, v.w};
    float o[4];
    wcpt_bloom_display_texel(GlobalTexture{bloom, bs.w}, bs, frame, x, y, in, o);
    if (RGBA8)
        out8[i] = make_uchar4(wcpt_unorm8(o[0]), wcpt_unorm8(o[1]), wcpt_unorm8(o[2]), 255);
    else
        out32[i] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace dev

uint64_t bloom_pyramid_texels(uint32_t levels, const uint32_t* lw, const uint32_t* lh)
{
    uint64_t n = 0;
    for (uint32_t l = 0; l < levels; l++) n += (uint64_t)lw[l] * lh[l];
    return n;
}

namespace {

/* blocks of tw x th texels over a level; 0 when the count does not fit a launch */
uint32_t bloom_blocks(const wcpt_bloom_size& s, uint32_t tw, uint32_t th, uint32_t* blocks_x)
{
    const uint64_t nx = ((uint64_t)s.w + tw - 1u) / tw, ny = ((uint64_t)s.h + th - 1u) / th;
    *blocks_x = (uint32_t)nx;
    return nx * ny > 0x7FFFFFFFull ? 0u : (uint32_t)(nx * ny);
}

template <int MODE>
hipError_t launch_bloom_step(dev::BloomStep s, hipStream_t stream)
{
    const uint32_t blocks = bloom_blocks(s.ds, 16u, 16u, &s.blocks_x);
    if (!blocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::bloom_step_kernel<MODE>, dim3(blocks), dim3(256), 0, stream, s);
    return hipGetLastError();
}

} // namespace

hipError_t launch_composite_bloom(const float4* img, uint32_t width, uint32_t height, float threshold, float knee,
                                  uint32_t levels, const uint32_t* lw, const uint32_t* lh, float4* down, float4* up, void* dst,
                                  bool rgba8, hipStream_t stream)
{
    if (levels < 2 || levels > WCPT_BLOOM_MAX_LEVELS) return hipErrorInvalidValue;
    const wcpt_bloom_curve curve = wcpt_bloom_make_curve(threshold, knee);
    const wcpt_bloom_size frame = wcpt_bloom_make_size(width, height);
    wcpt_bloom_size size[WCPT_BLOOM_MAX_LEVELS];
    uint64_t at[WCPT_BLOOM_MAX_LEVELS]; /* a level's first texel in its pyramid (both laid out alike) */
    uint64_t n = 0;
    for (uint32_t l = 0; l < levels; l++) {
        size[l] = wcpt_bloom_make_size(lw[l], lh[l]);
        at[l] = n;
        n += (uint64_t)lw[l] * lh[l];
    }
    hipError_t e;
    for (uint32_t l = 0; l < levels; l++) {
        dev::BloomStep s{l ? down + at[l - 1] : img, nullptr, down + at[l], l ? size[l - 1] : frame, size[l], curve, 0u};
        e = l ? launch_bloom_step<dev::kBloomDownsample>(s, stream) : launch_bloom_step<dev::kBloomPrefilter>(s, stream);
        if (e != hipSuccess) return e;
    }
    for (uint32_t l = levels - 1; l-- > 0;) {
        const float4* below = (l + 2 == levels ? down : up) + at[l + 1];
        dev::BloomStep s{below, down + at[l], up + at[l], size[l + 1], size[l], curve, 0u};
        e = launch_bloom_step<dev::kBloomUpsample>(s, stream);
        if (e != hipSuccess) return e;
    }
    uint32_t blocks_x = 0;
    const uint32_t blocks = bloom_blocks(frame, 32u, 8u, &blocks_x);
    if (!blocks) return hipErrorInvalidValue;
    if (rgba8)
        hipLaunchKernelGGL(dev::bloom_display_kernel<true>, dim3(blocks), dim3(256), 0, stream, img, up + at[0], size[0], frame,
                           blocks_x, nullptr, static_cast<uchar4*>(dst));
    else
        hipLaunchKernelGGL(dev::bloom_display_kernel<false>, dim3(blocks), dim3(256), 0, stream, img, up + at[0], size[0], frame,
                           blocks_x, static_cast<float4*>(dst), nullptr);
    return hipGetLastError();
}

} // namespace wcpt
