/*
 * pt_temporal.hip — temporal reprojection in front of the display step (the rule, the history's packing and every
 * operation's order in wcpt_temporal.h): a reproject-and-blend kernel for a call that restarts the sequence and a streaming
 * blend kernel for the others, both with the display step fused in (gamma, PBR Neutral, rgba32f or RGBA8) unless the
 * denoise follows, which then takes the new hist image as its source.
 *
 * One launch per call, on the caller's stream. The scratch holds two sides of {hist float4 image, packed guide row 0, row 1,
 * lengths} and one float4 plane of {base.rgb, n_b}: a restart reads the old side at four gathered taps per pixel while it
 * writes the other, so the sides ping-pong; the streaming kernel reads and writes only its own pixel and works in place.
 *
 * Reproject: one pixel per lane, 32x8 pixels per 256-thread block as in the denoise and bloom display kernels, so a wave's
 * reads of a tap are row pieces of up to 512 bytes in each plane wherever neighbouring pixels reproject to neighbouring
 * texels, which is the case on one surface. Per pixel it streams the 48-byte record and the accumulation texel in (64 bytes)
 * and base, the packed guide, hist and its length out (68 bytes) plus the display texel (4 or 16); the four taps read 4 x 52
 * bytes, of which, with a bilinear footprint shared by the neighbours, about 52 are compulsory: 188 to 200 bytes per pixel.
 * A lane tests a tap's weight and length first, then the first guide row's key, the second row's kind, normal and depth, and
 * only then loads the colour: a tap that does not count contributes nothing, so the order of the loads does not change the
 * bits. All loads and stores are 16 bytes wide but the length plane's and RGBA8's 4, and all stores are plain vector stores.
 *
 * Blend: a one-dimensional grid, one pixel per lane: 32 bytes in, 20 out and the display texel.
 */
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "wcpt_temporal.h"

namespace wcpt {
namespace dev {

/* one side of the scratch as the taps read it */
struct TemporalHistory {
    const uint4* __restrict__ row0;
    const uint4* __restrict__ row1;
    const float* __restrict__ len;
    const float4* __restrict__ texels;
    int w;
    __device__ size_t at(int x, int y) const { return (size_t)y * (size_t)w + (size_t)x; }
    __device__ static void get(const uint4* plane, size_t i, uint32_t r[4])
    {
        const uint4 v = plane[i];
        r[0] = v.x;
        r[1] = v.y;
        r[2] = v.z;
        r[3] = v.w;
    }
    __device__ void first(int x, int y, uint32_t r[4]) const { get(row0, at(x, y), r); }
    __device__ void second(int x, int y, uint32_t r[4]) const { get(row1, at(x, y), r); }
    __device__ float length(int x, int y) const { return len[at(x, y)]; }
    __device__ void colour(int x, int y, float rgba[4]) const
    {
        const float4 t = texels[at(x, y)];
        rgba[0] = t.x;
        rgba[1] = t.y;
        rgba[2] = t.z;
        rgba[3] = t.w;
    }
};

/* what a kernel writes of a side */
struct TemporalSide {
    uint4* row0;
    uint4* row1;
    float* len;
    float4* texels;
};

enum TemporalStore { kTemporalNone, kTemporalRgba32f, kTemporalRgba8 };

template <int STORE>
__device__ __forceinline__ void temporal_display(const float f[4], size_t i, float4* __restrict__ out32,
                                                 uchar4* __restrict__ out8)
{
    if (STORE == kTemporalNone) return;
    float o[4];
    wcpt_composite_texel(f, o);
    if (STORE == kTemporalRgba8)
        out8[i] = make_uchar4(wcpt_unorm8(o[0]), wcpt_unorm8(o[1]), wcpt_unorm8(o[2]), 255);
    else
        out32[i] = make_float4(o[0], o[1], o[2], o[3]);
}

/* A restart call. `has_hist` (the same in every lane): `old` and `cam` are the previous sequence's; without it base = 0,
 * n_b = 0 and `old` is not read. */
template <int STORE>
__global__ __launch_bounds__(256) void temporal_reproject_kernel(
    const uint4* __restrict__ records, const float4* __restrict__ cur, const int w, const int h, const uint32_t blocks_x,
    const float ox, const float oy, const float oz, const int has_hist, const wcpt_temporal_camera cam,
    const TemporalHistory old, const float f, const wcpt_temporal_consts k, float4* __restrict__ base_nb,
    const TemporalSide side, float4* __restrict__ out32, uchar4* __restrict__ out8)
{
    const uint32_t bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
    const int x = (int)(bx * 32u + (threadIdx.x & 31u)), y = (int)(by * 8u + (threadIdx.x >> 5));
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    const uint4 a = records[3 * i], b = records[3 * i + 1], c = records[3 * i + 2];
    const uint32_t rec[WCPT_TEMPORAL_RECORD_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    const float4 ct = cur[i];
    const float cp[4] = {ct.x, ct.y, ct.z, ct.w};
    const float o[3] = {ox, oy, oz};
    uint32_t p0[4], p1[4];
    wcpt_temporal_pack(rec, o, p0, p1);
    float base[3] = {0.0f, 0.0f, 0.0f}, n_b = 0.0f;
    if (has_hist) wcpt_temporal_reproject(rec, p0, p1, cam, old, w, h, k, base, &n_b);
    float out[4], len;
    wcpt_temporal_blend(cp, base, n_b, f, k, out, &len);
    base_nb[i] = make_float4(base[0], base[1], base[2], n_b);
    side.row0[i] = make_uint4(p0[0], p0[1], p0[2], p0[3]);
    side.row1[i] = make_uint4(p1[0], p1[1], p1[2], p1[3]);
    side.len[i] = len;
    side.texels[i] = make_float4(out[0], out[1], out[2], out[3]);
    temporal_display<STORE>(out, i, out32, out8);
}

/* Every other call: the stored base blended with the grown accumulation image, in place in the sequence's side */
template <int STORE>
__global__ __launch_bounds__(256) void temporal_blend_kernel(const float4* __restrict__ cur, const uint64_t pixels,
                                                             const float4* __restrict__ base_nb, const float f,
                                                             const wcpt_temporal_consts k, float* __restrict__ lengths,
                                                             float4* __restrict__ texels, float4* __restrict__ out32,
                                                             uchar4* __restrict__ out8)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float4 ct = cur[i], bt = base_nb[i];
    const float cp[4] = {ct.x, ct.y, ct.z, ct.w};
    const float base[3] = {bt.x, bt.y, bt.z};
    float out[4], len;
    wcpt_temporal_blend(cp, base, bt.w, f, k, out, &len);
    lengths[i] = len;
    texels[i] = make_float4(out[0], out[1], out[2], out[3]);
    temporal_display<STORE>(out, (size_t)i, out32, out8);
}

/* the scratch: the two sides' hist images, base with n_b, the sides' guide rows, the sides' lengths */
struct TemporalLayout {
    float4* texels[2];
    float4* base_nb;
    uint4* row0[2];
    uint4* row1[2];
    float* len[2];
};

static TemporalLayout temporal_layout(void* scratch, uint64_t pixels)
{
    TemporalLayout l;
    l.texels[0] = static_cast<float4*>(scratch);
    l.texels[1] = l.texels[0] + pixels;
    l.base_nb = l.texels[1] + pixels;
    l.row0[0] = reinterpret_cast<uint4*>(l.base_nb + pixels);
    l.row1[0] = l.row0[0] + pixels;
    l.row0[1] = l.row1[0] + pixels;
    l.row1[1] = l.row0[1] + pixels;
    l.len[0] = reinterpret_cast<float*>(l.row1[1] + pixels);
    l.len[1] = l.len[0] + pixels;
    return l;
}

} // namespace dev

uint64_t temporal_scratch_bytes(uint32_t width, uint32_t height)
{
    return (uint64_t)width * height * WCPT_TEMPORAL_SCRATCH_BYTES;
}

const float4* temporal_hist_image(void* scratch, uint32_t width, uint32_t height, uint32_t side)
{
    return dev::temporal_layout(scratch, (uint64_t)width * height).texels[side & 1u];
}

hipError_t launch_temporal_reproject(const float4* img, const void* records, uint32_t width, uint32_t height,
                                     const float position[3], bool has_hist, const wcpt_temporal_camera& hist_cam,
                                     uint32_t old_side, float frames, const wcpt_temporal_consts& k, void* scratch, void* dst,
                                     int store, hipStream_t stream)
{
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const uint64_t pixels = (uint64_t)width * height;
    const uint64_t nx = ((uint64_t)width + 31u) / 32u, ny = ((uint64_t)height + 7u) / 8u;
    if (pixels == 0 || nx * ny > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dev::TemporalLayout l = dev::temporal_layout(scratch, pixels);
    const uint32_t o = old_side & 1u, n = o ^ 1u;
    const dev::TemporalHistory old{l.row0[o], l.row1[o], l.len[o], l.texels[o], (int)width};
    const dev::TemporalSide side{l.row0[n], l.row1[n], l.len[n], l.texels[n]};
    const dim3 grid((uint32_t)(nx * ny)), block(256);
    const uint4* rec = static_cast<const uint4*>(records);
    const int w = (int)width, h = (int)height, hh = has_hist ? 1 : 0;
    if (store == dev::kTemporalRgba8)
        hipLaunchKernelGGL(dev::temporal_reproject_kernel<dev::kTemporalRgba8>, grid, block, 0, stream, rec, img, w, h,
                           (uint32_t)nx, position[0], position[1], position[2], hh, hist_cam, old, frames, k, l.base_nb, side,
                           nullptr, static_cast<uchar4*>(dst));
    else if (store == dev::kTemporalRgba32f)
        hipLaunchKernelGGL(dev::temporal_reproject_kernel<dev::kTemporalRgba32f>, grid, block, 0, stream, rec, img, w, h,
                           (uint32_t)nx, position[0], position[1], position[2], hh, hist_cam, old, frames, k, l.base_nb, side,
                           static_cast<float4*>(dst), nullptr);
    else
        hipLaunchKernelGGL(dev::temporal_reproject_kernel<dev::kTemporalNone>, grid, block, 0, stream, rec, img, w, h,
                           (uint32_t)nx, position[0], position[1], position[2], hh, hist_cam, old, frames, k, l.base_nb, side,
                           nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_temporal_blend(const float4* img, uint32_t width, uint32_t height, uint32_t side, float frames,
                                 const wcpt_temporal_consts& k, void* scratch, void* dst, int store, hipStream_t stream)
{
    const uint64_t pixels = (uint64_t)width * height;
    const uint64_t blocks = (pixels + 255u) / 256u;
    if (pixels == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dev::TemporalLayout l = dev::temporal_layout(scratch, pixels);
    const uint32_t s = side & 1u;
    const dim3 grid((uint32_t)blocks), block(256);
    if (store == dev::kTemporalRgba8)
        hipLaunchKernelGGL(dev::temporal_blend_kernel<dev::kTemporalRgba8>, grid, block, 0, stream, img, pixels, l.base_nb,
                           frames, k, l.len[s], l.texels[s], nullptr, static_cast<uchar4*>(dst));
    else if (store == dev::kTemporalRgba32f)
        hipLaunchKernelGGL(dev::temporal_blend_kernel<dev::kTemporalRgba32f>, grid, block, 0, stream, img, pixels, l.base_nb,
                           frames, k, l.len[s], l.texels[s], static_cast<float4*>(dst), nullptr);
    else
        hipLaunchKernelGGL(dev::temporal_blend_kernel<dev::kTemporalNone>, grid, block, 0, stream, img, pixels, l.base_nb,
                           frames, k, l.len[s], l.texels[s], nullptr, nullptr);
    return hipGetLastError();
}

} // namespace wcpt
