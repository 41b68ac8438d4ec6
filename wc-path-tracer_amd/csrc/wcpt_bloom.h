/*
 * wcpt_bloom.h — the bloom pyramid of the display step: bloom.comp:25-148 and the Bloom branch of composite.comp:44-45.
 *
 * One definition of the arithmetic, shared by the HIP kernels (pt_bloom.hip) and the CPU path (wcpt_bloom_host in
 * host/wcpt_host.cpp), so both compute the identical binary32 sequence (compiled with -ffp-contract=off): every
 * operation below is rounded to binary32 in the order written, and divisions are correctly rounded.
 *
 * bloom.comp leaves several things to the Vulkan implementation; this header fixes them:
 *   min / max / clamp   as GLSL defines them (min(x, y) = y < x ? y : x, max(x, y) = x < y ? y : x, clamp = min(max(x,
 *                       lo), hi)), so a NaN operand has one defined result; never fminf / fmaxf (bloom.comp:72-76, :83).
 *   the sampler         linear filter, clamp to edge, RGB only (every level's alpha is written as 1, bloom.comp:147). For a
 *                       level of (w, h) texels and a coordinate uv: px = uv.x * w - 0.5f, x0 = floor(px), fx = px - x0, the
 *                       same in y; the texel indices x0, x0 + 1, y0, y0 + 1 are each clamped to [0, size - 1]; per channel
 *                       (t00 * (1 - fx) + t10 * fx) * (1 - fy) + (t01 * (1 - fx) + t11 * fx) * fy. Vulkan leaves the
 *                       precision of the filter weights to the implementation: this binary32 lerp is the definition
 *                       (every textureLod of bloom.comp:28-46, :93-104 and the texture() of composite.comp:46).
 *   texel coordinates   of output texel (x, y) of a level of (ow, oh) texels, in the shader's order (bloom.comp:111-115,
 *                       composite.comp:37-41): float(x) / ow + (1.f / ow) * 0.5f.
 *   existing            textureLod(u_Texture, texCoords, LOD) of bloom.comp:130, :139 samples a level of the destination's
 *                       size at a texel centre: it is the destination texel itself, as in wcpt_composite_texel.
 *
 * The reference has no host code for the four Modes, so the chain is fixed here, in the order the
 * modes' parameters imply. For a W x H frame, level l has w_l = max(1, W >> (l + 1)), h_l = max(1, H >> (l + 1)) texels
 * (a half-resolution base and its mips); L = the requested count clipped to 1 + floor(log2(min(w_0, h_0))), at least 2.
 *   D[0]   = Prefilter(Box13(image, uv, 1 / size(image)))             MODE_PREFILTER
 *   D[l]   = Box13(D[l-1], uv, 1 / size(D[l-1])), l = 1 .. L-1        MODE_DOWNSAMPLE
 *   U[L-2] = D[L-2] + Tent9(D[L-1], uv, 1 / size(D[L-1]), 1)          MODE_UPSAMPLE_FIRST
 *   U[l]   = D[l] + Tent9(U[l+1], uv, 1 / size(U[l+1]), 1), l = L-3 .. 0   MODE_UPSAMPLE
 *   display: rgb = image(x, y).rgb + sample(U[0], uv of the full-size pixel), then wcpt_composite_texel.
 *
 * A texture is anything with `void operator()(int x, int y, float rgb[3]) const` for in-range texel indices: a float4
 * array on the host, global memory or a staged tile on the device.
 */
#ifndef WCPT_BLOOM_H
#define WCPT_BLOOM_H

#include "wcpt_composite.h"

#define WCPT_BLOOM_MAX_LEVELS 16 /* the arrays of wcpt_bloom_levels */
#define WCPT_BLOOM_MIN_REQUEST 2
#define WCPT_BLOOM_MAX_REQUEST 12

WCPT_HD float wcpt_bloom_min(float x, float y) { return y < x ? y : x; }
WCPT_HD float wcpt_bloom_max(float x, float y) { return x < y ? y : x; }
WCPT_HD float wcpt_bloom_clamp(float x, float lo, float hi) { return wcpt_bloom_min(wcpt_bloom_max(x, lo), hi); }

/* A level's size as the shaders use it: vec2(textureSize) / vec2(imageSize), 1.f / that, and half of that. Formed once
 * per step on the host in binary32. */
typedef struct wcpt_bloom_size {
    int w, h;
    float fw, fh;     /* float(w), float(h) */
    float tx, ty;     /* 1.f / fw, 1.f / fh */
    float hx, hy;     /* tx * 0.5f, ty * 0.5f: the texel-centre offset of bloom.comp:115, composite.comp:41 */
} wcpt_bloom_size;

static inline wcpt_bloom_size wcpt_bloom_make_size(uint32_t w, uint32_t h)
{
    wcpt_bloom_size s;
    s.w = (int)w;
    s.h = (int)h;
    s.fw = (float)w;
    s.fh = (float)h;
    s.tx = 1.0f / s.fw;
    s.ty = 1.0f / s.fh;
    s.hx = s.tx * 0.5f;
    s.hy = s.ty * 0.5f;
    return s;
}

/* Params of bloom.comp:20: (threshold, threshold - knee, knee * 2, 0.25 / knee), formed once on the host */
typedef struct wcpt_bloom_curve {
    float x, y, z, w;
} wcpt_bloom_curve;

static inline wcpt_bloom_curve wcpt_bloom_make_curve(float threshold, float knee)
{
    wcpt_bloom_curve c;
    c.x = threshold;
    c.y = threshold - knee;
    c.z = knee * 2.0f;
    c.w = 0.25f / knee;
    return c;
}

/* The chain's levels for a width x height frame: the clipped count and each level's size. Returns 0 when the frame or
 * the request admits no chain (requested outside 2..12, or fewer than 2 levels after clipping). */
static inline uint32_t wcpt_bloom_plan(uint32_t width, uint32_t height, uint32_t requested, uint32_t* w, uint32_t* h)
{
    if (requested < WCPT_BLOOM_MIN_REQUEST || requested > WCPT_BLOOM_MAX_REQUEST) return 0;
    const uint32_t w0 = width >> 1, h0 = height >> 1;
    uint32_t m = w0 < h0 ? w0 : h0, cap = 0;
    for (; m; m >>= 1) cap++; /* 1 + floor(log2(min(w_0, h_0))); 0 for a frame below 2 x 2 */
    const uint32_t levels = requested < cap ? requested : cap;
    if (levels < 2) return 0;
    for (uint32_t l = 0; l < levels; l++) {
        const uint32_t wl = width >> (l + 1), hl = height >> (l + 1);
        w[l] = wl ? wl : 1u;
        h[l] = hl ? hl : 1u;
    }
    return levels;
}

/* threshold and knee finite, knee > 0 (0.25 / knee and the division by max(brightness, Epsilon) stay defined) */
static inline int wcpt_bloom_curve_ok(float threshold, float knee)
{
    const uint32_t t = wcpt_f2u(threshold) & 0x7F800000u, k = wcpt_f2u(knee) & 0x7F800000u;
    return t != 0x7F800000u && k != 0x7F800000u && knee > 0.0f;
}

/* bloom.comp:114-115 / composite.comp:39-41: the coordinate of output texel i along an axis of `f` texels */
WCPT_HD float wcpt_bloom_coord(int i, float f, float half_texel) { return (float)i / f + half_texel; }

/* One axis of the sampler: the two clamped texel indices and the weight of the second */
WCPT_HD void wcpt_bloom_axis(float c, float f, int n, int* i0, int* i1, float* frac)
{
    const float p = c * f - 0.5f;
    const float fl = floorf(p);
    *frac = p - fl;
    const int a = (int)fl, b = a + 1;
    *i0 = a < 0 ? 0 : (a > n - 1 ? n - 1 : a);
    *i1 = b < 0 ? 0 : (b > n - 1 ? n - 1 : b);
}

/* textureLod(tex, (u, v), lod).rgb */
template <class Tex>
WCPT_HD void wcpt_bloom_sample(const Tex& tex, const wcpt_bloom_size& s, float u, float v, float out[3])
{
    int x0, x1, y0, y1;
    float fx, fy;
    wcpt_bloom_axis(u, s.fw, s.w, &x0, &x1, &fx);
    wcpt_bloom_axis(v, s.fh, s.h, &y0, &y1, &fy);
    float t00[3], t10[3], t01[3], t11[3];
    tex(x0, y0, t00);
    tex(x1, y0, t10);
    tex(x0, y1, t01);
    tex(x1, y1, t11);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    for (int c = 0; c < 3; c++) out[c] = (t00[c] * gx + t10[c] * fx) * gy + (t01[c] * gx + t11[c] * fx) * fy;
}

/* bloom.comp:25-65 DownsampleBox13. I and J read the same texel and L reads F's (:39-46): the taps at (2, -2) and (-2, 2)
 * are never read, which makes the filter asymmetric; the sums keep the shader's order. */
template <class Tex>
WCPT_HD void wcpt_bloom_box13(const Tex& tex, const wcpt_bloom_size& s, float u, float v, float out[3])
{
    const float tx = s.tx * 0.5f, ty = s.ty * 0.5f; /* :30 texelSize *= 0.5f */
    float A[3], B[3], C[3], D[3], E[3], F[3], G[3], H[3], I[3], K[3], M[3];
    wcpt_bloom_sample(tex, s, u, v, A);
    wcpt_bloom_sample(tex, s, u + tx * -1.0f, v + ty * -1.0f, B);
    wcpt_bloom_sample(tex, s, u + tx * -1.0f, v + ty * 1.0f, C);
    wcpt_bloom_sample(tex, s, u + tx * 1.0f, v + ty * 1.0f, D);
    wcpt_bloom_sample(tex, s, u + tx * 1.0f, v + ty * -1.0f, E);
    wcpt_bloom_sample(tex, s, u + tx * -2.0f, v + ty * -2.0f, F); /* = L */
    wcpt_bloom_sample(tex, s, u + tx * -2.0f, v + ty * 0.0f, G);
    wcpt_bloom_sample(tex, s, u + tx * 0.0f, v + ty * 2.0f, H);
    wcpt_bloom_sample(tex, s, u + tx * 2.0f, v + ty * 2.0f, I); /* = J */
    wcpt_bloom_sample(tex, s, u + tx * 2.0f, v + ty * 0.0f, K);
    wcpt_bloom_sample(tex, s, u + tx * 0.0f, v + ty * -2.0f, M);
    for (int c = 0; c < 3; c++) {
        const float J = I[c], L = F[c];
        float r = 0.0f;
        r += (B[c] + C[c] + D[c] + E[c]) * 0.5f;
        r += (F[c] + G[c] + A[c] + M[c]) * 0.125f;
        r += (G[c] + H[c] + I[c] + A[c]) * 0.125f;
        r += (A[c] + I[c] + J + K[c]) * 0.125f;
        r += (M[c] + A[c] + K[c] + L) * 0.125f;
        r *= 0.25f;
        out[c] = r;
    }
}

/* bloom.comp:80-86 Prefilter with :69-78 QuadraticThreshold, in place */
WCPT_HD void wcpt_bloom_prefilter(float c[3], const wcpt_bloom_curve& p)
{
    const float epsilon = 1.0e-4f; /* :6 */
    c[0] = wcpt_bloom_min(20.0f, c[0]);
    c[1] = wcpt_bloom_min(20.0f, c[1]);
    c[2] = wcpt_bloom_min(20.0f, c[2]);
    const float brightness = wcpt_bloom_max(wcpt_bloom_max(c[0], c[1]), c[2]);
    float rq = wcpt_bloom_clamp(brightness - p.y, 0.0f, p.z);
    rq = (rq * rq) * p.w;
    const float scale = wcpt_bloom_max(rq, brightness - p.x) / wcpt_bloom_max(brightness, epsilon);
    c[0] *= scale;
    c[1] *= scale;
    c[2] *= scale;
}

/* bloom.comp:88-107 UpsampleTent9 with radius 1: offset = texelSize.xyxy * (1, 1, -1, 0) * radius */
template <class Tex>
WCPT_HD void wcpt_bloom_tent9(const Tex& tex, const wcpt_bloom_size& s, float u, float v, float out[3])
{
    const float radius = 1.0f;
    const float ox = s.tx * 1.0f * radius, oy = s.ty * 1.0f * radius, oz = s.tx * -1.0f * radius, ow = s.ty * 0.0f * radius;
    float t[3], r[3];
    wcpt_bloom_sample(tex, s, u, v, t);
    for (int c = 0; c < 3; c++) r[c] = t[c] * 4.0f;
    wcpt_bloom_sample(tex, s, u - ox, v - oy, t);
    for (int c = 0; c < 3; c++) r[c] += t[c];
    wcpt_bloom_sample(tex, s, u - ow, v - oy, t);
    for (int c = 0; c < 3; c++) r[c] += t[c] * 2.0f;
    wcpt_bloom_sample(tex, s, u - oz, v - oy, t);
    for (int c = 0; c < 3; c++) r[c] += t[c];
    wcpt_bloom_sample(tex, s, u + oz, v + ow, t);
    for (int c = 0; c < 3; c++) r[c] += t[c] * 2.0f;
    wcpt_bloom_sample(tex, s, u + ox, v + ow, t);
    for (int c = 0; c < 3; c++) r[c] += t[c] * 2.0f;
    wcpt_bloom_sample(tex, s, u + oz, v + oy, t);
    for (int c = 0; c < 3; c++) r[c] += t[c];
    wcpt_bloom_sample(tex, s, u + ow, v + oy, t);
    for (int c = 0; c < 3; c++) r[c] += t[c] * 2.0f;
    wcpt_bloom_sample(tex, s, u + ox, v + oy, t);
    for (int c = 0; c < 3; c++) r[c] += t[c];
    for (int c = 0; c < 3; c++) out[c] = r[c] * (1.0f / 16.0f);
}

/* The four modes for output texel (x, y) of a level of size `dst`, reading a texture of size `src` */
template <class Tex>
WCPT_HD void wcpt_bloom_prefilter_texel(const Tex& image, const wcpt_bloom_size& src, const wcpt_bloom_size& dst, int x, int y,
                                        const wcpt_bloom_curve& p, float out[3])
{
    wcpt_bloom_box13(image, src, wcpt_bloom_coord(x, dst.fw, dst.hx), wcpt_bloom_coord(y, dst.fh, dst.hy), out);
    wcpt_bloom_prefilter(out, p);
}

template <class Tex>
WCPT_HD void wcpt_bloom_downsample_texel(const Tex& up, const wcpt_bloom_size& src, const wcpt_bloom_size& dst, int x, int y,
                                         float out[3])
{
    wcpt_bloom_box13(up, src, wcpt_bloom_coord(x, dst.fw, dst.hx), wcpt_bloom_coord(y, dst.fh, dst.hy), out);
}

/* MODE_UPSAMPLE_FIRST and MODE_UPSAMPLE differ only in which pyramid `below` comes from; `existing` = D[l](x, y) */
template <class Tex>
WCPT_HD void wcpt_bloom_upsample_texel(const Tex& below, const wcpt_bloom_size& src, const wcpt_bloom_size& dst, int x, int y,
                                       const float existing[3], float out[3])
{
    float t[3];
    wcpt_bloom_tent9(below, src, wcpt_bloom_coord(x, dst.fw, dst.hx), wcpt_bloom_coord(y, dst.fh, dst.hy), t);
    for (int c = 0; c < 3; c++) out[c] = existing[c] + t[c];
}

/* composite.comp:36-53 with Bloom set, for pixel (x, y) of a frame of size `frame`: `in` = image(x, y) */
template <class Tex>
WCPT_HD void wcpt_bloom_display_texel(const Tex& bloom, const wcpt_bloom_size& src, const wcpt_bloom_size& frame, int x, int y,
                                      const float in[4], float out[4])
{
    float t[3];
    wcpt_bloom_sample(bloom, src, wcpt_bloom_coord(x, frame.fw, frame.hx), wcpt_bloom_coord(y, frame.fh, frame.hy), t);
    const float sum[4] = {in[0] + t[0], in[1] + t[1], in[2] + t[2], in[3]};
    wcpt_composite_texel(sum, out);
}

#endif
