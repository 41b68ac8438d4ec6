/*
 * wcpt_denoise.h — the guided a-trous denoise in front of the display step (wcpt_composite_denoise, wcpt_denoise_host):
 * the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010 over the accumulation image, guided by the primary-hit
 * records of wcpt_trace_primary (primary_hit.h). The reference has no denoiser, so the rule is fixed here.
 *
 * One definition of the arithmetic, shared by the HIP kernels (pt_denoise.hip) and the CPU path (wcpt_denoise_host in
 * host/wcpt_host.cpp), so both compute the identical binary32 sequence (compiled with -ffp-contract=off): every
 * operation below is rounded to binary32 in the order written, divisions are correctly rounded, exp is wcpt_expf.
 *
 * Guide of a pixel, derived once from its record (wcpt_denoise_pack):
 *   hit       kind is sphere or triangle (a kind of 3, which wcpt_trace_primary never writes, and a hit whose t is NaN,
 *             which no traversal accepts, are taken as a miss)
 *   identity  (kind, key): key = index for a sphere, draw for a triangle, 0 for a miss. All triangles of a draw are one
 *             surface; the reference has no textures, so a surface's albedo is constant per object and stopping at
 *             another identity does what albedo demodulation does elsewhere
 *   n         the record's normal
 *   P         t * direction, three products: the hit point relative to the camera (the camera position cancels in every
 *             difference)
 *   izt2      1 / ((sigma_depth * t) * (sigma_depth * t))
 *   a miss has P = 0, n = 0, izt2 = 0.
 * Packed into two 16-byte rows of 32-bit words, each row a plane of its own ([height][width] uint4):
 *   row 0   P.x P.y P.z key
 *   row 1   n.x n.y n.z kz      kz = the bits of izt2 (never negative, never NaN for a hit) with bit 31 set for a
 *                               triangle; WCPT_DENOISE_MISS_KZ (a NaN pattern) for a miss
 * so a tap costs one 16-byte colour load and two 16-byte guide loads, and the key is known after the first of them.
 * Guide words are only compared and multiplied, never used as an index.
 *
 * Iteration i = 0 .. iterations-1 with step s = 1 << i, for pixel p with colour c_p (wcpt_denoise_texel):
 *   the 25 taps (dx, dy), dy = -2..2 outer, dx = -2..2 inner; q = p + s * (dx, dy); a tap outside the frame is skipped
 *   k = h[|dx|] * h[|dy|], h = {3/8, 1/4, 1/16} (exact, and so are the products)
 *   a tap of another identity is skipped
 *   e = dc2 * isc2, dc2 = ((c_p - c_q).x^2 + .y^2) + .z^2, isc2 = 1 / (sigma_color * sigma_color) (0 for +inf)
 *   for a hit pixel: e += dn2 * isn2, then e += dz * dz * izt2; dn2 = |n_p - n_q|^2 associated as dc2,
 *   isn2 = 1 / (sigma_normal * sigma_normal), dz = (n_p.x * d.x + n_p.y * d.y) + n_p.z * d.z with d = P_q - P_p (the
 *   distance of q's point from p's tangent plane), izt2 the one of p
 *   w = k * wcpt_expf(-e); a tap with !(w > 0) is skipped (zero and NaN)
 *   acc += w * c_q per channel, ws += w
 *   out = acc / ws per channel where ws > 0, c_p otherwise (the centre tap was skipped: a NaN colour); alpha is c_p's.
 * Each iteration reads the one before; wcpt_composite_texel and wcpt_unorm8 are applied to the last one's result.
 * sigma_color is not halved per iteration: on one-sample input halving protects the noise.
 *
 * An image is anything with `void operator()(int x, int y, float rgba[4]) const`, a guide anything with
 * `void first(int x, int y, uint32_t row0[4]) const` and `void second(int x, int y, uint32_t row1[4]) const`, for
 * in-range pixels: arrays on the host, global memory on the device.
 */
#ifndef WCPT_DENOISE_H
#define WCPT_DENOISE_H

#include "wcpt_composite.h"

#define WCPT_DENOISE_MIN_ITERATIONS 1u
#define WCPT_DENOISE_MAX_ITERATIONS 6u
#define WCPT_DENOISE_RECORD_WORDS 12u /* primary_hit.h kPrimHitWords */
#define WCPT_DENOISE_RECORD_BYTES 48u
#define WCPT_DENOISE_GUIDE_BYTES 32u   /* the two packed rows of a pixel */
#define WCPT_DENOISE_SCRATCH_BYTES (2u * 16u + WCPT_DENOISE_GUIDE_BYTES) /* per pixel: two float4 images + the guide */

#define WCPT_DENOISE_MISS_KZ 0x7FC00000u      /* kz of a miss: a NaN pattern no hit's izt2 has */
#define WCPT_DENOISE_TRIANGLE_BIT 0x80000000u /* kz bit 31: the hit is a triangle */

/* The parameters as the taps use them, formed once on the host in binary32 */
typedef struct wcpt_denoise_consts {
    float isc2;        /* 1 / (sigma_color * sigma_color) */
    float isn2;        /* 1 / (sigma_normal * sigma_normal) */
    float sigma_depth;
} wcpt_denoise_consts;

static inline wcpt_denoise_consts wcpt_denoise_make_consts(float sigma_color, float sigma_normal, float sigma_depth)
{
    wcpt_denoise_consts k;
    k.isc2 = 1.0f / (sigma_color * sigma_color);
    k.isn2 = 1.0f / (sigma_normal * sigma_normal);
    k.sigma_depth = sigma_depth;
    return k;
}

/* iterations 1..6; sigma_color > 0 and not NaN (+inf turns the colour term off); sigma_normal and sigma_depth finite, > 0 */
static inline int wcpt_denoise_params_ok(uint32_t iterations, float sigma_color, float sigma_normal, float sigma_depth)
{
    const uint32_t n = wcpt_f2u(sigma_normal) & 0x7F800000u, d = wcpt_f2u(sigma_depth) & 0x7F800000u;
    return iterations >= WCPT_DENOISE_MIN_ITERATIONS && iterations <= WCPT_DENOISE_MAX_ITERATIONS && sigma_color > 0.0f &&
           n != 0x7F800000u && d != 0x7F800000u && sigma_normal > 0.0f && sigma_depth > 0.0f;
}

/* The two guide rows of a record's twelve words */
WCPT_HD void wcpt_denoise_pack(const uint32_t rec[WCPT_DENOISE_RECORD_WORDS], float sigma_depth, uint32_t row0[4],
                               uint32_t row1[4])
{
    const uint32_t kind = rec[7] & 3u; /* kPrimHitKindMask */
    const float t = wcpt_u2f(rec[3]);
    if ((kind != 1u && kind != 2u) || t != t) { /* kPrimHitSphere, kPrimHitTriangle */
        row0[0] = row0[1] = row0[2] = row0[3] = 0u;
        row1[0] = row1[1] = row1[2] = 0u;
        row1[3] = WCPT_DENOISE_MISS_KZ;
        return;
    }
    row0[0] = wcpt_f2u(t * wcpt_u2f(rec[0]));
    row0[1] = wcpt_f2u(t * wcpt_u2f(rec[1]));
    row0[2] = wcpt_f2u(t * wcpt_u2f(rec[2]));
    row0[3] = kind == 1u ? rec[9] : rec[10]; /* a sphere's index, a triangle's draw */
    row1[0] = rec[4];
    row1[1] = rec[5];
    row1[2] = rec[6];
    const float st = sigma_depth * t;
    const float izt2 = 1.0f / (st * st);
    row1[3] = (wcpt_f2u(izt2) & ~WCPT_DENOISE_TRIANGLE_BIT) | (kind == 2u ? WCPT_DENOISE_TRIANGLE_BIT : 0u);
}

/* kz's kind: 0 miss, 1 sphere, 2 triangle */
WCPT_HD uint32_t wcpt_denoise_kind(uint32_t kz)
{
    if ((kz & ~WCPT_DENOISE_TRIANGLE_BIT) > 0x7F800000u) return 0u;
    return (kz & WCPT_DENOISE_TRIANGLE_BIT) ? 2u : 1u;
}

WCPT_HD float wcpt_denoise_h(int d) /* the B3 spline's weight of offset d = -2..2 */
{
    return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

WCPT_HD float wcpt_denoise_dist2(const float a[3], const float b[3])
{
    const float x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return (x * x + y * y) + z * z;
}

/* One iteration of step `step` for pixel (x, y) of a w x h frame: `out` = the filtered RGB and the pixel's alpha */
template <class Img, class Guide>
WCPT_HD void wcpt_denoise_texel(const Img& img, const Guide& guide, int w, int h, int x, int y, int step,
                                const wcpt_denoise_consts& k, float out[4])
{
    float cp[4];
    uint32_t p0[4], p1[4];
    img(x, y, cp);
    guide.first(x, y, p0);
    guide.second(x, y, p1);
    const uint32_t kind_p = wcpt_denoise_kind(p1[3]);
    const bool hit = kind_p != 0u;
    const float izt2 = hit ? wcpt_u2f(p1[3] & ~WCPT_DENOISE_TRIANGLE_BIT) : 0.0f;
    const float Pp[3] = {wcpt_u2f(p0[0]), wcpt_u2f(p0[1]), wcpt_u2f(p0[2])};
    const float np[3] = {wcpt_u2f(p1[0]), wcpt_u2f(p1[1]), wcpt_u2f(p1[2])};
    float acc[3] = {0.0f, 0.0f, 0.0f}, ws = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= w) continue;
            const float kk = wcpt_denoise_h(dx) * wcpt_denoise_h(dy);
            uint32_t q0[4], q1[4];
            guide.first(qx, qy, q0);
            if (q0[3] != p0[3]) continue;
            guide.second(qx, qy, q1);
            if (wcpt_denoise_kind(q1[3]) != kind_p) continue;
            float cq[4];
            img(qx, qy, cq);
            float e = wcpt_denoise_dist2(cp, cq) * k.isc2;
            if (hit) {
                const float nq[3] = {wcpt_u2f(q1[0]), wcpt_u2f(q1[1]), wcpt_u2f(q1[2])};
                e = e + wcpt_denoise_dist2(np, nq) * k.isn2;
                const float d0 = wcpt_u2f(q0[0]) - Pp[0], d1 = wcpt_u2f(q0[1]) - Pp[1], d2 = wcpt_u2f(q0[2]) - Pp[2];
                const float dz = (np[0] * d0 + np[1] * d1) + np[2] * d2;
                e = e + dz * dz * izt2;
            }
            const float wt = kk * wcpt_expf(-e);
            if (!(wt > 0.0f)) continue;
            acc[0] = acc[0] + wt * cq[0];
            acc[1] = acc[1] + wt * cq[1];
            acc[2] = acc[2] + wt * cq[2];
            ws = ws + wt;
        }
    }
    if (ws > 0.0f) {
        out[0] = acc[0] / ws;
        out[1] = acc[1] / ws;
        out[2] = acc[2] / ws;
    } else {
        out[0] = cp[0];
        out[1] = cp[1];
        out[2] = cp[2];
    }
    out[3] = cp[3];
}

#endif
