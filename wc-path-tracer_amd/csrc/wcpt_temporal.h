/*
 * wcpt_temporal.h — temporal reprojection in front of the display step (wcpt_composite_temporal, wcpt_temporal_host): the
 * temporal half of an SVGF-style pipeline (Schied et al. 2017). While something moves the reference's editor restarts the
 * accumulation every frame (editor.jai:149-152, 214), so each displayed frame is one fresh sample; the surfaces on screen are
 * mostly those of a frame ago, and with the primary-hit records (primary_hit.h) and the cameras of both frames the previous
 * result is looked up where each pixel's surface point was. The reference has no such stage, so the rule is fixed here.
 *
 * One definition of the arithmetic, shared by the HIP kernels (pt_temporal.hip) and the CPU path (wcpt_temporal_host in
 * host/wcpt_host.cpp), so both compute the identical binary32 sequence (compiled with -ffp-contract=off): every operation
 * of the per-pixel part is rounded to binary32 in the order written, divisions are correctly rounded. The camera part runs
 * on the host only, in binary64, in the order written.
 *
 * Camera of a frame (wcpt_temporal_make_camera), from the fields wcpt_trace_primary reads, so the reprojection inverts what
 * the rays really did whatever matrix convention the host has. Matrices are column-major; M[r][c] below is row r, column c.
 *   inverse(M)  Gauss-Jordan on [M | I] in binary64, column by column: the pivot is the row at or below the diagonal with
 *               the largest |entry| of the column (the first of equals), a pivot below 1e-300 in magnitude is singular;
 *               the pivot row is swapped into place and every entry of it divided by the pivot; then from each other row,
 *               in order, whose entry f in the column is not zero, f * (pivot row) is subtracted entry by entry
 *   A     the upper-left 3x3 of inverseView (the shader multiplies a direction with w = 0)
 *   P     inverse(inverseProjection), 4x4
 *   R     rows 0, 1 and 3 of P restricted to columns 0..2
 *   F     R * inverse(A): F[i][j] = (R[i][0] * Ai[0][j] + R[i][1] * Ai[1][j]) + R[i][2] * Ai[2][j], each entry then rounded
 *         once to binary32. F maps a world-space offset r from the camera to (cx, cy, cw): clip x, y and w.
 *   check the rounded F, in binary64: for the four corner pixels (x, y) in {0, width-1} x {0, height-1} the primary
 *         direction is formed as pathTracer.comp:290-302 forms it (c = x / width + (1 / width) * 0.5, the same for y,
 *         cy = 1 - cy, c * 2 - 1; target = inverseProjection * (cx, cy, 1, 1); d = normalize(target.xyz / target.w);
 *         direction = normalize(A * d)) and pushed through F and the pixel position below; cw must be > 0 and the position
 *         within 1e-3 pixel of (x, y) in both coordinates. A singular matrix or a missed corner refuses the camera: that
 *         covers a projection that is not a plain perspective, and every non-finite entry.
 *
 * State of a sequence (the calls between two restarts of the accumulation):
 *   base, n_b  float RGB and float per pixel: the history carried into the sequence and how many samples it counts (0: none)
 *   hist       the last output as a float4 image (alpha = the accumulation image's alpha, so the image can go through the
 *              denoise launch unchanged) with a plane of lengths beside it
 *   the guide and the camera position hist belongs to
 *
 * Guide of a pixel, derived once from its record (wcpt_temporal_pack) for the camera position `o` of its frame:
 *   hit, identity (kind, key)   exactly as wcpt_denoise_pack takes them: a kind other than sphere or triangle and a hit whose
 *              t is NaN are a miss; key = index for a sphere, draw for a triangle; a miss is (0, 0)
 *   W          o + t * direction per component, one product and one sum: the hit's world point; zeros for a miss
 *   n          the record's normal; zeros for a miss
 * Packed into two 16-byte rows of 32-bit words, each row a plane of its own ([height][width] uint4):
 *   row 0   W.x W.y W.z key
 *   row 1   n.x n.y n.z kind    kind 0 miss, 1 sphere, 2 triangle
 * Guide words are only compared and multiplied, never used as an index.
 *
 * Restart call (wcpt_temporal_reproject), for pixel p with record g of the new guide, the new frame's camera position o, and
 * the history frame's camera (F, o_h), frame w x h:
 *   1  hit, identity, W, n of p as above, t = g.t
 *   2  r = W - o_h per component for a hit, r = g.direction for a miss (the sky is at infinity)
 *   3  cx = (F[0][0] * r.x + F[0][1] * r.y) + F[0][2] * r.z, cy and cw the same with rows 1 and 2; !(cw > 0): no history
 *   4  nx = cx / cw, ny = cy / cw
 *      fx = (nx * 0.5f + 0.5f) * (float)w - 0.5f
 *      fy = (1.0f - (ny * 0.5f + 0.5f)) * (float)h - 0.5f
 *      unless fx >= -1.0f and fx < (float)w and fy >= -1.0f and fy < (float)h there is no history (NaN and the infinities
 *      fail these comparisons); only after this check is anything converted to an integer
 *      x0 = floor(fx), ax = fx - x0; y0 = floor(fy), ay = fy - y0
 *   5  the taps (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1) in this order, with the weights bx * by, ax * by, bx * ay,
 *      ax * ay where bx = 1.0f - ax, by = 1.0f - ay. A tap q counts only if it is inside the frame, its length is > 0, it
 *      has p's identity, its three colour channels are finite, its weight is > 0, and for a hit
 *        (n.x * n_q.x + n.y * n_q.y) + n.z * n_q.z >= normal_min
 *        |(n.x * d.x + n.y * d.y) + n.z * d.z| <= depth_tol * t with d = W_q - W per component
 *      (a NaN fails both). A counting tap adds acc += weight * c_q per channel, nacc += weight * len_q, ws += weight.
 *   6  ws > 0: base = acc / ws per channel, n_b = nacc / ws; otherwise base = +0.0 and n_b = 0.
 *
 * Blend, on every call (wcpt_temporal_blend): f = (float)frames, the samples in the accumulation image `cur`:
 *   n_b == 0: out.rgb = cur.rgb bit for bit
 *   otherwise tot = n_b + f, a = f / tot, out = base + (cur - base) * a per channel
 *   the stored length is min(n_b + f, (float)max_history) (n_b + 0 == n_b exactly, so the sum is formed either way)
 *   out.a = cur.a
 * A call that is not a restart re-blends the stored base with the grown accumulation image, so a still camera converges as
 * without this stage and nothing is counted twice.
 *
 * History accessors: anything with `void first(int x, int y, uint32_t row0[4]) const`, `void second(...) const`,
 * `float length(int x, int y) const` and `void colour(int x, int y, float rgba[4]) const` for in-range pixels: arrays on
 * the host, global memory on the device. A tap position comes only from the range-checked fx, fy.
 */
#ifndef WCPT_TEMPORAL_H
#define WCPT_TEMPORAL_H

#include "wcpt_composite.h"

#define WCPT_TEMPORAL_MAX_HISTORY 65536u
#define WCPT_TEMPORAL_RECORD_WORDS 12u /* primary_hit.h kPrimHitWords */
#define WCPT_TEMPORAL_RECORD_BYTES 48u
/* Scratch per pixel: hist (a float4 image, a length, the two guide rows) twice, because a restart's neighbours read the
 * old one while the new one is written, and base with n_b as one float4 */
#define WCPT_TEMPORAL_SIDE_BYTES (16u + 4u + 32u)
#define WCPT_TEMPORAL_SCRATCH_BYTES (2u * WCPT_TEMPORAL_SIDE_BYTES + 16u) /* 120 */

/* A frame's camera as the taps use it */
typedef struct wcpt_temporal_camera {
    float F[9];        /* row-major 3x3: a world-space offset from the camera -> (cx, cy, cw) */
    float position[3];
} wcpt_temporal_camera;

/* The parameters as the taps use them */
typedef struct wcpt_temporal_consts {
    float max_history; /* (float)max_history, exact up to 65536 */
    float normal_min;
    float depth_tol;
} wcpt_temporal_consts;

/* max_history 1..65536; normal_min finite in [-1, 1]; depth_tol finite, > 0 */
static inline int wcpt_temporal_params_ok(uint32_t max_history, float normal_min, float depth_tol)
{
    const uint32_t d = wcpt_f2u(depth_tol) & 0x7F800000u;
    return max_history >= 1u && max_history <= WCPT_TEMPORAL_MAX_HISTORY && normal_min >= -1.0f && normal_min <= 1.0f &&
           d != 0x7F800000u && depth_tol > 0.0f;
}

static inline wcpt_temporal_consts wcpt_temporal_make_consts(uint32_t max_history, float normal_min, float depth_tol)
{
    wcpt_temporal_consts k;
    k.max_history = (float)max_history;
    k.normal_min = normal_min;
    k.depth_tol = depth_tol;
    return k;
}

/* ---- the camera: host only, binary64 ---------------------------------------------------------------------------------- */
/* inverse(M) of the header comment for an n x n matrix, n <= 4, row-major; 0 when singular */
static inline int wcpt_temporal_invert(const double* m, int n, double* out)
{
    double t[4][8];
    for (int r = 0; r < n; r++)
        for (int c = 0; c < 2 * n; c++) t[r][c] = c < n ? m[r * n + c] : (c - n == r ? 1.0 : 0.0);
    for (int col = 0; col < n; col++) {
        int piv = col;
        for (int r = col + 1; r < n; r++) {
            const double a = t[r][col] < 0.0 ? -t[r][col] : t[r][col], b = t[piv][col] < 0.0 ? -t[piv][col] : t[piv][col];
            if (a > b) piv = r;
        }
        const double p = t[piv][col] < 0.0 ? -t[piv][col] : t[piv][col];
        if (!(p >= 1e-300)) return 0; /* NaN included */
        if (piv != col)
            for (int c = 0; c < 2 * n; c++) {
                const double s = t[piv][c];
                t[piv][c] = t[col][c];
                t[col][c] = s;
            }
        const double d = t[col][col];
        for (int c = 0; c < 2 * n; c++) t[col][c] = t[col][c] / d;
        for (int r = 0; r < n; r++) {
            if (r == col) continue;
            const double f = t[r][col];
            if (f == 0.0) continue;
            for (int c = 0; c < 2 * n; c++) t[r][c] = t[r][c] - f * t[col][c];
        }
    }
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) out[r * n + c] = t[r][c + n];
    return 1;
}

/* The pixel position (fx, fy) of the offset r in a frame of w x h pixels, in binary64 with the binary32 F; 0 when
 * !(cw > 0) */
static inline int wcpt_temporal_project64(const float F[9], const double r[3], double w, double h, double* fx, double* fy)
{
    const double cx = ((double)F[0] * r[0] + (double)F[1] * r[1]) + (double)F[2] * r[2];
    const double cy = ((double)F[3] * r[0] + (double)F[4] * r[1]) + (double)F[5] * r[2];
    const double cw = ((double)F[6] * r[0] + (double)F[7] * r[1]) + (double)F[8] * r[2];
    if (!(cw > 0.0)) return 0;
    *fx = (cx / cw * 0.5 + 0.5) * w - 0.5;
    *fy = (1.0 - (cy / cw * 0.5 + 0.5)) * h - 0.5;
    return 1;
}

static inline double wcpt_temporal_sqrt64(double v) { return __builtin_sqrt(v); }

/* The camera of a frame of width x height pixels from the scene data's column-major matrices; 0 when it is refused */
static inline int wcpt_temporal_make_camera(const float inverseProjection[16], const float inverseView[16],
                                            const float position[3], uint32_t width, uint32_t height,
                                            wcpt_temporal_camera* out)
{
    double ip[16], a[9], P[16], ai[9];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) ip[r * 4 + c] = (double)inverseProjection[c * 4 + r];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a[r * 3 + c] = (double)inverseView[c * 4 + r];
    if (width == 0 || height == 0 || !wcpt_temporal_invert(ip, 4, P) || !wcpt_temporal_invert(a, 3, ai)) return 0;
    static const int rows[3] = {0, 1, 3};
    wcpt_temporal_camera cam;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double* R = &P[rows[i] * 4];
            cam.F[i * 3 + j] = (float)((R[0] * ai[0 * 3 + j] + R[1] * ai[1 * 3 + j]) + R[2] * ai[2 * 3 + j]);
        }
    for (int c = 0; c < 3; c++) cam.position[c] = position[c];
    const double W = (double)width, H = (double)height;
    for (int corner = 0; corner < 4; corner++) {
        const double x = (corner & 1) ? W - 1.0 : 0.0, y = (corner & 2) ? H - 1.0 : 0.0;
        double cx = x / W + (1.0 / W) * 0.5, cy = y / H + (1.0 / H) * 0.5;
        cy = 1.0 - cy;
        cx = cx * 2.0 - 1.0;
        cy = cy * 2.0 - 1.0;
        double tg[4];
        for (int r = 0; r < 4; r++) tg[r] = ((ip[r * 4 + 0] * cx + ip[r * 4 + 1] * cy) + ip[r * 4 + 2]) + ip[r * 4 + 3];
        double d[3] = {tg[0] / tg[3], tg[1] / tg[3], tg[2] / tg[3]};
        const double dl = wcpt_temporal_sqrt64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        for (int c = 0; c < 3; c++) d[c] = d[c] / dl;
        double wd[3];
        for (int r = 0; r < 3; r++) wd[r] = (a[r * 3 + 0] * d[0] + a[r * 3 + 1] * d[1]) + a[r * 3 + 2] * d[2];
        const double wl = wcpt_temporal_sqrt64((wd[0] * wd[0] + wd[1] * wd[1]) + wd[2] * wd[2]);
        for (int c = 0; c < 3; c++) wd[c] = wd[c] / wl;
        double fx, fy;
        if (!wcpt_temporal_project64(cam.F, wd, W, H, &fx, &fy)) return 0;
        const double ex = fx - x, ey = fy - y;
        if (!(ex >= -1e-3 && ex <= 1e-3 && ey >= -1e-3 && ey <= 1e-3)) return 0;
    }
    *out = cam;
    return 1;
}

/* ---- per pixel: host and device, binary32 -------------------------------------------------------------------------------- */

/* The two guide rows of a record's twelve words for the camera position `o` of the record's frame */
WCPT_HD void wcpt_temporal_pack(const uint32_t rec[WCPT_TEMPORAL_RECORD_WORDS], const float o[3], uint32_t row0[4],
                                uint32_t row1[4])
{
    const uint32_t kind = rec[7] & 3u; /* kPrimHitKindMask */
    const float t = wcpt_u2f(rec[3]);
    if ((kind != 1u && kind != 2u) || t != t) { /* kPrimHitSphere, kPrimHitTriangle */
        row0[0] = row0[1] = row0[2] = row0[3] = 0u;
        row1[0] = row1[1] = row1[2] = row1[3] = 0u;
        return;
    }
    row0[0] = wcpt_f2u(o[0] + t * wcpt_u2f(rec[0]));
    row0[1] = wcpt_f2u(o[1] + t * wcpt_u2f(rec[1]));
    row0[2] = wcpt_f2u(o[2] + t * wcpt_u2f(rec[2]));
    row0[3] = kind == 1u ? rec[9] : rec[10]; /* a sphere's index, a triangle's draw */
    row1[0] = rec[4];
    row1[1] = rec[5];
    row1[2] = rec[6];
    row1[3] = kind;
}

WCPT_HD int wcpt_temporal_finite(float v) { return (wcpt_f2u(v) & 0x7F800000u) != 0x7F800000u; }

WCPT_HD float wcpt_temporal_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* Steps 2 to 6 of a restart call for the pixel whose record is `rec` and whose packed guide is (row0, row1): `base` and
 * *n_b from the history `hist` of a w x h frame seen by the camera `cam` */
template <class Hist>
WCPT_HD void wcpt_temporal_reproject(const uint32_t rec[WCPT_TEMPORAL_RECORD_WORDS], const uint32_t row0[4],
                                     const uint32_t row1[4], const wcpt_temporal_camera& cam, const Hist& hist, int w, int h,
                                     const wcpt_temporal_consts& k, float base[3], float* n_b)
{
    base[0] = base[1] = base[2] = 0.0f;
    *n_b = 0.0f;
    const bool hit = row1[3] != 0u;
    const float Wp[3] = {wcpt_u2f(row0[0]), wcpt_u2f(row0[1]), wcpt_u2f(row0[2])};
    const float np[3] = {wcpt_u2f(row1[0]), wcpt_u2f(row1[1]), wcpt_u2f(row1[2])};
    const float t = wcpt_u2f(rec[3]);
    float r[3];
    if (hit) {
        r[0] = Wp[0] - cam.position[0];
        r[1] = Wp[1] - cam.position[1];
        r[2] = Wp[2] - cam.position[2];
    } else {
        r[0] = wcpt_u2f(rec[0]);
        r[1] = wcpt_u2f(rec[1]);
        r[2] = wcpt_u2f(rec[2]);
    }
    const float cx = wcpt_temporal_dot(&cam.F[0], r), cy = wcpt_temporal_dot(&cam.F[3], r), cw = wcpt_temporal_dot(&cam.F[6], r);
    if (!(cw > 0.0f)) return;
    const float nx = cx / cw, ny = cy / cw;
    const float wf = (float)w, hf = (float)h;
    const float fx = (nx * 0.5f + 0.5f) * wf - 0.5f;
    const float fy = (1.0f - (ny * 0.5f + 0.5f)) * hf - 0.5f;
    if (!(fx >= -1.0f && fx < wf && fy >= -1.0f && fy < hf)) return;
    const float flx = floorf(fx), fly = floorf(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float ax = fx - flx, ay = fy - fly;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float wt[4] = {bx * by, ax * by, bx * ay, ax * ay};
    const float tol = k.depth_tol * t;
    float acc[3] = {0.0f, 0.0f, 0.0f}, nacc = 0.0f, ws = 0.0f;
    for (int j = 0; j < 4; j++) {
        const int qx = x0 + (j & 1), qy = y0 + (j >> 1);
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
        if (!(wt[j] > 0.0f)) continue;
        const float len = hist.length(qx, qy);
        if (!(len > 0.0f)) continue;
        uint32_t q0[4], q1[4];
        hist.first(qx, qy, q0);
        if (q0[3] != row0[3]) continue;
        hist.second(qx, qy, q1);
        if (q1[3] != row1[3]) continue;
        if (hit) {
            const float nq[3] = {wcpt_u2f(q1[0]), wcpt_u2f(q1[1]), wcpt_u2f(q1[2])};
            if (!(wcpt_temporal_dot(np, nq) >= k.normal_min)) continue;
            const float d[3] = {wcpt_u2f(q0[0]) - Wp[0], wcpt_u2f(q0[1]) - Wp[1], wcpt_u2f(q0[2]) - Wp[2]};
            if (!(fabsf(wcpt_temporal_dot(np, d)) <= tol)) continue;
        }
        float cq[4];
        hist.colour(qx, qy, cq);
        if (!wcpt_temporal_finite(cq[0]) || !wcpt_temporal_finite(cq[1]) || !wcpt_temporal_finite(cq[2])) continue;
        acc[0] = acc[0] + wt[j] * cq[0];
        acc[1] = acc[1] + wt[j] * cq[1];
        acc[2] = acc[2] + wt[j] * cq[2];
        nacc = nacc + wt[j] * len;
        ws = ws + wt[j];
    }
    if (ws > 0.0f) {
        base[0] = acc[0] / ws;
        base[1] = acc[1] / ws;
        base[2] = acc[2] / ws;
        *n_b = nacc / ws;
    }
}

/* The blend of every call: `out` = the new hist texel, *len its stored length */
WCPT_HD void wcpt_temporal_blend(const float cur[4], const float base[3], float n_b, float f, const wcpt_temporal_consts& k,
                                 float out[4], float* len)
{
    const float tot = n_b + f;
    if (n_b == 0.0f) {
        out[0] = cur[0];
        out[1] = cur[1];
        out[2] = cur[2];
    } else {
        const float a = f / tot;
        out[0] = base[0] + (cur[0] - base[0]) * a;
        out[1] = base[1] + (cur[1] - base[1]) * a;
        out[2] = base[2] + (cur[2] - base[2]) * a;
    }
    out[3] = cur[3];
    *len = tot < k.max_history ? tot : k.max_history;
}

#endif
