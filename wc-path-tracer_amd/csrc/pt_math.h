/* pt_math.h -- global-address pointer types, the constants of constants.glsl, the f3 vector math with the correctly
 * rounded reciprocal and square root, and the arithmetic modes (WCPT_OPTION_ARITH: the *_a helpers, kFuse, WCPT_FAST_*).
 * Part of pt_device.h. */
#ifndef WCPT_PT_MATH_H
#define WCPT_PT_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wcpt.h"

namespace wcpt::dev {

/* Scene buffers are reached through device addresses stored in DrawCommands (buffer device addresses in the
 * reference, pathTracer.comp:82-88). Casting them to address-space-1 (global) pointers makes hipcc emit
 * global_load_* instead of flat_load_*: flat loads count against lgkmcnt as well as vmcnt, so every LDS
 * stack access would otherwise also wait for outstanding node fetches. */
#define WCPT_GLOBAL __attribute__((address_space(1)))
typedef const WCPT_GLOBAL wcpt_node* gnode_ptr;
typedef const WCPT_GLOBAL uint32_t* gu32_ptr;
typedef const WCPT_GLOBAL float* gf32_ptr;
__device__ __forceinline__ gnode_ptr as_nodes(uint64_t a) { return (gnode_ptr)(uintptr_t)a; }
__device__ __forceinline__ gu32_ptr as_u32(uint64_t a) { return (gu32_ptr)(uintptr_t)a; }
__device__ __forceinline__ gf32_ptr as_f32(uint64_t a) { return (gf32_ptr)(uintptr_t)a; }

/* constants.glsl:4-9 */
constexpr float kBias = 1e-5f;
constexpr float kInfinity = 3.402823466e+38f;
constexpr float kPI = 3.14159265358979323846264338327950288f;

struct f3 { float x, y, z; };

__device__ __forceinline__ f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 operator*(float s, f3 a) { return mk3(s * a.x, s * a.y, s * a.z); }
/* Correctly rounded reciprocal 1/x: v_rcp_f32 followed by one FMA Newton step, with the general division for the
 * inputs where that fast sequence is not the IEEE quotient. 3 VALU + 1 check instead of the 11 of hipcc's
 * division sequence.
 *
 * The fast sequence equals 1.0f / x for every |x| in [2^-126, 2^126) (all 2^32 bit patterns checked on gfx950:
 * tools/rcp_exhaustive.hip and selftest fn 8/10). Outside that range it returns zero (|x| >= 2^126: the denormal
 * quotient is flushed) or NaN (x zero, denormal, infinite or NaN), never a normal number. So the fast result is
 * validated on its own class (one v_cmp_class): a normal result is the IEEE quotient, anything else takes the
 * general division. Checked over all 2^32 inputs: selftest fn 12 (0 mismatches), which also runs the packed pair
 * form rcp2_exact. */
__device__ __forceinline__ float rcp_fast_raw(float x)
{
    const float y = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, y, 1.0f);
    return __builtin_fmaf(e, y, y);
}
__device__ __forceinline__ bool rcp_fast_ok(float r) { return __builtin_isnormal(r); }
__device__ __forceinline__ float rcp_exact(float x)
{
    const float r = rcp_fast_raw(x);
    if (__builtin_expect(rcp_fast_ok(r), 1)) return r;
    return 1.0f / x;
}
typedef float v2f __attribute__((ext_vector_type(2)));
/* rcp_exact of both halves: two v_rcp_f32, the Newton step as two packed FMAs (v_pk_fma_f32: two independent
 * binary32 fused multiply-adds, the same operations as the scalar step) and one branch for both fallbacks. */
__device__ __forceinline__ v2f rcp2_exact(v2f x)
{
    v2f y;
    y.x = __builtin_amdgcn_rcpf(x.x);
    y.y = __builtin_amdgcn_rcpf(x.y);
    const v2f one = {1.0f, 1.0f};
    const v2f e = __builtin_elementwise_fma(-x, y, one);
    v2f r = __builtin_elementwise_fma(e, y, y);
    const bool okx = rcp_fast_ok(r.x), oky = rcp_fast_ok(r.y);
    if (__builtin_expect(!(okx && oky), 0)) {
        if (!okx) r.x = 1.0f / x.x;
        if (!oky) r.y = 1.0f / x.y;
    }
    return r;
}
__device__ __forceinline__ f3 rcp3(f3 a) { return mk3(rcp_exact(a.x), rcp_exact(a.y), rcp_exact(a.z)); }
/* GLSL vector / scalar (normalize, the sphere normal :145, target.xyz / target.w :301, result / samples :312):
 * v * RN(1/s) with the correctly rounded reciprocal, one reciprocal and three multiplies instead of three
 * correctly rounded divisions. Vulkan allows 2.5 ULP for GLSL division; this is <= 1.5 ULP, and the oracle
 * defines vector / scalar the same way (oracle/pt_oracle.c div3s), so the two stay bit-identical. */
__device__ __forceinline__ f3 operator/(f3 a, float s)
{
    const float r = rcp_exact(s);
    return mk3(a.x * r, a.y * r, a.z * r);
}
/* GLSL dot: (x*x' + y*y') + z*z' */
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
/* GLSL cross (4.50 spec §8.5) */
__device__ __forceinline__ f3 cross(f3 a, f3 b)
{
    return mk3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
/* Correctly rounded sqrt. hipcc's sqrtf is v_sqrt_f32 (not correctly rounded alone) + a one-ulp correction from two
 * FMA residuals, wrapped in a 2^32 scaling for inputs below 2^-96 and a zero/infinity class fixup: 17 VALU. For
 * x >= 2^-96 (including +inf) the correction alone is the IEEE square root -- checked against sqrtf over every such
 * input on the device (selftest fn 15) -- so that range takes the 9-VALU core and everything else (tiny, zero,
 * negative, NaN) the full sequence. */
__device__ __forceinline__ float sqrt_core(float x)
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __uint_as_float(__float_as_uint(s) - 1u);
    const float s_up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_dn = __builtin_fmaf(-s_dn, s, x);
    const float r_up = __builtin_fmaf(-s_up, s, x);
    float r = (r_dn <= 0.0f) ? s_dn : s;
    r = (r_up > 0.0f) ? s_up : r;
    return r;
}
__device__ __forceinline__ float sqrt_exact(float x)
{
    if (__builtin_expect(x >= 0x1p-96f, 1)) return sqrt_core(x);
    return sqrtf(x);
}
__device__ __forceinline__ f3 normalize(f3 v) { return v / sqrt_exact(dot(v, v)); }
__device__ __forceinline__ f3 reflect(f3 I, f3 N) { return I - N * (2.0f * dot(N, I)); }
__device__ __forceinline__ f3 refract(f3 I, f3 N, float eta)
{
    const float d = dot(N, I);
    const float k = 1.0f - eta * eta * (1.0f - d * d);
    if (k < 0.0f) return mk3(0.0f, 0.0f, 0.0f);
    return eta * I - N * (eta * d + sqrt_exact(k));
}
__device__ __forceinline__ float sign1(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

/* ---- arithmetic modes (WCPT_OPTION_ARITH) ---------------------------------------------------------------------
 * kArithExact is everything above and below as written: the reference's operand order, unfused, correctly rounded
 * reciprocal and square root, software log / cos -- bit-identical to the oracle. kArithFast is the megakernel's render
 * builds only (the A template parameter, a distinct kernel symbol per mode) and relaxes, piece by piece:
 *   WCPT_FAST_FMA    dot and cross products of the triangle tests, reflect / refract / Fresnel sums, normalize and
 *                    `p + t * d` as fused multiply-adds (the sphere test's stay unfused, see WCPT_FAST_FMA_SPHERE),
 *                    written out (__builtin_fmaf, __builtin_elementwise_fma = v_pk_fma_f32). Every translation unit
 *                    stays on -ffp-contract=off: which products fuse is defined here, once per formula, never chosen by
 *                    the compiler per call site -- the uniform and the per-lane leaf loops, every instantiation and every
 *                    tile order evaluate the same helper, so a pixel's bits do not depend on which pixels share its wave
 *                    (fast against fast stays bit for bit across row splits, tile orders, stacks, pipes and groups).
 *   WCPT_FAST_RCP    1/x and v / s as the bare v_rcp_f32 (1 ULP): no Newton step, class check or fallback branch.
 *   WCPT_FAST_SQRT   sqrt as the bare v_sqrt_f32 (1 ULP).
 *   WCPT_FAST_TRANS  RandomValueNormalDistribution's log as v_log_f32 x ln 2 and its cos(2 pi u) as v_cos_f32(u) (the
 *                    instruction takes revolutions: the 2 pi multiply and the range reduction both go).
 * Each switch set to 0 keeps that piece exact in the fast kernels, so an A/B can price it (tools/ab_build.sh).
 * (WCPT_FAST_RCP=0 does not build with ROCm 7.2: hipcc's register allocator crashes on one fast instantiation.)
 * Unchanged in both modes: the PCG stream, every integer decision (take_bits, the minimum3 acceptance, the sign
 * pre-reject), the traversal order, the slab test's (plane - origin) * inv form, wcpt_expf, the primary ray, the frame
 * accumulation, store_pixel / display_rgba8 and the derived records as the runtime builds them. */
constexpr int kArithExact = 0, kArithFast = 1;
#ifndef WCPT_FAST_FMA
#define WCPT_FAST_FMA 1
#endif
#ifndef WCPT_FAST_RCP
#define WCPT_FAST_RCP 1
#endif
#ifndef WCPT_FAST_SQRT
#define WCPT_FAST_SQRT 1
#endif
#ifndef WCPT_FAST_TRANS
#define WCPT_FAST_TRANS 1
#endif
/* Where the fused forms apply, site by site: the triangle tests and the shading arithmetic (default: WCPT_FAST_FMA) and
 * the sphere test (default 0). A site switched off evaluates the fast mode's other pieces on the exact mode's unfused
 * formulas (kArithFastUnfused, internal: never a kernel's A).
 * The sphere test stays unfused because its near root -b - sqrt(b * b - c), c = dot(oc, oc) - r * r, is dominated by
 * cancellation on a large sphere: on the reference scene's ground sphere (r = 100) dot(oc, oc) and b * b are ~1e4 (one
 * ULP ~1e-3) and c ~1e2, so rounding one product less moves t by ~1e-5 relative -- a hundred times the ULP-level
 * differences of every other relaxation, and more than the kBias offset of the next origin -- without being any more
 * accurate. Measured (MI355X, diverged pixels against the oracle, sphere products fused / unfused): the reference's scene
 * 52x44 x 6 frames 20 / 6 of 2288, 128x96 34 / 8 of 12288, 256x192 133 / 54 of 49152; default_dielectric 128x96 28 / 8;
 * the Cornell box 128x96 14 / 9. With the triangle or the shading products unfused instead, the reference's scene stays
 * at 20 / 17 of 2288. Four sphere tests per segment are a small share of the VALU work. */
#ifndef WCPT_FAST_FMA_TRI
#define WCPT_FAST_FMA_TRI WCPT_FAST_FMA
#endif
#ifndef WCPT_FAST_FMA_SPHERE
#define WCPT_FAST_FMA_SPHERE 0
#endif
#ifndef WCPT_FAST_FMA_SHADE
#define WCPT_FAST_FMA_SHADE WCPT_FAST_FMA
#endif
constexpr int kArithFastUnfused = 2;
template <int A> constexpr bool kFuse = A == kArithFast;
template <int A> constexpr int kTriA = (A == kArithFast && !(WCPT_FAST_FMA_TRI)) ? kArithFastUnfused : A;
template <int A> constexpr int kSphereA = (A == kArithFast && !(WCPT_FAST_FMA_SPHERE)) ? kArithFastUnfused : A;
template <int A> constexpr int kShadeA = (A == kArithFast && !(WCPT_FAST_FMA_SHADE)) ? kArithFastUnfused : A;
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
template <int A>
__device__ __forceinline__ float rcp_a(float x)
{
    if constexpr (A != kArithExact && WCPT_FAST_RCP) return __builtin_amdgcn_rcpf(x);
    else return rcp_exact(x);
}
template <int A>
__device__ __forceinline__ v2f rcp2_a(v2f x)
{
    if constexpr (A != kArithExact && WCPT_FAST_RCP) {
        v2f r;
        r.x = __builtin_amdgcn_rcpf(x.x);
        r.y = __builtin_amdgcn_rcpf(x.y);
        return r;
    } else {
        return rcp2_exact(x);
    }
}
template <int A>
__device__ __forceinline__ f3 rcp3_a(f3 a) { return mk3(rcp_a<A>(a.x), rcp_a<A>(a.y), rcp_a<A>(a.z)); }
template <int A>
__device__ __forceinline__ float sqrt_a(float x)
{
    if constexpr (A != kArithExact && WCPT_FAST_SQRT) return __builtin_amdgcn_sqrtf(x);
    else return sqrt_exact(x);
}
/* a / b of two scalars: the IEEE quotient, or a * rcp(b) */
template <int A>
__device__ __forceinline__ float div_a(float a, float b)
{
    if constexpr (A != kArithExact && WCPT_FAST_RCP) return a * __builtin_amdgcn_rcpf(b);
    else return a / b;
}
template <int A>
__device__ __forceinline__ f3 div3_a(f3 a, float s)
{
    const float r = rcp_a<A>(s);
    return mk3(a.x * r, a.y * r, a.z * r);
}
/* a * b + c and a * b - c * d as one formula per mode */
template <int A>
__device__ __forceinline__ float mad_a(float a, float b, float c)
{
    if constexpr (kFuse<A>) return __builtin_fmaf(a, b, c);
    else return a * b + c;
}
template <int A>
__device__ __forceinline__ float msub_a(float a, float b, float c, float d) /* a * b - c * d */
{
    if constexpr (kFuse<A>) return __builtin_fmaf(a, b, -(c * d));
    else return a * b - c * d;
}
template <int A>
__device__ __forceinline__ float nmad_a(float c, float a, float b) /* c - a * b */
{
    if constexpr (kFuse<A>) return __builtin_fmaf(-a, b, c);
    else return c - a * b;
}
template <int A>
__device__ __forceinline__ float madn_a(float a, float b, float c) /* a * b - c */
{
    if constexpr (kFuse<A>) return __builtin_fmaf(a, b, -c);
    else return a * b - c;
}
template <int A>
__device__ __forceinline__ v2f nmad2_a(v2f c, v2f a, v2f b)
{
    if constexpr (kFuse<A>) return fma2(-a, b, c);
    else return c - a * b;
}
template <int A>
__device__ __forceinline__ v2f madn2_a(v2f a, v2f b, v2f c)
{
    if constexpr (kFuse<A>) return fma2(a, b, -c);
    else return a * b - c;
}
template <int A>
__device__ __forceinline__ v2f msub2_a(v2f a, v2f b, v2f c, v2f d)
{
    if constexpr (kFuse<A>) return fma2(a, b, -(c * d));
    else return a * b - c * d;
}
/* (x * x' + y * y') + z * z'; fused: fma(z, z', fma(y, y', x * x')) */
template <int A>
__device__ __forceinline__ float dot_a(f3 a, f3 b)
{
    if constexpr (kFuse<A>) return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
    else return dot(a, b);
}
template <int A>
__device__ __forceinline__ v2f dot2_a(v2f ax, v2f ay, v2f az, v2f bx, v2f by, v2f bz)
{
    if constexpr (kFuse<A>) return fma2(az, bz, fma2(ay, by, ax * bx));
    else return (ax * bx + ay * by) + az * bz;
}
template <int A>
__device__ __forceinline__ f3 cross_a(f3 a, f3 b)
{
    if constexpr (kFuse<A>)
        return mk3(msub_a<A>(a.y, b.z, b.y, a.z), msub_a<A>(a.z, b.x, b.z, a.x), msub_a<A>(a.x, b.y, b.x, a.y));
    else return cross(a, b);
}
/* a + b * s per component (p + t * d, base + roughness * rd, p + n * bias) */
template <int A>
__device__ __forceinline__ f3 axpy_a(f3 a, f3 b, float s)
{
    if constexpr (kFuse<A>)
        return mk3(__builtin_fmaf(b.x, s, a.x), __builtin_fmaf(b.y, s, a.y), __builtin_fmaf(b.z, s, a.z));
    else return a + b * s;
}
template <int A>
__device__ __forceinline__ f3 normalize_a(f3 v)
{
    if constexpr (A != kArithExact) return div3_a<A>(v, sqrt_a<A>(dot_a<A>(v, v)));
    else return normalize(v);
}
template <int A>
__device__ __forceinline__ f3 reflect_a(f3 I, f3 N)
{
    if constexpr (kFuse<A>) {
        const float k = -2.0f * dot_a<A>(N, I);
        return axpy_a<A>(I, N, k);
    } else {
        return reflect(I, N);
    }
}
template <int A>
__device__ __forceinline__ f3 refract_a(f3 I, f3 N, float eta)
{
    if constexpr (A != kArithExact) {
        const float d = dot_a<A>(N, I);
        const float k = nmad_a<A>(1.0f, eta * eta, nmad_a<A>(1.0f, d, d)); /* 1 - eta^2 (1 - d^2) */
        if (k < 0.0f) return mk3(0.0f, 0.0f, 0.0f);
        const float c = -mad_a<A>(eta, d, sqrt_a<A>(k));
        return axpy_a<A>(eta * I, N, c);
    } else {
        return refract(I, N, eta);
    }
}
__device__ __forceinline__ f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ f3 ld3(gf32_ptr p) { return mk3(p[0], p[1], p[2]); } /* global_load_dwordx3 */
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

} // namespace wcpt::dev

#endif /* WCPT_PT_MATH_H */
