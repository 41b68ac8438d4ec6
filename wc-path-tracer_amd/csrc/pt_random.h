/* pt_random.h -- the PCG stream and RandomDirection of Random.glsl, in both arithmetic modes. Part of pt_device.h. */
#ifndef WCPT_PT_RANDOM_H
#define WCPT_PT_RANDOM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_math.h"
#include "wcpt_libm.h"

namespace wcpt::dev {

/* ---- Random.glsl:10-56 ------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t pcg_hash(uint32_t seed)
{
    const uint32_t state = seed * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
/* rand_pcg's output word is the PCG permutation of the *current* state (Random.glsl:18-24); rand() then
 * overwrites the state with that output (Random.glsl:29-30), discarding the LCG step of :21. */
__device__ __forceinline__ uint32_t pcg_permute(uint32_t state)
{
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
__device__ __forceinline__ float rand_f(uint32_t& state)
{
    const uint32_t x = pcg_permute(state);
    state = x;
    return (float)x * 2.3283064365386963e-10f; /* uintBitsToFloat(0x2f800000u) = 2^-32 */
}

__device__ __forceinline__ float RandomValueNormalDistribution(uint32_t& seed)
{
    const float theta = 2.0f * kPI * rand_f(seed);
    const float rho = sqrt_exact(-2.0f * wcpt_logf_rand(rand_f(seed))); /* == wcpt_logf on rand()'s values */
    return rho * wcpt_cosf_2pi(theta);                              /* == wcpt_cosf on [0, 2*pi] */
}
/* wcpt_libm.h's wcpt_logf_rand and wcpt_cosf_2pi on two arguments at once: the same binary32 operations in the same
 * order per half, with the float arithmetic on packed FP32 instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32
 * for the reciprocal's Newton step) and the integer and rounding steps per half. Bit-identical to the scalar
 * functions (and so to the oracle) by construction; selftest fn 7 checks RandomDirection against the oracle. */
__device__ __forceinline__ v2f bcast2(float s) { v2f r = {s, s}; return r; }
__device__ __forceinline__ v2f logf_rand2(v2f x)
{
    const float ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f;
    const float Lg1 = 0.66666662693f, Lg2 = 0.40000972152f, Lg3 = 0.28498786688f, Lg4 = 0.24279078841f;
    uint32_t ix0 = __float_as_uint(x.x) + (0x3f800000u - 0x3f3504f3u);
    uint32_t ix1 = __float_as_uint(x.y) + (0x3f800000u - 0x3f3504f3u);
    const int k0 = (int)(ix0 >> 23) - 127, k1 = (int)(ix1 >> 23) - 127;
    ix0 = (ix0 & 0x007fffffu) + 0x3f3504f3u;
    ix1 = (ix1 & 0x007fffffu) + 0x3f3504f3u;
    const v2f m = {__uint_as_float(ix0), __uint_as_float(ix1)};
    const v2f f = m - bcast2(1.0f);
    const v2f den = bcast2(2.0f) + f;
    v2f y;
    y.x = __builtin_amdgcn_rcpf(den.x);
    y.y = __builtin_amdgcn_rcpf(den.y);
    const v2f e = __builtin_elementwise_fma(-den, y, bcast2(1.0f));
    const v2f rc = __builtin_elementwise_fma(e, y, y); /* wcpt_rcp1_2 per half */
    const v2f sv = f * rc;
    const v2f z = sv * sv;
    const v2f w = z * z;
    const v2f t1 = w * (bcast2(Lg2) + w * bcast2(Lg4));
    const v2f t2 = z * (bcast2(Lg1) + w * bcast2(Lg3));
    const v2f R = t2 + t1;
    const v2f hfsq = bcast2(0.5f) * f * f;
    const v2f dk = {(float)k0, (float)k1};
    v2f out = sv * (hfsq + R) + dk * bcast2(ln2_lo) - hfsq + f + dk * bcast2(ln2_hi);
    if (x.x == 0.0f) out.x = __uint_as_float(0xff800000u);
    if (x.y == 0.0f) out.y = __uint_as_float(0xff800000u);
    return out;
}
__device__ __forceinline__ float cos_quadrant(int j, float c, float s)
{
    switch (j & 3) {
    case 0: return c;
    case 1: return -s;
    case 2: return -c;
    default: return s;
    }
}
__device__ __forceinline__ v2f cosf_2pi2(v2f ax)
{
    const float two_over_pi = 0.63661977236758134f;
    const float pio2_1 = 1.5703125f, pio2_2 = 4.837512969970703125e-4f, pio2_3 = 7.5497899548e-8f;
    const float S1 = -1.6666654611e-1f, S2 = 8.3321608736e-3f, S3 = -1.9515295891e-4f;
    const float C1 = 4.166664568298827e-2f, C2 = -1.388731625493765e-3f, C3 = 2.443315711809948e-5f;
    const v2f q = ax * bcast2(two_over_pi) + bcast2(0.5f);
    const v2f jf = {floorf(q.x), floorf(q.y)};
    const int j0 = (int)jf.x, j1 = (int)jf.y;
    const v2f r = ((ax - jf * bcast2(pio2_1)) - jf * bcast2(pio2_2)) - jf * bcast2(pio2_3);
    const v2f z = r * r;
    v2f c = ((bcast2(C3) * z + bcast2(C2)) * z + bcast2(C1)) * z * z;
    c = c - bcast2(0.5f) * z;
    c = c + bcast2(1.0f);
    v2f sn = ((bcast2(S3) * z + bcast2(S2)) * z + bcast2(S1)) * z * r;
    sn = sn + r;
    v2f out;
    out.x = cos_quadrant(j0, c.x, sn.x);
    out.y = cos_quadrant(j1, c.y, sn.y);
    return out;
}
/* The fast mode's normal variate (Random.glsl:32-41): ln(u) = log2(u) * ln 2 on v_log_f32, so rho = sqrt(log2(u) *
 * (-2 ln 2)), and cos(2 pi u) = v_cos_f32(u), whose operand is in revolutions. u = 0 gives rho = +inf as in the exact
 * mode (log(0) = -inf). Same draws from the PCG stream, in the same order. */
__device__ __forceinline__ float log_fast(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994530942f; }
__device__ __forceinline__ float cos2pi_fast(float u) { return __builtin_amdgcn_cosf(u); }
__device__ __forceinline__ float normal_fast(uint32_t& seed)
{
    const float u0 = rand_f(seed);
    const float u1 = rand_f(seed);
    const float rho = sqrt_a<kArithFast>(-2.0f * log_fast(u1));
    return rho * cos2pi_fast(u0);
}
template <int A = kArithExact>
__device__ __forceinline__ f3 RandomDirection(uint32_t& seed)
{
    if constexpr (A != kArithExact && WCPT_FAST_TRANS) {
        const float x = normal_fast(seed);
        const float y = normal_fast(seed);
        const float z = normal_fast(seed);
        return normalize_a<A>(mk3(x, y, z));
    } else if constexpr (A != kArithExact) {
        const float x = RandomValueNormalDistribution(seed);
        const float y = RandomValueNormalDistribution(seed);
        const float z = RandomValueNormalDistribution(seed);
        return normalize_a<A>(mk3(x, y, z));
    } else {
    /* Random.glsl:43-56 with the draws in the reference order: theta_x, rho_x, theta_y, rho_y, theta_z, rho_z */
    const float ux0 = rand_f(seed), ux1 = rand_f(seed);
    const float uy0 = rand_f(seed), uy1 = rand_f(seed);
    const v2f theta = bcast2(2.0f * kPI) * (v2f){ux0, uy0};
    const v2f lg = logf_rand2((v2f){ux1, uy1});
    const v2f m2 = bcast2(-2.0f) * lg;
    const v2f rho = {sqrt_exact(m2.x), sqrt_exact(m2.y)};
    const v2f xy = rho * cosf_2pi2(theta);
    const float z = RandomValueNormalDistribution(seed);
    return normalize(mk3(xy.x, xy.y, z));
    }
}

} // namespace wcpt::dev

#endif /* WCPT_PT_RANDOM_H */
