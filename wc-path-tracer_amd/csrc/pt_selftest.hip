/*
 * pt_selftest.hip — the device self-tests (wcpt.h wcpt_selftest, wcpt_selftest_geometry): kernels that evaluate the
 * device definitions of pt_device.h -- the RNG, the deterministic libm, the reciprocal and square root, and the
 * composite geometry and shading functions in both arithmetic modes -- on host inputs, as the render kernels call
 * them. A translation unit of its own, compiled with pt_kernels.hip's flags, so the render kernels' one stays about
 * rendering.
 */
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace wcpt {
namespace dev {

/* Device self-tests: evaluate the device definitions of the RNG and the deterministic libm on host inputs. */
__global__ __launch_bounds__(256) void pt_selftest(int fn, const uint32_t* __restrict__ in, const uint32_t* __restrict__ in2,
                                                   uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t a = in[i];
    switch (fn) {
    case 0: out[i] = pcg_hash(a); break;
    case 1: {
        uint32_t s = a;
        for (int k = 0; k < 4; k++) out[4u * i + (uint32_t)k] = __float_as_uint(rand_f(s));
        break;
    }
    case 2: out[i] = __float_as_uint(wcpt_logf(__uint_as_float(a))); break;
    case 3: out[i] = __float_as_uint(wcpt_cosf(__uint_as_float(a))); break;
    case 4: out[i] = __float_as_uint(wcpt_expf(__uint_as_float(a))); break;
    case 5: out[i] = __float_as_uint(sqrt_exact(__uint_as_float(a))); break;
    case 6: out[i] = __float_as_uint(__uint_as_float(a) / __uint_as_float(in2[i])); break;
    case 8: { /* exhaustive fast-reciprocal check: mismatches of rcp_exact's fast path vs IEEE 1/x over the 2^16
                 inputs (a << 16) | k inside the fast path's range */
        uint32_t bad = 0;
        for (uint32_t k = 0; k < 65536u; k++) {
            const float x = __uint_as_float((a << 16) | k);
            const float ax = fabsf(x);
            if (!(ax >= 0x1p-126f && ax < 0x1p126f)) continue;
            const float y = __builtin_amdgcn_rcpf(x);
            const float e = __builtin_fmaf(-x, y, 1.0f);
            const float r = __builtin_fmaf(e, y, y);
            bad += (__float_as_uint(r) != __float_as_uint(1.0f / x)) ? 1u : 0u;
        }
        out[i] = bad;
        break;
    }
    case 9: out[i] = __float_as_uint(rcp_exact(__uint_as_float(a))); break;
    case 10:   /* as 8, over every normal binary32 input (v_cmp_class range test) */
    case 11: { /* as 8, over every input (no range test) */
        uint32_t bad = 0;
        for (uint32_t k = 0; k < 65536u; k++) {
            const float x = __uint_as_float((a << 16) | k);
            if (fn == 10 && !__builtin_isnormal(x)) continue;
            const float y = __builtin_amdgcn_rcpf(x);
            const float e = __builtin_fmaf(-x, y, 1.0f);
            const float r = __builtin_fmaf(e, y, y);
            const float q = 1.0f / x;
            bad += (__float_as_uint(r) != __float_as_uint(q) && !(r != r && q != q)) ? 1u : 0u;
        }
        out[i] = bad;
        break;
    }
    case 12: { /* the kernels' reciprocals vs the IEEE quotient over the 2^16 inputs x = (a << 16) | k: rcp_exact(x), and
                  rcp2_exact on the pair (x, ~x) (every bit pattern in both halves); mismatches, NaN == NaN */
        uint32_t bad = 0;
        for (uint32_t k = 0; k < 65536u; k++) {
            const uint32_t bits = (a << 16) | k;
            const float x = __uint_as_float(bits), x2 = __uint_as_float(~bits);
            const float r = rcp_exact(x);
            v2f xx;
            xx.x = x;
            xx.y = x2;
            const v2f rr = rcp2_exact(xx);
            const float q = 1.0f / x, q2 = 1.0f / x2;
            bad += (__float_as_uint(r) != __float_as_uint(q) && !(r != r && q != q)) ? 1u : 0u;
            bad += (__float_as_uint(rr.x) != __float_as_uint(q) && !(rr.x != rr.x && q != q)) ? 1u : 0u;
            bad += (__float_as_uint(rr.y) != __float_as_uint(q2) && !(rr.y != rr.y && q2 != q2)) ? 1u : 0u;
        }
        out[i] = bad;
        break;
    }
    case 13: { /* how many of the 2^16 inputs (a << 16) | k fail the fast result's class check (general division) */
        uint32_t slow = 0;
        for (uint32_t k = 0; k < 65536u; k++)
            slow += rcp_fast_ok(rcp_fast_raw(__uint_as_float((a << 16) | k))) ? 0u : 1u;
        out[i] = slow;
        break;
    }
    case 14: { /* acceptance tests on (u, v) = (in, in2) with t = 1: bit 0 = accept_tri, bit 1 = accept_tri_w */
        const float u = __uint_as_float(a), v = __uint_as_float(in2[i]);
        const float uv = u + v;
        out[i] = (accept_tri(1.0f, u, v, uv) ? 1u : 0u) | (accept_tri_w(1.0f, u, v, 1.0f - uv) ? 2u : 0u);
        break;
    }
    case 15: { /* the kernels' sqrt (sqrt_exact) vs hipcc's correctly rounded sqrtf over the 2^16 inputs (a << 16) | k:
                  mismatches, NaN == NaN */
        uint32_t bad = 0;
        for (uint32_t k = 0; k < 65536u; k++) {
            const float x = __uint_as_float((a << 16) | k);
            const float r = sqrt_exact(x), q = sqrtf(x);
            bad += (__float_as_uint(r) != __float_as_uint(q) && !(r != r && q != q)) ? 1u : 0u;
        }
        out[i] = bad;
        break;
    }
    case 17: { /* the take's two forms (pt_device.h take_bits) over t = (a << 16) | k, k < 2^16, for rec.t = in2: mismatches
                  between (t > 0 && t < rec.t) and bits(t) - 1 < bits(rec.t) - 1 */
        const float rt = __uint_as_float(in2[i]);
        const uint32_t rb = take_bits(rt);
        uint32_t bad = 0;
        for (uint32_t k = 0; k < 65536u; k++) {
            const float t = __uint_as_float((a << 16) | k);
            bad += ((t > 0.0f && t < rt) != (take_bits(t) < rb)) ? 1u : 0u;
        }
        out[i] = bad;
        break;
    }
    case 16: { /* GLSL vector / scalar as the kernels evaluate it (pt_device.h operator/): in * RN(1 / in2) */
        const f3 q = mk3(__uint_as_float(a), 0.0f, 0.0f) / __uint_as_float(in2[i]);
        out[i] = __float_as_uint(q.x);
        break;
    }
    case 7: { /* RandomDirection: 3 words per input */
        uint32_t s = a;
        const f3 d = RandomDirection(s);
        out[3u * i + 0u] = __float_as_uint(d.x);
        out[3u * i + 1u] = __float_as_uint(d.y);
        out[3u * i + 2u] = __float_as_uint(d.z);
        break;
    }
    /* the fast arithmetic mode's device functions (pt_device.h kArithFast), mirroring fn 2, 3, 5, 9 and 7 */
    case 18: out[i] = __float_as_uint(log_fast(__uint_as_float(a))); break;
    case 19: out[i] = __float_as_uint(cos2pi_fast(__uint_as_float(a))); break; /* cos(2 pi u) given u */
    case 20: out[i] = __float_as_uint(sqrt_a<kArithFast>(__uint_as_float(a))); break;
    case 21: out[i] = __float_as_uint(rcp_a<kArithFast>(__uint_as_float(a))); break;
    case 22: { /* fast RandomDirection: 3 words per input */
        uint32_t s = a;
        const f3 d = RandomDirection<kArithFast>(s);
        out[3u * i + 0u] = __float_as_uint(d.x);
        out[3u * i + 1u] = __float_as_uint(d.y);
        out[3u * i + 2u] = __float_as_uint(d.z);
        break;
    }
    default: break;
    }
}

/* Geometry self-tests: the composite device functions of the render kernels, called as those kernels call them, in the
 * arithmetic mode A (wcpt.h wcpt_selftest_geometry lists the fn numbers and the words of an item). The runtime checks
 * fn, in_words and out_words, so item i owns in[i * in_words ..) and out[i * out_words ..). One kernel per function
 * and mode: each is a few dozen instructions (and hipcc 7.2's register allocator crashes on all of them in one switch). */
template <int A, int FN>
__global__ __launch_bounds__(256) void pt_selftest_geometry(const uint32_t* __restrict__ in, uint32_t in_words,
                                                            uint32_t* __restrict__ out, uint32_t out_words, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t* x = in + (uint64_t)i * in_words;
    uint32_t* y = out + (uint64_t)i * out_words;
    auto f = [&](uint32_t k) { return __uint_as_float(x[k]); };
    auto v3 = [&](uint32_t k) { return mk3(f(k), f(k + 1u), f(k + 2u)); };
    auto put = [&](uint32_t k, float v) { y[k] = __float_as_uint(v); };
    auto put3 = [&](uint32_t k, f3 v) { put(k, v.x); put(k + 1u, v.y); put(k + 2u, v.z); };
    Ray r; /* fn 0..4 and 7 start with origin, direction (fn 5 and 6 have fewer words: nothing else is read for them;
              fn 8 brings its own invDirection) */
    if constexpr (FN <= 4 || FN == 7) {
        r.origin = v3(0);
        r.direction = v3(3);
        r.invDirection = rcp3_a<A>(r.direction);
    }
    if constexpr (FN == 0) { /* origin, direction, a, b, c */
        const f3 a = v3(6), b = v3(9), c = v3(12);
        put(0, rayTriangleE<A>(r, a, b - a, c - a));
    } else if constexpr (FN == 1 || FN == 2) { /* origin, direction, then (a, e1, e2) of the pair's two triangles */
        TriPair p;
        p.ax = v2f{f(6), f(15)};   p.ay = v2f{f(7), f(16)};   p.az = v2f{f(8), f(17)};
        p.e1x = v2f{f(9), f(18)};  p.e1y = v2f{f(10), f(19)}; p.e1z = v2f{f(11), f(20)};
        p.e2x = v2f{f(12), f(21)}; p.e2y = v2f{f(13), f(22)}; p.e2z = v2f{f(14), f(23)};
        PairHit h;
        if constexpr (FN == 1) {
            h = rayTrianglePair<A>(r, p);
        } else { /* the primary-ray record of this origin, as build_primary_pairs derives it */
            float t0[7], t1[7];
            primary_terms(r.origin.x, r.origin.y, r.origin.z, p.ax.x, p.ay.x, p.az.x, p.e1x.x, p.e1y.x, p.e1z.x, p.e2x.x,
                          p.e2y.x, p.e2z.x, t0);
            primary_terms(r.origin.x, r.origin.y, r.origin.z, p.ax.y, p.ay.y, p.az.y, p.e1x.y, p.e1y.y, p.e1z.y, p.e2x.y,
                          p.e2y.y, p.e2z.y, t1);
            TriPairP q;
            q.e1x = p.e1x; q.e1y = p.e1y; q.e1z = p.e1z;
            q.e2x = p.e2x; q.e2y = p.e2y; q.e2z = p.e2z;
            q.oax = v2f{t0[0], t1[0]}; q.oay = v2f{t0[1], t1[1]}; q.oaz = v2f{t0[2], t1[2]};
            q.qx = v2f{t0[3], t1[3]};  q.qy = v2f{t0[4], t1[4]};  q.qz = v2f{t0[5], t1[5]};
            q.tq = v2f{t0[6], t1[6]};
            h = rayTrianglePairP<A>(r, q);
        }
        put(0, h.t.x);
        put(1, h.t.y);
        y[2] = h.hit0 ? 1u : 0u;
        y[3] = h.hit1 ? 1u : 0u;
    } else if constexpr (FN == 3) { /* origin, direction, centre, radius */
        put(0, raySphereNear<A>(r, v3(6), f(9)));
    } else if constexpr (FN == 4) { /* origin, direction, t, centre, radius: the hit epilogue of a sphere */
        wcpt_sphere s;
        s.position[0] = f(7); s.position[1] = f(8); s.position[2] = f(9);
        s.radius = f(10);
        s.material = 0u;
        const Hit h = resolve_hit<kShadeA<A>>(r, f(6), kSpherePrim, 0u, &s, nullptr, nullptr);
        put3(0, h.p);
        put3(3, h.normal);
        y[6] = h.front ? 1u : 0u;
    } else if constexpr (FN == 5) { /* direction, normal, iorA, iorB: the optics of path_shade's dielectric branch */
        constexpr int S = kShadeA<A>;
        const f3 d = v3(0), nrm = v3(3);
        const float iorA = f(6), iorB = f(7);
        put3(0, reflect_a<S>(d, nrm));
        put3(3, refract_a<S>(d, nrm, div_a<S>(iorA, iorB)));
        put(6, CalculateReflectance<S>(d, nrm, iorA, iorB));
    } else if constexpr (FN == 6) { /* a 3-vector: normalize and the component reciprocals (path_shade's new direction) */
        constexpr int S = kShadeA<A>;
        put3(0, normalize_a<S>(v3(0)));
        put3(3, rcp3_a<S>(v3(0)));
    } else if constexpr (FN == 7) { /* origin, direction, Hit p, normal, t, front, one material (15 words), rng state,
                                       transmittance: one path_shade step that is neither the last segment nor a miss */
        static_assert(sizeof(wcpt_material) == 60, "15 words");
        uint32_t mw[15];
        for (uint32_t k = 0; k < 15u; k++) mw[k] = x[14u + k];
        wcpt_material m;
        __builtin_memcpy(&m, mw, sizeof(m));
        PathState ps;
        ps.ray = r;
        ps.totalLight = mk3(0.0f, 0.0f, 0.0f);
        ps.transmittance = v3(30);
        ps.bounce = 0;
        Hit h;
        h.p = v3(6);
        h.normal = v3(9);
        h.t = f(12);
        h.front = x[13] != 0u;
        h.hit = true;
        h.material = 0;
        wcpt_scene_data sd = {};
        sd.maxBounceCount = 1000u;
        uint32_t rng = x[29];
        f3 L;
        (void)path_shade<kShadeA<A>>(ps, h, rng, sd, &m, L, false);
        put3(0, ps.ray.origin);
        put3(3, ps.ray.direction);
        put3(6, ps.transmittance);
        y[9] = rng;
    } else if constexpr (FN == 8) { /* origin, invDirection, the left and the right child's box (min, max), rec.t: the
                                       child-pair decision, and the root cull of the left box (no fast form: A is unused) */
        r.origin = v3(0);
        r.direction = mk3(0.0f, 0.0f, 0.0f); /* the box test reads invDirection alone */
        r.invDirection = v3(3);
        auto box = [&](uint32_t k) {
            NodeV n; /* {min.xyz, max.x | max.yz, left, count} */
            n.a = v4f{f(k), f(k + 1u), f(k + 2u), f(k + 3u)};
            n.b = v4u{x[k + 4u], x[k + 5u], 0u, 0u};
            return n;
        };
        const NodeV L = box(6), R = box(12);
        const ChildPair c = child_pair(r, L, R);
        y[0] = c.leftFirst ? 1u : 0u;
        y[1] = c.passL ? 1u : 0u;
        y[2] = c.passR ? 1u : 0u;
        put(3, c.l0);
        put(4, c.r0);
        y[5] = root_survives(r, L, f(18)) ? 1u : 0u;
    }
}

} // namespace dev

hipError_t launch_selftest(int fn, const uint32_t* in, const uint32_t* in2, uint32_t* out, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::pt_selftest, dim3((n + 255u) / 256u), dim3(256), 0, stream, fn, in, in2, out, n);
    return hipGetLastError();
}

bool selftest_geometry_words(int fn, uint32_t& in_words, uint32_t& out_words)
{
    static const uint32_t words[9][2] = {{15, 1}, {24, 4}, {24, 4}, {10, 1}, {11, 7}, {8, 7}, {3, 6}, {33, 10}, {19, 6}};
    if (fn < 0 || fn > 8) return false;
    in_words = words[fn][0];
    out_words = words[fn][1];
    return true;
}

hipError_t launch_selftest_geometry(int fn, int arith, const uint32_t* in, uint32_t in_words, uint32_t* out,
                                    uint32_t out_words, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const dim3 grid((n + 255u) / 256u), block(256);
#define WCPT_GEOMETRY_CASE(FN)                                                                                          \
    case FN:                                                                                                            \
        if (arith == WCPT_ARITH_FAST)                                                                                   \
            hipLaunchKernelGGL((dev::pt_selftest_geometry<dev::kArithFast, FN>), grid, block, 0, stream, in, in_words, \
                               out, out_words, n);                                                                      \
        else                                                                                                            \
            hipLaunchKernelGGL((dev::pt_selftest_geometry<dev::kArithExact, FN>), grid, block, 0, stream, in, in_words, \
                               out, out_words, n);                                                                      \
        break;
    switch (fn) {
        WCPT_GEOMETRY_CASE(0)
        WCPT_GEOMETRY_CASE(1)
        WCPT_GEOMETRY_CASE(2)
        WCPT_GEOMETRY_CASE(3)
        WCPT_GEOMETRY_CASE(4)
        WCPT_GEOMETRY_CASE(5)
        WCPT_GEOMETRY_CASE(6)
        WCPT_GEOMETRY_CASE(7)
        WCPT_GEOMETRY_CASE(8)
    default: return hipErrorInvalidValue;
    }
#undef WCPT_GEOMETRY_CASE
    return hipGetLastError();
}

} // namespace wcpt
