/* pt_shading.h -- what happens to a path after an Intersect (pathTracer.comp:213-280): Fresnel reflectance, the sky, the
 * path state and path_shade. Part of pt_device.h. */
#ifndef WCPT_PT_SHADING_H
#define WCPT_PT_SHADING_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wcpt.h"
#include "pt_counters.h"
#include "pt_geometry.h"
#include "pt_math.h"
#include "pt_random.h"
#include "wcpt_libm.h"

namespace wcpt::dev {

/* pathTracer.comp:213-234 */
template <int A = kArithExact>
__device__ __forceinline__ float CalculateReflectance(f3 inDir, f3 normal, float iorA, float iorB)
{
    const float refractRatio = div_a<A>(iorA, iorB);
    const float cosAngleIn = -dot_a<A>(inDir, normal);
    const float sinSqr = refractRatio * refractRatio * nmad_a<A>(1.0f, cosAngleIn, cosAngleIn);
    if (sinSqr >= 1.0f) return 1.0f;
    const float cosRefr = sqrt_a<A>(1.0f - sinSqr);
    const float dPerp = mad_a<A>(iorA, cosAngleIn, iorB * cosRefr);
    const float dPar = mad_a<A>(iorB, cosAngleIn, iorA * cosRefr);
    if (fminf(dPerp, dPar) < 1e-8f) return 1.0f;
    float rPerp = div_a<A>(msub_a<A>(iorA, cosAngleIn, iorB, cosRefr), dPerp);
    rPerp *= rPerp;
    float rPar = div_a<A>(msub_a<A>(iorB, cosAngleIn, iorA, cosRefr), dPar);
    rPar *= rPar;
    return (rPerp + rPar) / 2.0f;
}

/* pathTracer.comp:236-239 */
__device__ __forceinline__ f3 ray_color(const Ray& r)
{
    const float a = 0.5f * (r.direction.y + 1.0f);
    const float ia = 1.0f - a;
    return mk3(0.5f * ia + 1.0f * a, 0.7f * ia + 1.0f * a, 1.0f * ia + 1.0f * a);
}

/* State of one path between segments: the loop-carried variables of TraceRay (pathTracer.comp:241-245). */
struct PathState {
    Ray ray;
    f3 totalLight;
    f3 transmittance;
    uint32_t bounce; /* loop index i of :245 */
};

template <int A = kArithExact>
__device__ __forceinline__ void path_begin(PathState& ps, f3 origin, f3 dir)
{
    ps.ray.origin = origin;
    ps.ray.direction = dir;
    ps.ray.invDirection = rcp3_a<A>(dir);
    ps.totalLight = mk3(0.0f, 0.0f, 0.0f);
    ps.transmittance = mk3(1.0f, 1.0f, 1.0f);
    ps.bounce = 0;
}

/* The last segment of a pixel's last sample ends the path whatever it samples next: after its emission term
 * (:253) the reference still draws the BSDF sample of :256-280 -- the next direction, transmittance and RNG state --
 * but the loop then exits (:245, :283) and nothing reads them again (the RNG state carries over only into a next
 * sample, :309-310). path_shade returns right after the emission term there: the same radiance
 * bits, without the dead RandomDirection, reflection, normalize and 1/direction. The condition is wave-uniform in
 * the megakernel (the lanes of a wave start every sample together). */
/* Shading after an Intersect (pathTracer.comp:248-280). Returns true when the path is finished, with its
 * radiance in L: on a miss (:248-249) or when the bounce loop is exhausted (:245, :283). lastSample: this is the
 * pixel's last sample (its RNG state is not read after the path). */
template <int A = kArithExact>
__device__ __forceinline__ bool path_shade(PathState& ps, const Hit& h, uint32_t& rng, const wcpt_scene_data& sd,
                                           const wcpt_material* __restrict__ mats, f3& L, bool lastSample)
{
    Ray& ray = ps.ray;
    if (!h.hit) {
        L = ps.totalLight + ray_color(ray) * ps.transmittance;
        return true;
    }
    const wcpt_material& m = mats[h.material];
    const uint32_t mtype = m.type;
    const f3 emission = ld3(m.emission);
    const float emissionStrength = m.emissionStrength;
    const float roughness = m.roughness;
    ps.totalLight = ps.totalLight + (emission * emissionStrength) * ps.transmittance;
    if (lastSample && ps.bounce + 1u > sd.maxBounceCount) { /* the loop's last iteration (:245): nothing below is read */
        L = ps.totalLight;
        return true;
    }

    /* Both branches of :256-280 end in normalize(base + roughness * RandomDirection(rng)) and a new 1/direction.
     * That tail is shared here, after the dielectric-only part (Fresnel, refract and the :273 rand, which must
     * precede RandomDirection in the lane's RNG sequence), so a wave whose lanes hit both kinds of material runs
     * RandomDirection (6 rand, 3 log, 3 cos, 4 sqrt) once instead of once per branch. Every lane performs the
     * reference's operations in the reference's order. */
    const bool metal = mtype == WCPT_MATERIAL_METAL;
    const f3 R = reflect_a<A>(ray.direction, h.normal);
    f3 base = R;
    bool followReflection = true;
    if (!metal) {
        const float ior = m.ior;
        const float etaI = h.front ? 1.0f : ior;
        const float etaT = h.front ? ior : 1.0f;
        const float reflectProb = CalculateReflectance<A>(ray.direction, h.normal, etaI, etaT);
        const f3 T = refract_a<A>(ray.direction, h.normal, div_a<A>(etaI, etaT));
        followReflection = (T.x == 0.0f && T.y == 0.0f && T.z == 0.0f);
        if (!followReflection) followReflection = (rand_f(rng) <= reflectProb); /* :273 short-circuit */
        if (!followReflection) base = T;
    }
    const f3 rd = RandomDirection<A>(rng);
#if WCPT_DUP_RANDDIR
    {
        uint32_t r2 = launder_u(rng);
        const f3 d2 = RandomDirection<A>(r2);
        sink(d2.x + d2.y + d2.z);
    }
#endif
    const f3 dir = normalize_a<A>(axpy_a<A>(base, rd, roughness));
    if (metal) {
        ray.origin = axpy_a<A>(h.p, h.normal, kBias);                         /* :257 */
        ps.transmittance = ps.transmittance * ld3(m.albedo);                  /* :261 */
    } else {
        if (!followReflection && !h.front) {                                  /* :276-278 */
            const f3 e = ((ld3(m.absorption) * -1.0f) * m.absorptionStrength) * h.t;
            ps.transmittance = ps.transmittance * mk3(wcpt_expf(e.x), wcpt_expf(e.y), wcpt_expf(e.z));
        }
        ray.origin = h.p + (kBias * h.normal) * sign1(dot_a<A>(dir, h.normal)); /* :279 */
    }
    ray.direction = dir;
    ray.invDirection = rcp3_a<A>(dir);
    ps.bounce++;
    if (ps.bounce > sd.maxBounceCount) { /* loop exhausted: no sky term (:283) */
        L = ps.totalLight;
        return true;
    }
    return false;
}

} // namespace wcpt::dev

#endif /* WCPT_PT_SHADING_H */
