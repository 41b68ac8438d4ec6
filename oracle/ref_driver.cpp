/*
 * ref_driver.cpp — runs the reference's own compute shaders on the CPU.  TEST INFRASTRUCTURE ONLY.
 *
 * The three shaders are translated mechanically (oracle/ref_translate.py) into oracle/_ref/gen/ and included here, each in
 * a namespace of its own inside namespace glsl (two of them define Epsilon), behind the types and built-ins of
 * oracle/glsl_cpu.hpp. One invocation is one call of the shader's main with gl_GlobalInvocationID set; there are no
 * barriers and no shared memory, so the invocations run one after another. Neither the translated text nor anything
 * compiled from it is committed: `make -C oracle ref` builds oracle/_ref/libwcpt_ref.so where the reference is present.
 *
 * The reference's traversal stack is a real uint[32] here: a caller must not render a case whose traversal goes deeper
 * (the oracle counts ref_stack_max and ref_stack_overflow_segments for that purpose).
 */
#include "glsl_cpu.hpp"

namespace glsl {
namespace pt {
#include "pathTracer.comp.inc"
}
namespace comp {
#include "composite.comp.inc"
}
namespace bloom {
#include "bloom.comp.inc"
}
}  // namespace glsl

using namespace glsl;

/* scalar block layout: what the host writes is what the shader's structs read */
static_assert(sizeof(pt::SceneData) == 164, "SceneData");
static_assert(sizeof(pt::Material) == 60, "Material");
static_assert(sizeof(pt::Sphere) == 20, "Sphere");
static_assert(sizeof(pt::Node) == 32, "Node");
static_assert(sizeof(pt::DrawCommand) == 32, "DrawCommand");
static_assert(sizeof(vec3) == 12 && sizeof(vec4) == 16 && sizeof(mat4) == 64, "vectors");

/* One draw command with host pointers (the layout of oracle_draw in pt_oracle.c). */
struct ref_draw {
    const float* vertices;
    const uint32_t* indices;
    const void* bvh;
};

/* A texture's levels, float4 texels (the layout of glsl::texture_levels). */
typedef texture_levels ref_texture;

extern "C" {

/* pathTracer.comp over rows [y0, y0 + rows) of a W x H image; `image` holds those rows (float4, read and written). */
void ref_render(const void* scene_data, const void* materials, const void* spheres, const ref_draw* draws, uint32_t n_draws,
                float* image, uint32_t W, uint32_t H, uint32_t y0, uint32_t rows)
{
    pt::DrawCommand* dc = new pt::DrawCommand[n_draws ? n_draws : 1]();
    for (uint32_t i = 0; i < n_draws; i++) {
        dc[i].vertexBP.vertices = (vec3*)draws[i].vertices;
        dc[i].indexBP.indices = (uint*)draws[i].indices;
        dc[i].bvhBP.bvh = (pt::Node*)draws[i].bvh;
        dc[i].indexCount = 0;                     /* not read by the shader */
    }
    bind_block(pt::sdp, (pt::SceneData*)scene_data);
    pt::mbp.materials = (pt::Material*)materials;
    pt::sphereBP.spheres = (pt::Sphere*)spheres;
    pt::drawCommandBP.drawCommands = dc;
    pt::o_Image = image2D{image, (int)W, (int)H, (int)y0};
    for (uint32_t y = y0; y < y0 + rows; y++)
        for (uint32_t x = 0; x < W; x++) {
            gl_GlobalInvocationID = uvec3(x, y, 0);
            pt::main_pathTracer();
        }
    delete[] dc;
}

/* composite.comp: `image` (W x H float4) is screenTexture; `bloom` (bw x bh float4) is bloomTexture, or null: Bloom off. */
void ref_composite(const float* image, const float* bloom, uint32_t bw, uint32_t bh, uint32_t W, uint32_t H, float* out)
{
    texture_levels screen{}, bl{};
    screen.data[0] = image; screen.w[0] = (int)W; screen.h[0] = (int)H;
    bl.data[0] = bloom; bl.w[0] = (int)bw; bl.h[0] = (int)bh;
    comp::screenTexture = sampler2D{&screen};
    comp::bloomTexture = sampler2D{&bl};
    comp::Bloom = bloom != nullptr;
    comp::o_Image = image2D{out, (int)W, (int)H, 0};
    destination_size = ivec2((int)W, (int)H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            gl_GlobalInvocationID = uvec3(x, y, 0);
            comp::main_composite();
        }
}

/* One dispatch of bloom.comp over a w x h output image. */
void ref_bloom_dispatch(int mode, const float* params4, float lod, const ref_texture* u_texture,
                        const ref_texture* u_bloom_texture, float* out, uint32_t w, uint32_t h)
{
    bloom::Params = vec4(params4[0], params4[1], params4[2], params4[3]);
    bloom::LOD = lod;
    bloom::Mode = mode;
    bloom::u_Texture = sampler2D{u_texture};
    bloom::u_BloomTexture = sampler2D{u_bloom_texture};
    bloom::o_Image = image2D{out, (int)w, (int)h, 0};
    destination_size = ivec2((int)w, (int)h);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            gl_GlobalInvocationID = uvec3(x, y, 0);
            bloom::main_bloom();
        }
}

/* ---- the shader's own functions, one item per call ---------------------------------------------------------------- */
uint32_t ref_pcg_hash(uint32_t seed) { return pt::pcg_hash(seed); }
float ref_rand(uint32_t* state) { return pt::rand(*state); }
void ref_random_direction(uint32_t* state, float* out3)
{
    const vec3 d = pt::RandomDirection(*state);
    out3[0] = d.x; out3[1] = d.y; out3[2] = d.z;
}
static pt::Ray make_ray(const float* o, const float* d, const float* inv)
{
    return pt::Ray(vec3(o[0], o[1], o[2]), vec3(d[0], d[1], d[2]), vec3(inv[0], inv[1], inv[2]));
}
/* n items: origin, direction and invDirection as given (3 floats each) */
void ref_ray_box(const float* o, const float* d, const float* inv, const float* bmin, const float* bmax, float* out2,
                 uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const float *B0 = bmin + 3 * i, *B1 = bmax + 3 * i;
        const vec2 t = pt::rayBoxIntersect(make_ray(o + 3 * i, d + 3 * i, inv + 3 * i), vec3(B0[0], B0[1], B0[2]),
                                           vec3(B1[0], B1[1], B1[2]));
        out2[2 * i] = t.x; out2[2 * i + 1] = t.y;
    }
}
void ref_ray_sphere(const float* o, const float* d, const float* c, const float* radius, float* out2, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const float* C = c + 3 * i;
        const vec2 t = pt::raySphereIntersect(make_ray(o + 3 * i, d + 3 * i, d + 3 * i), vec3(C[0], C[1], C[2]), radius[i]);
        out2[2 * i] = t.x; out2[2 * i + 1] = t.y;
    }
}
void ref_ray_triangle(const float* o, const float* d, const float* a, const float* b, const float* c, float* out3,
                      uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const float *A = a + 3 * i, *B = b + 3 * i, *C = c + 3 * i;
        const vec3 t = pt::rayTriangleIntersect(make_ray(o + 3 * i, d + 3 * i, d + 3 * i), vec3(A[0], A[1], A[2]),
                                                vec3(B[0], B[1], B[2]), vec3(C[0], C[1], C[2]));
        out3[3 * i] = t.x; out3[3 * i + 1] = t.y; out3[3 * i + 2] = t.z;
    }
}
void ref_reflectance(const float* in_dir, const float* normal, const float* ior_a, const float* ior_b, float* out, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const float *I = in_dir + 3 * i, *N = normal + 3 * i;
        out[i] = pt::CalculateReflectance(vec3(I[0], I[1], I[2]), vec3(N[0], N[1], N[2]), ior_a[i], ior_b[i]);
    }
}
/* the two built-ins TraceRay calls around CalculateReflectance, as the prelude defines them */
void ref_reflect_refract(const float* in_dir, const float* normal, const float* eta, float* out6, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const float *I = in_dir + 3 * i, *N = normal + 3 * i;
        const vec3 r = reflect(vec3(I[0], I[1], I[2]), vec3(N[0], N[1], N[2]));
        const vec3 t = refract(vec3(I[0], I[1], I[2]), vec3(N[0], N[1], N[2]), eta[i]);
        float* q = out6 + 6 * i;
        q[0] = r.x; q[1] = r.y; q[2] = r.z; q[3] = t.x; q[4] = t.y; q[5] = t.z;
    }
}

}  // extern "C"
