// CPU test driver for tests/test_host_sanitizers.py: the product's host utilities
// (wc-path-tracer_amd/host/wcpt_host.cpp: OBJ loader, midpoint and SAH BVH builders, camera, scene generators), built
// together with this file under AddressSanitizer and UndefinedBehaviorSanitizer (sanitizers on the host
// side), exercised on the reference's own mesh, malformed OBJ text, random and degenerate triangle soups, undersized
// node arrays and every scene generator. Any sanitizer report aborts the process; the checks below return 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/frame_prep.h"
#include "../wc-path-tracer_amd/csrc/mk_variant.h"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

/* Structural checks of a built tree: children inside the used nodes, leaves inside the index range. */
static void check_tree(const std::vector<wcpt_node>& nodes, uint32_t used, uint32_t index_count)
{
    CHECK(used >= 1 && used <= nodes.size());
    uint64_t leaf_indices = 0;
    for (uint32_t i = 0; i < used; i++) {
        const wcpt_node& n = nodes[i];
        if (n.triangleCount == 0) {
            CHECK(n.leftNodeOrTriangleIndex > i && n.leftNodeOrTriangleIndex + 1 < used);
        } else {
            CHECK(n.triangleCount % 3 == 0);
            CHECK((uint64_t)n.leftNodeOrTriangleIndex + n.triangleCount <= index_count);
            leaf_indices += n.triangleCount;
        }
    }
    CHECK(leaf_indices == index_count); /* every triangle in exactly one leaf */
}

static void build_both(const std::vector<float>& pos, std::vector<uint32_t> idx)
{
    const uint32_t nv = (uint32_t)(pos.size() / 3), ni = (uint32_t)idx.size();
    const uint32_t cap = 2 * ni / 3 + 1;
    for (int sah = 0; sah < 2; sah++) {
        std::vector<uint32_t> ix = idx;
        std::vector<wcpt_node> nodes(cap);
        uint32_t used = 0;
        const int rc = sah ? wcpt_bvh_build_sah(pos.data(), nv, ix.data(), ni, nodes.data(), cap, &used)
                           : wcpt_bvh_build(pos.data(), nv, ix.data(), ni, nodes.data(), cap, &used);
        CHECK(rc == WCPT_SUCCESS);
        if (rc == WCPT_SUCCESS) check_tree(nodes, used, ni);
        /* an array too small for the tree: an error, never a write past it */
        if (used > 1) {
            std::vector<uint32_t> iy = idx;
            std::vector<wcpt_node> small(used - 1);
            uint32_t u2 = 0;
            const int r2 = sah ? wcpt_bvh_build_sah(pos.data(), nv, iy.data(), ni, small.data(), used - 1, &u2)
                               : wcpt_bvh_build(pos.data(), nv, iy.data(), ni, small.data(), used - 1, &u2);
            CHECK(r2 != WCPT_SUCCESS);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s mushroom.obj\n", argv[0]);
        return 2;
    }
    /* 1. the reference's mesh: load, build, write back as OBJ, parse again */
    wcpt_mesh m = {};
    CHECK(wcpt_obj_load(argv[1], &m) == WCPT_SUCCESS);
    CHECK(m.vertex_count > 0 && m.index_count > 0 && m.index_count % 3 == 0);
    {
        std::vector<float> pos(m.positions, m.positions + 3ull * m.vertex_count);
        std::vector<uint32_t> idx(m.indices, m.indices + m.index_count);
        build_both(pos, idx);
        char* text = nullptr;
        uint64_t len = 0;
        CHECK(wcpt_mesh_to_obj(&m, &text, &len) == WCPT_SUCCESS);
        wcpt_mesh m2 = {};
        CHECK(wcpt_obj_parse(text, len, &m2) == WCPT_SUCCESS);
        CHECK(m2.index_count == m.index_count);
        wcpt_mesh_free(&m2);
        wcpt_string_free(text);
    }
    wcpt_mesh_free(&m);
    CHECK(wcpt_obj_load("/nonexistent/file.obj", &m) != WCPT_SUCCESS);

    /* 2. malformed and edge-case OBJ text: an error code or a mesh, never a bad access */
    const char* cases[] = {
        "", "\n\n\n", "v", "v 1 2", "v 1 2 3", "f 1 2 3", "v 0 0 0\nf 1 1", "v 0 0 0\nf 0 1 2", "v 0 0 0\nf -1 -1 -1",
        "v 0 0 0\nf -5 -6 -7", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 99999999999",
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/1/1 2/2/2 3/3/3", "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/1",
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1", "v nan inf -inf\nv 1 0 0\nv 0 1 0\nf 1 2 3",
        "v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3\r\n", "# comment only\n", "v 1e40 1e-40 -0\nv 1 0 0\nv 0 1 0\nf 1 2 3",
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 3 4 1 2 3 4 1 2", "f", "f //", "f 1/", "v 0 0 0\nf 1 1 1 1 1 1 1",
        "o name\ng group\nusemtl m\ns off\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3", "v\t0\t0\t0\nv 1 0 0\nv 0 1 0\nf 1\t2\t3",
    };
    for (const char* c : cases) {
        wcpt_mesh t = {};
        const int rc = wcpt_obj_parse(c, std::strlen(c), &t);
        if (rc == WCPT_SUCCESS) {
            CHECK(t.index_count % 3 == 0);
            for (uint32_t i = 0; i < t.index_count; i++) CHECK(t.indices[i] < t.vertex_count);
        }
        wcpt_mesh_free(&t);
    }
    {   /* a long line and a text without a terminating newline, parsed from an exact-length buffer */
        std::string big = "v 0 0 0\nv 1 0 0\nv 0 1 0\nf";
        for (int i = 0; i < 20000; i++) big += " 1 2 3";
        std::vector<char> exact(big.begin(), big.end());
        wcpt_mesh t = {};
        (void)wcpt_obj_parse(exact.data(), exact.size(), &t);
        wcpt_mesh_free(&t);
    }
    {   /* random bytes */
        std::mt19937 rng(1234);
        for (int k = 0; k < 200; k++) {
            std::vector<char> buf(rng() % 512);
            const char alphabet[] = "vf/ -0123456789.e\n#\r\tnaixt";
            for (char& ch : buf) ch = alphabet[rng() % (sizeof(alphabet) - 1)];
            wcpt_mesh t = {};
            const int rc = wcpt_obj_parse(buf.data(), buf.size(), &t);
            if (rc == WCPT_SUCCESS)
                for (uint32_t i = 0; i < t.index_count; i++) CHECK(t.indices[i] < t.vertex_count);
            wcpt_mesh_free(&t);
        }
    }

    /* 3. triangle soups: random, all-coincident, collinear, one triangle, large */
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(-10.0f, 10.0f);
    for (int k = 0; k < 40; k++) {
        const uint32_t nv = 3 + rng() % 300, nt = 1 + rng() % 400;
        std::vector<float> pos(3ull * nv);
        for (float& f : pos) f = U(rng);
        if (k % 5 == 1) std::fill(pos.begin(), pos.end(), 1.5f);                       /* every vertex the same */
        if (k % 5 == 2)
            for (uint32_t v = 0; v < nv; v++) pos[3 * v + 1] = pos[3 * v + 2] = 0.0f;  /* collinear */
        std::vector<uint32_t> idx(3ull * nt);
        for (uint32_t& i : idx) i = rng() % nv;
        build_both(pos, idx);
    }
    {
        const uint32_t nt = 60000;
        std::vector<float> pos(9ull * nt);
        for (float& f : pos) f = U(rng);
        std::vector<uint32_t> idx(3ull * nt);
        for (uint32_t i = 0; i < idx.size(); i++) idx[i] = i;
        build_both(pos, idx);
    }
    {   /* argument errors */
        float p[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
        uint32_t ix[3] = {0, 1, 5};
        wcpt_node n[4];
        uint32_t used = 0;
        CHECK(wcpt_bvh_build(p, 3, ix, 3, n, 4, &used) != WCPT_SUCCESS); /* index past the vertices */
        CHECK(wcpt_bvh_build(p, 3, ix, 2, n, 4, &used) != WCPT_SUCCESS); /* not a multiple of 3 */
        CHECK(wcpt_bvh_build(nullptr, 3, ix, 3, n, 4, &used) != WCPT_SUCCESS);
    }

    /* 4. every scene generator, and the camera at its edges */
    const char* scenes[] = {"default", "default_dielectric", "default_emissive", "cornell", "atrium", "no-such-scene"};
    for (const char* name : scenes) {
        wcpt_scene s = {};
        const int rc = wcpt_scene_generate(name, 0, &s);
        CHECK((rc == WCPT_SUCCESS) == (std::strcmp(name, "no-such-scene") != 0));
        if (rc == WCPT_SUCCESS && s.mesh.index_count) {
            for (uint32_t i = 0; i < s.mesh.index_count; i++) CHECK(s.mesh.indices[i] < s.mesh.vertex_count);
            if (s.mesh.index_count < 30000) {
                std::vector<float> pos(s.mesh.positions, s.mesh.positions + 3ull * s.mesh.vertex_count);
                build_both(pos, std::vector<uint32_t>(s.mesh.indices, s.mesh.indices + s.mesh.index_count));
            }
        }
        if (rc == WCPT_SUCCESS) {
            for (float aspect : {1e-6f, 1.0f, 16.0f / 9.0f, 1e6f}) {
                wcpt_camera cam = s.camera;
                CHECK(wcpt_camera_update(&cam, aspect) == WCPT_SUCCESS);
            }
            wcpt_camera cam = s.camera;
            CHECK(wcpt_camera_update(&cam, 0.0f) != WCPT_SUCCESS);
            CHECK(wcpt_camera_update(&cam, std::nanf("")) != WCPT_SUCCESS);
        }
        wcpt_scene_free(&s);
    }

    /* 5. the megakernel's variant selection (mk_variant.h, host only): every selection over its inputs' cross product,
     * out-of-range ones included, is built, and its number indexes the dispatcher's table */
    for (int mode = -1; mode <= 3; mode++)
        for (int stack = -1; stack <= 2; stack++)
            for (uint32_t draws = 0; draws <= 2; draws++)
                for (uint32_t samples : {0u, 1u, 2u, 16u, 0xFFFFFFFFu})
                    for (int pc = -1; pc <= 3; pc++)
                        for (int arith = -1; arith <= 2; arith++)
                            for (int k = 0; k < 4; k++) {
                                const wcpt::MkSelection s = wcpt::mk_variant_select(mode, stack, (k & 1) != 0, draws,
                                                                                     samples, pc, arith, (k & 2) != 0);
                                CHECK(s.n == 1u || s.n == 2u);
                                for (uint32_t i = 0; i < s.n; i++) {
                                    CHECK(wcpt::mk_variant_built(s.v[i]));
                                    CHECK(wcpt::mk_variant_code(s.v[i]) < wcpt::kMkVariantCodes);
                                }
                            }

    /* 6. frame preparation's rules (frame_prep.h, host only) at their boundaries: no overflow, no shift past a word */
    for (uint32_t ntri : {0u, 1u, 2u, 5u, 6u, 1u << 26, 0xFFFFFFFFu / 3u}) {
        const wcpt::RecordLayout l = wcpt::record_layout(ntri);
        CHECK(l.pair_offset % 256u == 0u && l.pair_offset >= 48ull * ntri && l.bytes >= l.pair_offset + 40ull * ntri);
        CHECK(l.prim_pairs == ((uint64_t)ntri + 1u) / 2u && l.prim_bytes == 112u * l.prim_pairs);
    }
    CHECK(wcpt::vertex_bound(true, ~0ull) == 0xFFFFFFFFu && wcpt::vertex_bound(true, 35) == 2u);
    CHECK(wcpt::vertex_bound(false, 0) == 0xFFFFFFFFu);
    CHECK(wcpt::bvh_node_count(false, ~0ull) == wcpt::kNodesUnknown && wcpt::bvh_node_count(true, ~0ull) == ~0ull / 32u);
    CHECK(wcpt::leaf_estimate(true, ~0ull, 7) == (~0ull / 32u + 1u) / 2u && wcpt::leaf_estimate(false, ~0ull, 7) == 7u);
    for (uint64_t nodes : {(uint64_t)0, (uint64_t)3, ((uint64_t)1 << 24) - 1u, (uint64_t)1 << 24, wcpt::kNodesUnknown})
        for (uint32_t ic : {0u, 102u, (1u << 24) - 1u, 1u << 24, 0xFFFFFFFFu})
            for (uint32_t scan = 0; scan < 8u; scan++)
                for (int tiny = -1; tiny <= 1; tiny++)
                    for (int k = 0; k < 4; k++) {
                        const bool fits = nodes < (1ull << 24) && ic < (1u << 24);
                        CHECK(wcpt::draw_needs_scan(k & 1, (k & 2) != 0, nodes, ic) == (k == 3 && fits));
                        const wcpt::DrawWords w = wcpt::draw_words(k & 1, (k & 2) != 0, nodes, ic, scan, tiny, 0xFFFFFFFFu);
                        CHECK((uint32_t)w.word2 == ic / 3u && (w.flags >> 32) == 0xFFFFFFFFu);
                        CHECK(((w.flags & wcpt::kTriFlagPackedRefs) != 0u) == ((k & 1) && fits));
                        CHECK((w.word2 >> 32) == ((k & 1) && fits ? nodes : 0u));
                        if (k != 3 || !fits) CHECK((w.flags & 0xFFFFFFFCull) == 0u);
                    }
    CHECK(wcpt::check_draw_args(30, 1, 1, true, 120) == wcpt::kDrawArgsOk);
    CHECK(wcpt::check_draw_args(33, 1, 1, true, 120) == wcpt::kDrawIndexCountPastBuffer);
    CHECK(wcpt::check_draw_args(0xFFFFFFFFu, 1, 1, true, ~0ull) == wcpt::kDrawArgsOk);
    CHECK(wcpt::check_draw_args(0xFFFFFFFFu, 1, 1, true, 0) == wcpt::kDrawIndexCountPastBuffer);
    CHECK(wcpt::check_draw_args(2, 0, 0, false, 0) == wcpt::kDrawArgsOk);
    CHECK(wcpt::check_draw_args(3, 0, 1, false, 0) == wcpt::kDrawNullBuffer);
    for (uint32_t n : {0u, 1u, 2u, 0xFFFFFFFFu})
        for (uint64_t tris : {0ull, 7ull, 8ull, 1ull << 26, (1ull << 26) + 1u, ~0ull})
            for (uint64_t leaves : {0ull, 2ull, ~0ull})
                for (int pair = -1; pair <= 1; pair++)
                    for (int kernel = 0; kernel <= 2; kernel++) {
                        const wcpt::FramePlan p = wcpt::frame_plan(n, ~0ull, ~0ull, tris, leaves, tris, pair, kernel);
                        CHECK(p.kernel_run == WCPT_KERNEL_MEGAKERNEL || p.kernel_run == WCPT_KERNEL_WAVEFRONT);
                        CHECK(kernel == WCPT_KERNEL_AUTO || p.kernel_run == kernel);
                        CHECK(p.want_primary == (p.pair_records && p.kernel_run == WCPT_KERNEL_MEGAKERNEL));
                        CHECK((p.wf_fast || p.tiny_tree) == (n == 1u));
                        if (n == 0u || tris > wcpt::kPairMaxTriangles || pair == 0) CHECK(!p.pair_records);
                    }
    std::printf("host sanitizer driver: %d failed checks\n", failures);
    return failures ? 1 : 0;
}
