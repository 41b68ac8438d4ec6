// CPU test driver for tests/test_mk_tiny_rule_sanitizers.py: the tiny-tree classifier
// (wc-path-tracer_amd/csrc/mk_tiny_rule.h, the function the device scan runs on a draw's BVH buffer) under
// AddressSanitizer and UndefinedBehaviorSanitizer, on node arrays of exactly the size it is told -- trees of the host
// builders (wc-path-tracer_amd/host/wcpt_host.cpp), every prefix of them, and random node words -- so a read past the
// nodes it may touch is a report. Any sanitizer report aborts the process; the checks below return 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/mk_tiny_rule.h"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

/* the rule on a heap copy of exactly n nodes (n = 0: a null pointer) */
static uint32_t classify(const wcpt_node* src, uint64_t n, uint32_t lim3)
{
    std::vector<wcpt_node> exact(src, src + n);
    return wcpt::mk_tiny_leaves(n ? exact.data() : nullptr, n, lim3);
}

/* what the rule must say, written independently of it */
static uint32_t expected(const wcpt_node* nd, uint64_t n, uint32_t lim3)
{
    auto leaf_ok = [&](const wcpt_node& k) {
        return k.triangleCount != 0 && k.leftNodeOrTriangleIndex % 3 == 0 &&
               (uint64_t)k.leftNodeOrTriangleIndex + k.triangleCount <= lim3;
    };
    if (n == 0) return 0;
    if (nd[0].triangleCount != 0) return leaf_ok(nd[0]) ? 1 : 0;
    const uint64_t l = nd[0].leftNodeOrTriangleIndex;
    if (l + 1 >= n) return 0;
    return leaf_ok(nd[l]) && leaf_ok(nd[l + 1]) ? 2 : 0;
}

static void built_trees(std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    for (uint32_t tris = 1; tris <= 40; tris++) {
        for (int rep = 0; rep < 4; rep++) {
            std::vector<float> pos(9 * tris);
            /* rep 0: a stack with one centroid (a root leaf); else random soup around a few centres */
            for (uint32_t t = 0; t < tris; t++)
                for (int v = 0; v < 3; v++)
                    for (int c = 0; c < 3; c++)
                        pos[9 * t + 3 * v + c] = rep == 0 ? (c == 2 ? (v == 2 ? 2.0f : -1.0f) : (c == 1 ? (v == 0 ? -1.0f : (v == 1 ? 1.0f : 0.0f)) : 3.0f + 0.01f * t))
                                                          : u(rng) * 0.2f + (float)((t * (rep + 1)) % 3);
            std::vector<uint32_t> idx(3 * tris);
            for (uint32_t i = 0; i < 3 * tris; i++) idx[i] = i;
            const uint32_t cap = 2 * tris + 1;
            for (int sah = 0; sah < 2; sah++) {
                std::vector<uint32_t> ix = idx;
                std::vector<wcpt_node> nodes(cap);
                uint32_t used = 0;
                const int rc = sah ? wcpt_bvh_build_sah(pos.data(), 3 * tris, ix.data(), 3 * tris, nodes.data(), cap, &used)
                                   : wcpt_bvh_build(pos.data(), 3 * tris, ix.data(), 3 * tris, nodes.data(), cap, &used);
                CHECK(rc == WCPT_SUCCESS);
                if (rc != WCPT_SUCCESS) continue;
                const uint32_t got = classify(nodes.data(), used, 3 * tris);
                CHECK(got == expected(nodes.data(), used, 3 * tris));
                CHECK((used == 1) == (got == 1));
                CHECK(used <= 3 || got == 0); /* a child of the root is interior */
                if (rep == 0 && !sah) CHECK(used == 1 && got == 1);
                /* a buffer that holds fewer nodes than the tree, and fewer records than the leaves need */
                for (uint32_t n = 0; n <= used; n++) CHECK(classify(nodes.data(), n, 3 * tris) == expected(nodes.data(), n, 3 * tris));
                for (uint32_t lim3 : {0u, 3u, 3u * tris - 3u, 3u * tris - 1u, 3u * tris + 3u})
                    CHECK(classify(nodes.data(), used, lim3) == expected(nodes.data(), used, lim3));
            }
        }
    }
}

static void random_nodes(std::mt19937& rng)
{
    const uint32_t edge[] = {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 9u, 51u, 0x7FFFFFFFu, 0xFFFFFFFCu, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    std::uniform_int_distribution<int> pick(0, (int)(sizeof(edge) / sizeof(edge[0])) - 1);
    for (int it = 0; it < 20000; it++) {
        const uint64_t n = (uint64_t)(rng() % 9u);
        std::vector<wcpt_node> nodes(n);
        for (wcpt_node& k : nodes) {
            std::memset(&k, 0, sizeof(k));
            k.leftNodeOrTriangleIndex = edge[pick(rng)];
            k.triangleCount = (rng() & 1u) ? 0u : edge[pick(rng)];
        }
        const uint32_t lim3 = edge[pick(rng)];
        CHECK(classify(nodes.data(), n, lim3) == expected(nodes.data(), n, lim3));
    }
}

int main()
{
    std::mt19937 rng(20240611u);
    built_trees(rng);
    random_nodes(rng);
    CHECK(wcpt::mk_tiny_enabled(-1, 2) && wcpt::mk_tiny_enabled(1, 1) && !wcpt::mk_tiny_enabled(0, 2) && !wcpt::mk_tiny_enabled(1, 0));
    std::printf("%d failed checks\n", failures);
    return failures ? 1 : 0;
}
