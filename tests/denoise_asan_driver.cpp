// CPU test driver for tests/test_denoise_host.py: the host loop of wc-path-tracer_amd/csrc/wcpt_denoise.h
// (wcpt_denoise_host in wc-path-tracer_amd/host/wcpt_host.cpp) and the header's functions called directly, under
// AddressSanitizer and UndefinedBehaviorSanitizer. Every image, guide and output is a heap array of exactly the size the
// entry point documents -- 4 floats, 48 bytes, 4 floats, 4 bytes per pixel -- so that a read or write one element
// outside is a report. Frames of 1x1, 3x2 and 37x23 pixels and one narrower than the widest step (5x40, step 32), one to
// six iterations, records of every kind and images with NaN, inf and negative values.
// Any sanitizer report aborts the process; the checks below return 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/wcpt_denoise.h"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

/* records in vertical bands: sky, a sphere per band, two draws; the hit distance and the normal vary with the pixel */
static std::vector<wcpt_primary_hit> records(uint32_t w, uint32_t h, std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<wcpt_primary_hit> r((size_t)w * h);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            wcpt_primary_hit& q = r[(size_t)y * w + x];
            std::memset(&q, 0, sizeof(q));
            q.direction[0] = u(rng);
            q.direction[1] = u(rng);
            q.direction[2] = -1.0f;
            const uint32_t band = (x / 3u + y / 5u) % 4u;
            if (band == 0) {
                q.t = 3.402823466e38f;
                q.kind = WCPT_HIT_MISS;
                continue;
            }
            q.t = 2.0f + 0.25f * u(rng);
            q.normal[0] = 0.1f * u(rng);
            q.normal[1] = 0.1f * u(rng);
            q.normal[2] = 1.0f;
            if (band == 1) {
                q.kind = WCPT_HIT_SPHERE | WCPT_HIT_FRONT;
                q.index = y / 5u;
                q.material = 1;
            } else {
                q.kind = WCPT_HIT_TRIANGLE;
                q.index = x + y;
                q.draw = band - 2u;
            }
        }
    return r;
}

static std::vector<float> noise(uint32_t w, uint32_t h, std::mt19937& rng, bool special)
{
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> img((size_t)w * h * 4);
    for (size_t i = 0; i < img.size(); i++) img[i] = (i % 4 == 3) ? 1.0f : 16.0f * std::pow(u(rng), 4.0f);
    if (special) {
        const float vals[] = {0.0f, 25.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                              -1.0f};
        for (size_t i = 0; i < sizeof(vals) / sizeof(vals[0]) && i < (size_t)w * h; i++) img[4 * i] = vals[i];
    }
    return img;
}

static void frame(uint32_t w, uint32_t h, std::mt19937& rng)
{
    const size_t n = (size_t)w * h;
    const std::vector<wcpt_primary_hit> rec = records(w, h, rng);
    for (uint32_t iterations = 1; iterations <= 6; iterations++)
        for (int special = 0; special < 2; special++) {
            const std::vector<float> img = noise(w, h, rng, special != 0);
            const std::vector<float> before = img;
            std::vector<float> out32(n * 4, -7.0f);
            std::vector<uint8_t> out8(n * 4, 7);
            wcpt_denoise_params p = {iterations, special ? std::numeric_limits<float>::infinity() : 4.0f, 0.5f, 0.05f};
            CHECK(wcpt_denoise_host(img.data(), rec.data(), w, h, &p, out32.data(), out8.data()) == WCPT_SUCCESS);
            CHECK(std::memcmp(img.data(), before.data(), n * 16) == 0);
            for (size_t i = 0; i < n; i++) {
                CHECK(out32[4 * i + 3] == 1.0f && out8[4 * i + 3] == 255);
                if (!special) CHECK(std::isfinite(out32[4 * i]) && std::isfinite(out32[4 * i + 1]) && std::isfinite(out32[4 * i + 2]));
            }
            /* either output alone */
            std::vector<float> only32(n * 4, -7.0f);
            std::vector<uint8_t> only8(n * 4, 7);
            CHECK(wcpt_denoise_host(img.data(), rec.data(), w, h, &p, only32.data(), nullptr) == WCPT_SUCCESS);
            CHECK(wcpt_denoise_host(img.data(), rec.data(), w, h, &p, nullptr, only8.data()) == WCPT_SUCCESS);
            CHECK(std::memcmp(only8.data(), out8.data(), n * 4) == 0);
            if (!special) CHECK(std::memcmp(only32.data(), out32.data(), n * 16) == 0);
        }
    /* a constant image comes back: the display value of 1.0 in every pixel */
    std::vector<float> one(n * 4, 1.0f), out32(n * 4, -7.0f);
    const float in1[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    float want[4];
    wcpt_composite_texel(in1, want);
    wcpt_denoise_params p = {6, 4.0f, 0.5f, 0.05f};
    CHECK(wcpt_denoise_host(one.data(), rec.data(), w, h, &p, out32.data(), nullptr) == WCPT_SUCCESS);
    for (size_t i = 0; i < n; i++) CHECK(std::memcmp(&out32[4 * i], want, 16) == 0);
}

/* the header alone: the packing of each kind, and a texel of a one-pixel frame at the widest step */
static void header()
{
    wcpt_primary_hit q;
    std::memset(&q, 0, sizeof(q));
    q.direction[2] = -1.0f;
    q.t = 2.0f;
    q.normal[2] = 1.0f;
    q.index = 7;
    q.draw = 9;
    uint32_t rec[WCPT_DENOISE_RECORD_WORDS], r0[4], r1[4];
    const uint32_t kinds[] = {WCPT_HIT_MISS, WCPT_HIT_SPHERE, WCPT_HIT_TRIANGLE | WCPT_HIT_FRONT, 3u};
    const uint32_t want_kind[] = {0u, 1u, 2u, 0u}, want_key[] = {0u, 7u, 9u, 0u};
    for (int i = 0; i < 4; i++) {
        q.kind = kinds[i];
        std::memcpy(rec, &q, sizeof(rec));
        wcpt_denoise_pack(rec, 0.05f, r0, r1);
        CHECK(wcpt_denoise_kind(r1[3]) == want_kind[i] && r0[3] == want_key[i]);
        if (want_kind[i]) {
            CHECK(wcpt_u2f(r0[2]) == -2.0f && wcpt_u2f(r1[2]) == 1.0f);
            CHECK(wcpt_u2f(r1[3] & ~WCPT_DENOISE_TRIANGLE_BIT) == 1.0f / ((0.05f * 2.0f) * (0.05f * 2.0f)));
        } else {
            CHECK(r0[0] == 0 && r0[1] == 0 && r0[2] == 0 && r1[0] == 0 && r1[1] == 0 && r1[2] == 0);
        }
    }
    CHECK(wcpt_denoise_params_ok(1, 4.0f, 0.5f, 0.05f) && wcpt_denoise_params_ok(6, INFINITY, 0.5f, 0.05f));
    CHECK(!wcpt_denoise_params_ok(0, 4.0f, 0.5f, 0.05f) && !wcpt_denoise_params_ok(7, 4.0f, 0.5f, 0.05f));
    CHECK(!wcpt_denoise_params_ok(5, NAN, 0.5f, 0.05f) && !wcpt_denoise_params_ok(5, 4.0f, INFINITY, 0.05f));
    CHECK(!wcpt_denoise_params_ok(5, 4.0f, 0.5f, 0.0f) && !wcpt_denoise_params_ok(5, 4.0f, 0.5f, INFINITY));
}

int main()
{
    std::mt19937 rng(7);
    frame(1, 1, rng);
    frame(3, 2, rng);
    frame(37, 23, rng);
    frame(5, 40, rng); /* narrower than steps 4 to 32 */
    header();
    /* refusals write nothing */
    std::vector<float> img(4, 1.0f), out(4, -7.0f);
    wcpt_primary_hit rec;
    std::memset(&rec, 0, sizeof(rec));
    wcpt_denoise_params bad = {0, 4.0f, 0.5f, 0.05f};
    CHECK(wcpt_denoise_host(img.data(), &rec, 1, 1, &bad, out.data(), nullptr) == WCPT_ERROR_INVALID_ARGUMENT);
    CHECK(wcpt_denoise_host(img.data(), &rec, 1, 1, nullptr, out.data(), nullptr) == WCPT_ERROR_INVALID_ARGUMENT);
    CHECK(out[0] == -7.0f && out[3] == -7.0f);
    std::printf("%d failed checks\n", failures);
    return failures ? 1 : 0;
}
