// CPU test driver for tests/test_temporal_host.py: the host chain of wc-path-tracer_amd/csrc/wcpt_temporal.h
// (wcpt_temporal_host in wc-path-tracer_amd/host/wcpt_host.cpp) and the header's functions called directly, under
// AddressSanitizer and UndefinedBehaviorSanitizer. Every image, guide, plane and output is a heap array of exactly the size
// the entry point documents -- 4 floats, 48 bytes, 1 float, 3 floats per pixel -- so that a read or write one element
// outside is a report. Frames of 1x1, 3x2, 37x23 and 5x40 pixels; chains of restarts with the camera still, yawing,
// shifted, turned away and looking at records whose points lie anywhere (behind the camera, at infinity, NaN), so that
// the reprojected position is out of the frame, not finite or negative in every way; histories with NaN, inf and
// negative values; the refusals, which write nothing.
// Any sanitizer report aborts the process; the checks below return 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/wcpt_temporal.h"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

static wcpt_scene_data scene_of(float px, float py, float pz, float yaw, uint32_t w, uint32_t h)
{
    wcpt_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position[0] = px;
    cam.position[1] = py;
    cam.position[2] = pz;
    cam.yaw = yaw;
    cam.fov = 90.0f;
    CHECK(wcpt_camera_update(&cam, (float)w / (float)h) == WCPT_SUCCESS);
    wcpt_scene_data sd;
    std::memset(&sd, 0, sizeof(sd));
    std::memcpy(sd.inverseProjection, cam.inverseProjection, sizeof(sd.inverseProjection));
    std::memcpy(sd.inverseView, cam.inverseView, sizeof(sd.inverseView));
    std::memcpy(sd.position, cam.position, sizeof(sd.position));
    return sd;
}

/* records in vertical bands: sky, a sphere per band, two draws. `wild`: directions and distances of any size and sign,
 * NaN and infinities among them, so that the points lie anywhere; `forward`: the x of the other records' directions (the
 * cameras look along +x at yaw 0) */
static std::vector<wcpt_primary_hit> records(uint32_t w, uint32_t h, std::mt19937& rng, bool wild, float forward = 1.0f)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    const float odd[] = {0.0f, -0.0f, 1.0e30f, -1.0e30f, std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(), 1.0e-30f};
    std::vector<wcpt_primary_hit> r((size_t)w * h);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            wcpt_primary_hit& q = r[(size_t)y * w + x];
            std::memset(&q, 0, sizeof(q));
            q.direction[0] = forward;
            q.direction[1] = u(rng);
            q.direction[2] = u(rng);
            const uint32_t band = (x / 3u + y / 5u) % 4u;
            if (wild) {
                q.direction[0] = u(rng);
                if ((x + y) % 3u == 0) q.direction[rng() % 3u] = odd[rng() % 8u];
            }
            if (band == 0) {
                q.t = 3.402823466e38f;
                q.kind = WCPT_HIT_MISS;
                continue;
            }
            q.t = 2.0f + 0.25f * u(rng);
            if (wild && (x + y) % 2u == 0) q.t = odd[rng() % 8u];
            q.normal[0] = -1.0f;
            q.normal[1] = 0.1f * u(rng);
            q.normal[2] = 0.1f * u(rng);
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

struct State {
    std::vector<float> rgba, length, base, n_b;
    std::vector<wcpt_primary_hit> rec;
    wcpt_scene_data sd;
    bool valid = false;
};

/* one call of the chain; the new state replaces `s` */
static void call(State& s, uint32_t w, uint32_t h, const std::vector<float>& img, uint32_t frames, bool restart,
                 const std::vector<wcpt_primary_hit>& rec, const wcpt_scene_data& sd, const wcpt_temporal_params& p)
{
    const size_t n = (size_t)w * h;
    const std::vector<float> before = img;
    std::vector<float> out(n * 4, -7.0f), length(n, -7.0f);
    std::vector<float> base = s.base, n_b = s.n_b;
    if (restart || !s.valid) {
        base.assign(n * 3, -7.0f);
        n_b.assign(n, -7.0f);
        CHECK(wcpt_temporal_host(img.data(), frames, 1, rec.data(), &sd, w, h, &p, s.valid ? s.rgba.data() : nullptr,
                                 s.valid ? s.length.data() : nullptr, s.valid ? s.rec.data() : nullptr, s.valid ? &s.sd : nullptr,
                                 base.data(), n_b.data(), out.data(), length.data()) == WCPT_SUCCESS);
        s.rec = rec;
        s.sd = sd;
    } else {
        CHECK(wcpt_temporal_host(img.data(), frames, 0, rec.data(), &sd, w, h, &p, nullptr, nullptr, nullptr, nullptr,
                                 base.data(), n_b.data(), out.data(), length.data()) == WCPT_SUCCESS);
        CHECK(base == s.base || std::memcmp(base.data(), s.base.data(), n * 12) == 0);
    }
    CHECK(std::memcmp(img.data(), before.data(), n * 16) == 0);
    for (size_t i = 0; i < n; i++) {
        CHECK(n_b[i] >= 0.0f && length[i] >= 1.0f && length[i] <= (float)p.max_history);
        CHECK(std::memcmp(&out[4 * i + 3], &img[4 * i + 3], 4) == 0);
        CHECK(std::isfinite(base[3 * i]) && std::isfinite(base[3 * i + 1]) && std::isfinite(base[3 * i + 2]));
        if (n_b[i] == 0.0f) CHECK(std::memcmp(&out[4 * i], &img[4 * i], 12) == 0);
    }
    s.rgba = out;
    s.length = length;
    s.base = base;
    s.n_b = n_b;
    s.valid = true;
}

static void frame(uint32_t w, uint32_t h, std::mt19937& rng)
{
    const wcpt_temporal_params params[] = {{32, 0.9f, 0.05f, 0}, {1, -1.0f, 1.0e30f, 0}, {65536, 1.0f, 1.0e-6f, 0}};
    for (const wcpt_temporal_params& p : params) {
        State s;
        const wcpt_scene_data still = scene_of(0.0f, 0.0f, 0.0f, 0.0f, w, h);
        const std::vector<wcpt_primary_hit> rec0 = records(w, h, rng, false);
        call(s, w, h, noise(w, h, rng, false), 1, true, rec0, still, p);
        call(s, w, h, noise(w, h, rng, false), 2, false, rec0, still, p);
        call(s, w, h, noise(w, h, rng, true), 3, false, rec0, still, p);
        call(s, w, h, noise(w, h, rng, false), 1, true, rec0, still, p); /* the camera unmoved */
        size_t found = 0;
        for (float v : s.n_b) found += v > 0.0f;
        CHECK(found > 0 || w * h < 4);
        call(s, w, h, noise(w, h, rng, true), 1, true, records(w, h, rng, false), scene_of(0.0f, 0.0f, 0.0f, 1.5f, w, h), p);
        call(s, w, h, noise(w, h, rng, false), 1, true, records(w, h, rng, false), scene_of(0.3f, -0.2f, 0.1f, 1.5f, w, h), p);
        call(s, w, h, noise(w, h, rng, false), 1, true, records(w, h, rng, false, -1.0f), scene_of(0.3f, -0.2f, 0.1f, 181.5f, w, h), p);
        for (float v : s.n_b) CHECK(v == 0.0f); /* a half-turn: nothing of the old frame is in front */
        /* points anywhere: out of the frame on every side, behind the camera, not finite */
        for (int i = 0; i < 4; i++)
            call(s, w, h, noise(w, h, rng, i == 1), 1, true, records(w, h, rng, true),
                 scene_of(10.0f * (float)i, -3.0f, 1.0e3f * (float)(i & 1), 77.0f * (float)i, w, h), p);
        call(s, w, h, noise(w, h, rng, false), 1, true, rec0, still, p);
    }
}

/* the header alone: the packing of each kind, the camera, the blend */
static void header()
{
    wcpt_primary_hit q;
    std::memset(&q, 0, sizeof(q));
    q.direction[0] = 1.0f;
    q.t = 2.0f;
    q.normal[0] = -1.0f;
    q.index = 7;
    q.draw = 9;
    const float o[3] = {0.5f, 0.25f, -1.0f};
    uint32_t rec[WCPT_TEMPORAL_RECORD_WORDS], r0[4], r1[4];
    const uint32_t kinds[] = {WCPT_HIT_MISS, WCPT_HIT_SPHERE, WCPT_HIT_TRIANGLE | WCPT_HIT_FRONT, 3u};
    const uint32_t want_kind[] = {0u, 1u, 2u, 0u}, want_key[] = {0u, 7u, 9u, 0u};
    for (int i = 0; i < 4; i++) {
        q.kind = kinds[i];
        std::memcpy(rec, &q, sizeof(rec));
        wcpt_temporal_pack(rec, o, r0, r1);
        CHECK(r1[3] == want_kind[i] && r0[3] == want_key[i]);
        if (want_kind[i])
            CHECK(wcpt_u2f(r0[0]) == 2.5f && wcpt_u2f(r0[1]) == 0.25f && wcpt_u2f(r0[2]) == -1.0f && wcpt_u2f(r1[0]) == -1.0f);
        else
            CHECK(r0[0] == 0 && r0[1] == 0 && r0[2] == 0 && r1[0] == 0 && r1[1] == 0 && r1[2] == 0);
    }
    q.kind = WCPT_HIT_SPHERE;
    q.t = NAN; /* a NaN distance is a miss */
    std::memcpy(rec, &q, sizeof(rec));
    wcpt_temporal_pack(rec, o, r0, r1);
    CHECK(r1[3] == 0u && r0[3] == 0u);
    CHECK(wcpt_temporal_params_ok(1, -1.0f, 1.0e-30f) && wcpt_temporal_params_ok(65536, 1.0f, 1.0e30f));
    CHECK(!wcpt_temporal_params_ok(0, 0.9f, 0.05f) && !wcpt_temporal_params_ok(65537, 0.9f, 0.05f));
    CHECK(!wcpt_temporal_params_ok(32, NAN, 0.05f) && !wcpt_temporal_params_ok(32, 1.5f, 0.05f));
    CHECK(!wcpt_temporal_params_ok(32, 0.9f, 0.0f) && !wcpt_temporal_params_ok(32, 0.9f, INFINITY) &&
          !wcpt_temporal_params_ok(32, 0.9f, NAN));
    const wcpt_temporal_consts k = wcpt_temporal_make_consts(4, 0.9f, 0.05f);
    const float cur[4] = {1.0f, 2.0f, 3.0f, 0.5f}, base[3] = {3.0f, 2.0f, 1.0f};
    float out[4], len;
    wcpt_temporal_blend(cur, base, 0.0f, 1.0f, k, out, &len);
    CHECK(std::memcmp(out, cur, 16) == 0 && len == 1.0f);
    wcpt_temporal_blend(cur, base, 3.0f, 1.0f, k, out, &len);
    CHECK(out[0] == 2.5f && out[1] == 2.0f && out[2] == 1.5f && out[3] == 0.5f && len == 4.0f);
    wcpt_temporal_blend(cur, base, 7.0f, 1.0f, k, out, &len);
    CHECK(len == 4.0f);
    /* cameras: a singular matrix, one with a NaN and an orthographic projection are refused */
    wcpt_scene_data sd = scene_of(1.0f, 2.0f, 3.0f, 30.0f, 37, 23);
    wcpt_temporal_camera cam;
    CHECK(wcpt_temporal_make_camera(sd.inverseProjection, sd.inverseView, sd.position, 37, 23, &cam));
    CHECK(cam.position[0] == 1.0f && cam.position[2] == 3.0f);
    wcpt_scene_data bad = sd;
    std::memcpy(&bad.inverseView[4], &bad.inverseView[0], 16);
    CHECK(!wcpt_temporal_make_camera(bad.inverseProjection, bad.inverseView, bad.position, 37, 23, &cam));
    bad = sd;
    std::memset(bad.inverseProjection, 0, sizeof(bad.inverseProjection));
    CHECK(!wcpt_temporal_make_camera(bad.inverseProjection, bad.inverseView, bad.position, 37, 23, &cam));
    bad = sd;
    bad.inverseProjection[5] = NAN;
    CHECK(!wcpt_temporal_make_camera(bad.inverseProjection, bad.inverseView, bad.position, 37, 23, &cam));
    bad = sd;
    std::memset(bad.inverseProjection, 0, sizeof(bad.inverseProjection));
    bad.inverseProjection[0] = 2.0f; /* orthographic: a diagonal inverse */
    bad.inverseProjection[5] = 2.0f;
    bad.inverseProjection[10] = -100.0f;
    bad.inverseProjection[15] = 1.0f;
    CHECK(!wcpt_temporal_make_camera(bad.inverseProjection, bad.inverseView, bad.position, 37, 23, &cam));
    CHECK(!wcpt_temporal_make_camera(sd.inverseProjection, sd.inverseView, sd.position, 0, 23, &cam));
}

int main()
{
    std::mt19937 rng(11);
    frame(1, 1, rng);
    frame(3, 2, rng);
    frame(37, 23, rng);
    frame(5, 40, rng);
    header();
    /* refusals write nothing */
    std::vector<float> img(4, 1.0f), out(4, -7.0f), base(3, -7.0f), n_b(1, -7.0f), length(1, -7.0f);
    wcpt_primary_hit rec;
    std::memset(&rec, 0, sizeof(rec));
    const wcpt_scene_data sd = scene_of(0.0f, 0.0f, 0.0f, 0.0f, 1, 1);
    wcpt_scene_data flat = sd;
    std::memset(flat.inverseView, 0, sizeof(flat.inverseView));
    const wcpt_temporal_params good = {32, 0.9f, 0.05f, 0}, bad = {0, 0.9f, 0.05f, 0};
    const int refused = WCPT_ERROR_INVALID_ARGUMENT;
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &sd, 1, 1, &bad, nullptr, nullptr, nullptr, nullptr, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &sd, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(wcpt_temporal_host(img.data(), 0, 1, &rec, &sd, 1, 1, &good, nullptr, nullptr, nullptr, nullptr, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &flat, 1, 1, &good, nullptr, nullptr, nullptr, nullptr, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &sd, 1, 1, &good, img.data(), length.data(), &rec, &flat, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &sd, 1, 1, &good, img.data(), nullptr, &rec, &sd, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &sd, 0, 1, &good, nullptr, nullptr, nullptr, nullptr, base.data(),
                             n_b.data(), out.data(), length.data()) == refused);
    CHECK(out[0] == -7.0f && out[3] == -7.0f && base[0] == -7.0f && n_b[0] == -7.0f && length[0] == -7.0f);
    CHECK(wcpt_temporal_host(img.data(), 1, 1, &rec, &sd, 1, 1, &good, nullptr, nullptr, nullptr, nullptr, base.data(),
                             n_b.data(), out.data(), length.data()) == WCPT_SUCCESS);
    CHECK(out[0] == 1.0f && n_b[0] == 0.0f && length[0] == 1.0f);
    std::printf("%d failed checks\n", failures);
    return failures ? 1 : 0;
}
