// Test shim (CPU): exposes the primary-hit record (wc-path-tracer_amd/csrc/primary_hit.h: what pt_primary.hip stores and
// wcpt_trace_primary / wcpt_pick hand out), the ABI's struct of it (include/wcpt.h wcpt_primary_hit) and the row map a
// pass takes from the screen's layout (screen_layout.h) to tests/test_primary_hit.py over ctypes. Built by the test with
// g++; no HIP involved.
#include <cstddef>
#include <cstdint>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/primary_hit.h"
#include "../wc-path-tracer_amd/csrc/screen_layout.h"

// in: {dir.xyz, t, normal.xyz, front, material, prim, draw} as bits; the record of the traversal's winner, packed
extern "C" void phit_pack_of(const uint32_t* in, uint32_t* words)
{
    wcpt::primary_hit_pack(wcpt::primary_hit_of(in, in[3], in + 4, in[7] != 0u, in[8], in[9], in[10]), words);
}

// in: {dir.xyz, t, normal.xyz, kind, front, material, index, draw}
extern "C" void phit_pack(const uint32_t* in, uint32_t* words)
{
    wcpt::PrimaryHit r;
    for (int i = 0; i < 3; i++) {
        r.dir[i] = in[i];
        r.normal[i] = in[4 + i];
    }
    r.t = in[3];
    r.kind = in[7];
    r.front = in[8] != 0u;
    r.material = in[9];
    r.index = in[10];
    r.draw = in[11];
    wcpt::primary_hit_pack(r, words);
}

// out: {dir.xyz, t, normal.xyz, kind, front, material, index, draw}
extern "C" void phit_unpack(const uint32_t* words, uint32_t* out)
{
    const wcpt::PrimaryHit r = wcpt::primary_hit_unpack(words);
    for (int i = 0; i < 3; i++) {
        out[i] = r.dir[i];
        out[4 + i] = r.normal[i];
    }
    out[3] = r.t;
    out[7] = r.kind;
    out[8] = r.front ? 1u : 0u;
    out[9] = r.material;
    out[10] = r.index;
    out[11] = r.draw;
}

// the constants: {words, bytes, miss t bits, miss, sphere, triangle, kind mask, front bit, no prim, sphere prim}
extern "C" void phit_constants(uint32_t* out)
{
    const uint32_t v[10] = {wcpt::kPrimHitWords, wcpt::kPrimHitBytes, wcpt::kPrimHitMissT, wcpt::kPrimHitMiss,
                            wcpt::kPrimHitSphere, wcpt::kPrimHitTriangle, wcpt::kPrimHitKindMask, wcpt::kPrimHitFrontBit,
                            wcpt::kPrimHitNoPrim, wcpt::kPrimHitSpherePrim};
    for (int i = 0; i < 10; i++) out[i] = v[i];
}

// the header's struct: {sizeof, offsetof direction, t, normal, kind, material, index, draw, _pad}, then the ABI's macros
// {WCPT_HIT_MISS, _SPHERE, _TRIANGLE, _KIND_MASK, _FRONT}
extern "C" void phit_struct(uint32_t* out)
{
    const uint32_t v[14] = {(uint32_t)sizeof(wcpt_primary_hit),
                            (uint32_t)offsetof(wcpt_primary_hit, direction),
                            (uint32_t)offsetof(wcpt_primary_hit, t),
                            (uint32_t)offsetof(wcpt_primary_hit, normal),
                            (uint32_t)offsetof(wcpt_primary_hit, kind),
                            (uint32_t)offsetof(wcpt_primary_hit, material),
                            (uint32_t)offsetof(wcpt_primary_hit, index),
                            (uint32_t)offsetof(wcpt_primary_hit, draw),
                            (uint32_t)offsetof(wcpt_primary_hit, _pad),
                            WCPT_HIT_MISS, WCPT_HIT_SPHERE, WCPT_HIT_TRIANGLE, WCPT_HIT_KIND_MASK, WCPT_HIT_FRONT};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}

extern "C" uint64_t phit_offset(uint64_t ly, uint64_t x, uint64_t width) { return wcpt::primary_hit_offset(ly, x, width); }
extern "C" uint64_t phit_bytes(uint64_t width, uint64_t rows) { return wcpt::primary_hit_bytes(width, rows); }

// Where frame pixel (x, y) lies in the pass over a context that holds `rows` rows of a frame `width` wide from frame row
// y0 (stripe 0: a block; else stripes of `stripe` rows every `period`): the byte offset of its record, or ~0 when the
// context does not hold the row. The rows are walked through the layout's row map, as the kernel does.
extern "C" uint64_t phit_offset_of_frame_pixel(uint32_t width, uint32_t y0, uint32_t rows, uint32_t stripe, uint32_t period,
                                               uint32_t x, uint32_t y)
{
    wcpt::ScreenLayout l;
    l.width = width;
    l.y0 = y0;
    l.rows = rows;
    l.stripe = stripe;
    l.period = period;
    l.sharded = true;
    const wcpt::RowMap m = wcpt::layout_row_map(l);
    for (uint32_t ly = 0; ly < rows; ly++)
        if (wcpt::frame_row(m, ly) == y) return wcpt::primary_hit_offset(ly, x, width);
    return ~0ull;
}
