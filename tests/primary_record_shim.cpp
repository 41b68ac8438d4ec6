// Test shim (CPU): exposes the primary cache's entry format (wc-path-tracer_amd/csrc/primary_record.h, what the megakernel
// stores and loads and what launch_megakernel allocates) to tests/test_primary_record.py over ctypes. Built by the test
// with g++; no HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/primary_record.h"

// in: {dir.xyz, normal.xyz, t, material, front} as bits
extern "C" void prec_pack(const uint32_t* in, uint32_t* words)
{
    wcpt::PrimaryRecord r;
    for (int i = 0; i < 3; i++) {
        r.dir[i] = in[i];
        r.normal[i] = in[3 + i];
    }
    r.t = in[6];
    r.material = in[7];
    r.front = in[8] != 0u;
    r.hit = r.t != wcpt::kPrimRecMissBits;
    wcpt::primary_record_pack(r, words);
}

// out: {dir.xyz, normal.xyz, t, material, front, hit}
extern "C" void prec_unpack(const uint32_t* words, uint32_t* out)
{
    const wcpt::PrimaryRecord r = wcpt::primary_record_unpack(words);
    for (int i = 0; i < 3; i++) {
        out[i] = r.dir[i];
        out[3 + i] = r.normal[i];
    }
    out[6] = r.t;
    out[7] = r.material;
    out[8] = r.front ? 1u : 0u;
    out[9] = r.hit ? 1u : 0u;
}

extern "C" uint32_t prec_words(void) { return wcpt::kPrimRecWords; }
extern "C" uint32_t prec_miss_bits(void) { return wcpt::kPrimRecMissBits; }
extern "C" uint64_t prec_bytes(uint64_t tiles) { return wcpt::primary_record_bytes(tiles); }
extern "C" uint64_t prec_word(uint64_t tile, uint32_t lane) { return wcpt::primary_record_word(tile, lane); }
