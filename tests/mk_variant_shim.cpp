// Test shim (CPU): exposes the megakernel's variant list and selection (wc-path-tracer_amd/csrc/mk_variant.h, what
// launch_megakernel applies and pt_kernels.hip's dispatcher instantiates) to tests/test_mk_variant.py over ctypes.
// Built by the test with g++; no HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/mk_variant.h"

// a variant as nine ints: count, diag, stack, pairs, single, reuse, pcache, arith, stage
static void put(const wcpt::MkVariant& v, int* out)
{
    out[0] = v.count; out[1] = v.diag; out[2] = v.stack; out[3] = v.pairs; out[4] = v.single; out[5] = v.reuse;
    out[6] = v.pcache; out[7] = v.arith; out[8] = v.stage;
}
static wcpt::MkVariant get(const int* f)
{
    return wcpt::MkVariant{f[0] != 0, f[1] != 0, f[2], f[3] != 0, f[4] != 0, f[5] != 0, f[6], f[7], f[8]};
}

extern "C" uint32_t mkv_codes(void) { return wcpt::kMkVariantCodes; }
extern "C" void mkv_decode(uint32_t code, int* out) { put(wcpt::mk_variant_decode(code), out); }
extern "C" uint32_t mkv_code(const int* f) { return wcpt::mk_variant_code(get(f)); }
extern "C" int mkv_built(const int* f) { return wcpt::mk_variant_built(get(f)) ? 1 : 0; }

// out: 2 x 9 ints; returns the number of launches (1: whole, 2: head then tail)
extern "C" uint32_t mkv_select(int mode, int stack_kind, int pair_records, uint32_t draws, uint32_t samples, int pcmode,
                               int arith, int split, int* out)
{
    const wcpt::MkSelection s =
        wcpt::mk_variant_select(mode, stack_kind, pair_records != 0, draws, samples, pcmode, arith, split != 0);
    put(s.v[0], out);
    put(s.v[1], out + 9);
    return s.n;
}

// the same selection evaluated by the compiler: the functions are usable in constant expressions (the dispatcher's
// `if constexpr (mk_variant_built(...))` needs that)
static_assert(wcpt::mk_variant_select(wcpt::kModeRender, 1, true, 1, 1, wcpt::kPrimaryCacheRead, WCPT_ARITH_FAST, true).n == 2,
              "a split render is two launches");
static_assert(wcpt::mk_variant_built(wcpt::mk_variant_decode(0)), "the plain exact scratch-stack render");
