/* mk_variant.h — the megakernel's instances as values: what an instance is specialised on (MkVariant), which
 * combinations are compiled (mk_variant_built), and which of them a launch takes (mk_variant_select). Plain C++17, no
 * HIP: tests/mk_variant_shim.cpp compiles it with g++, and pt_kernels.hip turns a runtime MkVariant into the kernel's
 * template arguments (mk_dispatch), so this file is the list of instances.
 *
 * The instances (a device code object holds 136 pt_megakernel and 8 pt_mk_tail):
 *   96 render   whole launches: stack 2 x pairs 2 x single draw 2 x arithmetic 2 x (sample reuse, primary cache) 6
 *   24 head     the first launch of a split render: LDS stack and one sample only, so pairs 2 x single draw 2 x
 *               arithmetic 2 x primary cache 3
 *   16 count    the counting and the diagnostics build: stack 2 x pairs 2 x single draw 2 x diag 2; exact arithmetic,
 *               never cached, never split (their counters are the reference's)
 *    8 tail     the second launch of a split render (pt_mk_tail): pairs 2 x single draw 2 x arithmetic 2; no primary
 *               segment, so no cache and no reuse */
#ifndef WCPT_MK_VARIANT_H
#define WCPT_MK_VARIANT_H

#include <stdint.h>

#include "primary_cache_key.h"

namespace wcpt {

/* Launch modes: render the frame; count the reference algorithm's work (no image write); count + SIMD
 * diagnostics (ballot-based step counters, tools/diag.py). */
constexpr int kModeRender = 0, kModeCount = 1, kModeDiag = 2;

/* whole: the one launch of an unsplit render; head / tail: the two launches of a split one (mk_split_rule.h) */
constexpr int kMkStageWhole = 0, kMkStageHead = 1, kMkStageTail = 2;

/* The nine values an instance is specialised on, in the order of pt_megakernel's template parameters. */
struct MkVariant {
    bool count;  /* counts the reference's work instead of rendering */
    bool diag;   /* ... and the SIMD lane / wave steps */
    int stack;   /* 0: private (scratch) stack, 1: LDS stack with a private spill */
    bool pairs;  /* leaf tests on pair records */
    bool single; /* one draw command: no draw loop */
    bool reuse;  /* samples > 1: later samples resolve their primary segment from sample 0's record */
    int pcache;  /* kPrimaryCacheNone / Write / Read */
    int arith;   /* WCPT_ARITH_EXACT / WCPT_ARITH_FAST */
    int stage;   /* kMkStageWhole / Head / Tail */
};

/* Which combinations are compiled: the single statement of it (the dispatcher instantiates exactly these). */
constexpr bool mk_variant_built(const MkVariant& v)
{
    if (v.stack < 0 || v.stack > 1 || v.pcache < kPrimaryCacheNone || v.pcache > kPrimaryCacheRead ||
        v.arith < WCPT_ARITH_EXACT || v.arith > WCPT_ARITH_FAST || v.stage < kMkStageWhole || v.stage > kMkStageTail)
        return false;
    /* a tail finishes paths behind their primary segment, on the LDS stack like its head: pairs x single x arith */
    if (v.stage == kMkStageTail) return !v.count && !v.diag && v.stack == 1 && !v.reuse && v.pcache == kPrimaryCacheNone;
    /* counting builds are exact, never cached, never split and trace every sample's primary segment */
    if (v.count) return v.arith == WCPT_ARITH_EXACT && v.pcache == kPrimaryCacheNone && v.stage == kMkStageWhole && !v.reuse;
    if (v.diag) return false; /* the diagnostics are counters */
    /* a head is LDS-stack and one-sample only */
    if (v.stage == kMkStageHead) return v.stack == 1 && !v.reuse;
    return true;
}

/* Dense numbering of the field combinations, for enumerating them: mk_variant_decode(c) for c < kMkVariantCodes is
 * every combination once. */
constexpr uint32_t kMkVariantCodes = 2u * 2u * 2u * 2u * 2u * 2u * 3u * 2u * 3u;
constexpr MkVariant mk_variant_decode(uint32_t c)
{
    MkVariant v = {};
    v.count = c % 2u != 0u;    c /= 2u;
    v.diag = c % 2u != 0u;     c /= 2u;
    v.stack = (int)(c % 2u);   c /= 2u;
    v.pairs = c % 2u != 0u;    c /= 2u;
    v.single = c % 2u != 0u;   c /= 2u;
    v.reuse = c % 2u != 0u;    c /= 2u;
    v.pcache = (int)(c % 3u);  c /= 3u;
    v.arith = (int)(c % 2u);   c /= 2u;
    v.stage = (int)(c % 3u);
    return v;
}
/* of a combination whose fields are in range (every built one is) */
constexpr uint32_t mk_variant_code(const MkVariant& v)
{
    uint32_t c = (uint32_t)v.stage;
    c = c * 2u + (uint32_t)v.arith;
    c = c * 3u + (uint32_t)v.pcache;
    c = c * 2u + (v.reuse ? 1u : 0u);
    c = c * 2u + (v.single ? 1u : 0u);
    c = c * 2u + (v.pairs ? 1u : 0u);
    c = c * 2u + (uint32_t)v.stack;
    c = c * 2u + (v.diag ? 1u : 0u);
    c = c * 2u + (v.count ? 1u : 0u);
    return c;
}

/* What one launch_megakernel call launches per pipe: the whole kernel, or a head and then its tail. */
struct MkSelection {
    uint32_t n; /* 1: v[0] whole; 2: v[0] head, v[1] tail */
    MkVariant v[2];
};

/* The selection. mode: kModeRender / Count / Diag; stack_kind: the option (0 scratch, else LDS); pair_records:
 * LaunchArgs::pair_records; draws: drawCommandCount; samples: the scene's; pcmode: what primary_cache_decide returned;
 * arith: LaunchArgs::arith; split: mk_split_cut returned a cut. Every variant returned is built.
 *   - counting runs ignore the cache, the arithmetic and the split;
 *   - a split is taken only where a head exists (render, LDS stack, one sample: what mk_split_cut also demands);
 *   - the read form for one sample holds the sample count as a constant and is used only for samples == 1, every other
 *     sample count takes the reuse form; without a read, reuse is samples > 1;
 *   - a reuse-write build stores the cache entry from the caller (shade_pixel), after its sample loop, which the kernel
 *     derives from the pair. */
constexpr MkSelection mk_variant_select(int mode, int stack_kind, bool pair_records, uint32_t draws, uint32_t samples,
                                        int pcmode, int arith, bool split)
{
    MkVariant v = {};
    v.stack = stack_kind == 0 ? 0 : 1;
    v.pairs = pair_records;
    v.single = draws == 1u; /* the reference's case */
    v.pcache = kPrimaryCacheNone;
    v.arith = WCPT_ARITH_EXACT;
    v.stage = kMkStageWhole;
    MkSelection s = {1u, {v, v}};
    if (mode != kModeRender) {
        s.v[0].count = true;
        s.v[0].diag = mode != kModeCount;
        s.v[1] = s.v[0];
        return s;
    }
    v.arith = arith == WCPT_ARITH_FAST ? WCPT_ARITH_FAST : WCPT_ARITH_EXACT;
    if (split && v.stack == 1 && samples == 1u) {
        s.n = 2u;
        s.v[1] = v;
        s.v[1].stage = kMkStageTail;
        v.stage = kMkStageHead;
    }
    v.pcache = pcmode == kPrimaryCacheRead ? kPrimaryCacheRead
                                           : (pcmode == kPrimaryCacheWrite ? kPrimaryCacheWrite : kPrimaryCacheNone);
    if (s.n == 1u) v.reuse = v.pcache == kPrimaryCacheRead ? samples != 1u : samples > 1u;
    s.v[0] = v;
    if (s.n == 1u) s.v[1] = v;
    return s;
}

} // namespace wcpt

#endif
