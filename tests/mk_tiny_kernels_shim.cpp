// CPU test program for tests/test_mk_tiny_kernels.py: the condition under which a megakernel render takes the walk-only
// head and tail (wc-path-tracer_amd/csrc/mk_tiny_rule.h mk_tiny_kernels, the function pt_kernels.hip launch_megakernel
// calls), printed over its whole truth table: one line "mode tiny_tree split pairs single arith -> 0|1" per combination.
// Stand-alone (its own main), so it runs under AddressSanitizer and UndefinedBehaviorSanitizer as it is.
#include <cstdio>

#include "../include/wcpt.h"
#include "../wc-path-tracer_amd/csrc/mk_tiny_rule.h"

int main()
{
    const int modes[] = {wcpt::kModeRender, wcpt::kModeCount, wcpt::kModeDiag};
    const int ariths[] = {WCPT_ARITH_EXACT, WCPT_ARITH_FAST};
    int lines = 0;
    for (int mode : modes)
        for (int tiny = 0; tiny < 2; tiny++)
            for (int split = 0; split < 2; split++)
                for (int pairs = 0; pairs < 2; pairs++)
                    for (int single = 0; single < 2; single++)
                        for (int arith : ariths) {
                            const bool k = wcpt::mk_tiny_kernels(mode, tiny != 0, split != 0, pairs != 0, single != 0, arith);
                            std::printf("%d %d %d %d %d %d -> %d\n", mode, tiny, split, pairs, single, arith, k ? 1 : 0);
                            lines++;
                        }
    /* the selection the launch feeds it: a split exists only where mk_variant_select returns two instances */
    const wcpt::MkSelection s = wcpt::mk_variant_select(wcpt::kModeRender, 1, true, 1u, 1u, wcpt::kPrimaryCacheRead,
                                                        WCPT_ARITH_EXACT, true);
    std::printf("select %u %d %d %d\n", s.n, s.v[0].pairs ? 1 : 0, s.v[0].single ? 1 : 0, s.v[0].arith);
    std::printf("%d lines\n", lines);
    return 0;
}
