// Test shim (CPU): exposes the split-render rule and queue layout (wc-path-tracer_amd/csrc/mk_split_rule.h, what
// launch_megakernel applies) to tests/test_mk_split_rule.py over ctypes. Built by the test with g++; no HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/mk_split_rule.h"

extern "C" uint32_t mks_cut(int option, int splittable, uint32_t samples, uint32_t max_bounce, uint64_t waves,
                            uint64_t wave_slots, uint64_t triangles)
{
    return wcpt::mk_split_cut(option, splittable != 0, samples, max_bounce, waves, wave_slots, triangles);
}

// out: {cap[0], cap[1], first[0], first[1], entries}
extern "C" void mks_layout(uint32_t tiles, int piped, uint64_t* out)
{
    const wcpt::MkSplitLayout l = wcpt::mk_split_layout(tiles, piped != 0);
    out[0] = l.cap[0];
    out[1] = l.cap[1];
    out[2] = l.first[0];
    out[3] = l.first[1];
    out[4] = l.entries;
}

extern "C" uint32_t mks_sub_first(uint32_t blocks, uint32_t j) { return wcpt::mk_split_sub_first(blocks, j); }
extern "C" uint32_t mks_sub_cap(uint32_t blocks, uint32_t j) { return wcpt::mk_split_sub_cap(blocks, j); }
extern "C" int mks_sub_queues(void) { return (int)wcpt::kMkSplitSubQueues; }
extern "C" int mks_counter_words(void) { return (int)wcpt::kMkSplitCounterWords; }
extern "C" int mks_auto_cut(void) { return (int)wcpt::kMkSplitAutoCut; }
extern "C" int mks_entry_bytes(void) { return (int)wcpt::kMkSplitEntryBytes; }
extern "C" int mks_max_cut(void) { return wcpt::kMkSplitMaxCut; }
