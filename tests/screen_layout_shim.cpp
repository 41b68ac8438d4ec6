// Test shim (CPU): exposes the row layout's rules (wc-path-tracer_amd/csrc/screen_layout.h, what the runtime asks on
// wcpt_create_screen / wcpt_resize, wcpt_set_row_range, wcpt_set_row_stripes and the group's frame block, and the splits
// behind wcpt_row_block / wcpt_row_stripes) to tests/test_screen_layout.py over ctypes. Built by the test with g++; no
// HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/screen_layout.h"

using namespace wcpt;

namespace {

// a layout as 7 words: width, height, y0, rows, stripe, period, sharded
ScreenLayout unpack(const uint32_t* w)
{
    ScreenLayout l;
    l.width = w[0], l.height = w[1], l.y0 = w[2], l.rows = w[3], l.stripe = w[4], l.period = w[5], l.sharded = w[6] != 0;
    return l;
}

// 0 accepted (and the layout written), 1 no rows / zero size, 2 bad stripes, 3 past the frame, 4 past row 2^32
int answer(LayoutRefusal r, const ScreenLayout& l, uint32_t* w)
{
    switch (r) {
    case kLayoutOk:
        w[0] = l.width, w[1] = l.height, w[2] = l.y0, w[3] = l.rows, w[4] = l.stripe, w[5] = l.period, w[6] = l.sharded;
        return 0;
    case kLayoutNoRows: return 1;
    case kLayoutBadStripes: return 2;
    case kLayoutPastFrame: return 3;
    case kLayoutPastRow32: return 4;
    }
    return -1;
}

} // namespace

extern "C" int sl_range(const uint32_t* old, uint32_t y0, uint32_t rows, uint32_t* out)
{
    ScreenLayout next;
    return answer(layout_set_range(unpack(old), y0, rows, next), next, out);
}

extern "C" int sl_stripes(const uint32_t* old, uint32_t y_first, uint32_t rows, uint32_t stripe, uint32_t period, uint32_t* out)
{
    ScreenLayout next;
    return answer(layout_set_stripes(unpack(old), y_first, rows, stripe, period, next), next, out);
}

extern "C" int sl_resize(const uint32_t* old, uint32_t width, uint32_t height, uint32_t* out)
{
    ScreenLayout next;
    return answer(layout_resize(unpack(old), width, height, next), next, out);
}

extern "C" int sl_frame_block(const uint32_t* old, uint32_t width, uint32_t height, uint32_t y0, uint32_t rows, uint32_t stripe,
                              uint32_t period, uint32_t* out)
{
    ScreenLayout next;
    return answer(layout_frame_block(unpack(old), width, height, y0, rows, stripe, period, next), next, out);
}

extern "C" uint64_t sl_last_row(const uint32_t* l) { return layout_last_row(unpack(l)); }

// out: y0, shift, gap
extern "C" void sl_row_map(const uint32_t* l, uint32_t* out)
{
    const RowMap m = layout_row_map(unpack(l));
    out[0] = m.y0, out[1] = m.shift, out[2] = m.gap;
}

extern "C" uint32_t sl_frame_row(const uint32_t* l, uint32_t ly) { return frame_row(layout_row_map(unpack(l)), ly); }

// out: y_first, rows (n > 0, rank < n, stripe 0 or a power of two: what wcpt_row_block / wcpt_row_stripes have checked)
extern "C" void sl_split(uint32_t height, uint32_t n, uint32_t rank, uint32_t stripe, uint32_t* out)
{
    if (stripe) split_row_stripes(height, n, rank, stripe, out[0], out[1]);
    else split_row_block(height, n, rank, out[0], out[1]);
}

// the 8x8 tiles of the layout's rows, and whether a render can address them
extern "C" uint64_t sl_tiles(const uint32_t* l) { return layout_tiles(unpack(l)); }
extern "C" int sl_renderable(const uint32_t* l) { return layout_renderable(unpack(l)) ? 1 : 0; }

extern "C" int sl_stripe_pow2(uint32_t stripe) { return stripe_pow2(stripe) ? 1 : 0; }
