/* screen_layout.h — which rows of the frame a context holds, and every way that changes, as functions of plain values.
 * Plain C++17, no HIP type: the runtime (wcpt_screen.hip), the group (wcpt_group.hip) and tests/screen_layout_shim.cpp
 * (g++) evaluate the same functions.
 *
 * A layout is the frame's size and the context's `rows` local rows of it: the whole frame (not sharded, y0 0, rows ==
 * height), a contiguous block [y0, y0 + rows) (stripe 0), or interleaved stripes of `stripe` rows every `period` rows,
 * the first at frame row y0, the last possibly short (row_map.h). height == 0: no screen yet; a block or stripes named
 * then are held unchecked until the first screen applies the resize rule to them.
 *
 * Each transition takes the old layout and the call's arguments and gives the new layout or a refusal; the runtime
 * words the refusal and does the device's part (sync, image, zeroing).
 */
#ifndef WCPT_SCREEN_LAYOUT_H
#define WCPT_SCREEN_LAYOUT_H

#include <stdint.h>

#include "row_map.h"

namespace wcpt {

struct ScreenLayout {
    uint32_t width = 0, height = 0, y0 = 0, rows = 0; /* rows == height when not sharded */
    uint32_t stripe = 0, period = 0;                 /* 0: a contiguous block [y0, y0 + rows) */
    bool sharded = false;
};

enum LayoutRefusal {
    kLayoutOk = 0,
    kLayoutNoRows,      /* a zero width, height or row count where the call needs one */
    kLayoutBadStripes,  /* stripe no power of two in 1..32768, or period < stripe */
    kLayoutPastFrame,   /* the last row lies at or past the frame's height */
    kLayoutPastRow32,   /* the last row does not fit 32 bits */
};

constexpr uint32_t kMaxStripeRows = 32768;

inline bool stripe_pow2(uint32_t stripe) { return (stripe & (stripe - 1u)) == 0; }
/* stripes a context can hold (stripe != 0) */
inline bool stripes_ok(uint32_t stripe, uint32_t period)
{
    return stripe_pow2(stripe) && stripe <= kMaxStripeRows && period >= stripe;
}

/* The layout's row map (row_map.h): frame row of each local row. */
inline RowMap layout_row_map(const ScreenLayout& l)
{
    if (!l.stripe) return {l.y0, kContiguousShift, 0u};
    return {l.y0, (uint32_t)__builtin_ctz(l.stripe), l.period - l.stripe};
}

/* The frame row of the layout's last local row (its rows must be > 0), in 64 bits. */
inline uint64_t layout_last_row(const ScreenLayout& l) { return frame_row64(layout_row_map(l), l.rows - 1u); }

/* What a render can address (include/wcpt.h, "Frame sizes"). The frame may be any width x height of 32 bits: a pixel's
 * seed takes x + y * width in 32-bit arithmetic, wrapping as the reference's uint does. The context's own rows are
 * rendered in 8x8 tiles of 64 lanes, and tiles, lanes, path slots and queue entries are counted in 32 bits: its rows
 * may cover at most kMaxTiles tiles, 2^32 - 64 lanes (the wavefront's grid-stride loops add up to 64 to an index before
 * they compare it), that is an image of just under 64 GiB. At most 2^29 x 2^29 tiles: the product fits 64 bits. */
constexpr uint64_t kMaxTiles = 0x3FFFFFFull;
inline uint64_t layout_tiles(const ScreenLayout& l)
{
    return (((uint64_t)l.width + 7u) / 8u) * (((uint64_t)l.rows + 7u) / 8u);
}
inline bool layout_renderable(const ScreenLayout& l) { return layout_tiles(l) <= kMaxTiles; }

/* `old` holding `rows` rows from frame row y0, in stripes or (stripe 0) as one block */
inline ScreenLayout layout_with_rows(ScreenLayout old, uint32_t y0, uint32_t rows, uint32_t stripe, uint32_t period)
{
    old.sharded = true;
    old.y0 = y0;
    old.rows = rows;
    old.stripe = stripe;
    old.period = stripe ? period : 0u;
    return old;
}

/* wcpt_set_row_range: the block [y0, y0 + rows) of the frame; rows == 0 returns to the whole frame (with no screen
 * there is none to return to: y0 / rows stay). */
inline LayoutRefusal layout_set_range(const ScreenLayout& old, uint32_t y0, uint32_t rows, ScreenLayout& next)
{
    if (rows == 0) {
        next = old;
        next.sharded = false;
        next.stripe = next.period = 0;
        if (old.height) next.y0 = 0, next.rows = old.height;
        return kLayoutOk;
    }
    next = layout_with_rows(old, y0, rows, 0, 0);
    return old.height && layout_last_row(next) >= old.height ? kLayoutPastFrame : kLayoutOk;
}

/* wcpt_set_row_stripes with stripe != 0 (stripe == 0 is layout_set_range). When it answers kLayoutPastFrame, `next`
 * is the refused layout (for the message's last row). */
inline LayoutRefusal layout_set_stripes(const ScreenLayout& old, uint32_t y_first, uint32_t rows, uint32_t stripe,
                                        uint32_t period, ScreenLayout& next)
{
    if (rows == 0) return kLayoutNoRows;
    if (!stripes_ok(stripe, period)) return kLayoutBadStripes;
    next = layout_with_rows(old, y_first, rows, stripe, period);
    const uint64_t last = layout_last_row(next);
    if (old.height && last >= old.height) return kLayoutPastFrame;
    return last > 0xFFFFFFFFull ? kLayoutPastRow32 : kLayoutOk;
}

/* wcpt_create_screen / wcpt_resize: stripes are kept while their last row lies in the new frame, a block is clipped to
 * the new height, and what the new frame cannot hold falls back to the whole frame. */
inline LayoutRefusal layout_resize(const ScreenLayout& old, uint32_t width, uint32_t height, ScreenLayout& next)
{
    if (width == 0 || height == 0) return kLayoutNoRows;
    next = old;
    next.width = width;
    next.height = height;
    if (old.sharded && old.stripe) {
        if (old.rows && layout_last_row(old) < height) return kLayoutOk;
    } else if (old.sharded && old.y0 < height) {
        if ((uint64_t)old.y0 + old.rows > height) next.rows = height - old.y0;
        return kLayoutOk;
    }
    next.sharded = false;
    next.stripe = next.period = 0;
    next.y0 = 0;
    next.rows = height;
    return kLayoutOk;
}

/* The group's create-screen of one rank (wcpt::set_frame_block): frame size and the rank's rows in one step. The
 * context counts as sharded even when the block is the whole frame. */
inline LayoutRefusal layout_frame_block(const ScreenLayout& old, uint32_t width, uint32_t height, uint32_t y0, uint32_t rows,
                                        uint32_t stripe, uint32_t period, ScreenLayout& next)
{
    if (stripe && !stripes_ok(stripe, period)) return kLayoutBadStripes;
    if (width == 0 || rows == 0) return kLayoutNoRows;
    next = layout_with_rows(old, y0, rows, stripe, period);
    next.width = width;
    next.height = height;
    return layout_last_row(next) >= height ? kLayoutPastFrame : kLayoutOk;
}

/* ---- the formats a frame's rows are presented in (wcpt.h WCPT_PAYLOAD_*: the gather output, the group's frame) ------- */

enum PayloadFormat : uint32_t { kPayloadRgb32f = 3, kPayloadRgba32f = 4, kPayloadDisplayRgba8 = 8 };

inline bool payload_format_valid(uint32_t f) { return f == kPayloadRgb32f || f == kPayloadRgba32f || f == kPayloadDisplayRgba8; }
/* bytes per pixel: 3 or 4 floats, or 4 bytes; format 0 (no output) holds none */
inline uint64_t payload_pixel_bytes(uint32_t format) { return format == kPayloadDisplayRgba8 ? 4u : 4ull * format; }

/* ---- a frame's rows split among n ranks (wcpt_row_block, wcpt_row_stripes; n > 0, rank < n) ------------------------- */

/* rank r of n holds rows [r * height / n, (r + 1) * height / n): blocks differ by at most one row */
inline void split_row_block(uint32_t height, uint32_t n, uint32_t rank, uint32_t& y0, uint32_t& rows)
{
    const uint32_t a = (uint32_t)((uint64_t)rank * height / n);
    const uint32_t b = (uint32_t)((uint64_t)(rank + 1) * height / n);
    y0 = a;
    rows = b - a;
}

/* rank r of n holds the stripes r, r + n, ... below T = ceil(height / stripe) (stripe a power of two); only the frame's
 * last stripe can be short */
inline void split_row_stripes(uint32_t height, uint32_t n, uint32_t rank, uint32_t stripe, uint32_t& y_first, uint32_t& rows)
{
    const uint64_t T = ((uint64_t)height + stripe - 1u) / stripe;
    const uint64_t count = T > rank ? (T - 1u - rank) / n + 1u : 0u;
    uint64_t r = count * stripe;
    if (count && (T - 1u - rank) % n == 0 && height % stripe) r -= stripe - height % stripe; /* it holds the short one */
    y_first = rank * stripe;
    rows = (uint32_t)r;
}

} // namespace wcpt

#endif
