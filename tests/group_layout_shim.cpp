// Test shim (CPU): exposes the product's group frame layout (wc-path-tracer_amd/csrc/group_layout.h, what wcpt_group.hip
// addresses a frame's renders, transfers and copies by) to tests/test_group_layout.py over ctypes. Built by the test
// with g++; no HIP involved.
#include <cstdint>

#include "../wc-path-tracer_amd/csrc/group_layout.h"

namespace gl = wcpt::glayout;

extern "C" {

uint64_t pixel_bytes(uint32_t format) { return wcpt::payload_pixel_bytes(format); }
int format_valid(uint32_t format) { return wcpt::payload_format_valid(format) ? 1 : 0; }

int screen_refusal(int nranks, uint32_t stripe, uint32_t width, uint32_t height)
{
    return (int)gl::screen_refusal(nranks, stripe, width, height);
}

int output_refusal(uint32_t width, uint32_t height, uint32_t format, uint64_t dst, uint64_t bytes)
{
    return (int)gl::output_refusal(width, height, format, dst, bytes);
}

// head: frame_bytes, stage_bytes. out, 15 values per rank: y0, rows, bytes, frame_off, writes_frame, whole_frame,
// stage_off, then the stripe copy: dst_off, dst_pitch, src_pitch, span, count, tail_dst_off, tail_src_off, tail_bytes.
void lay_out(int nranks, int root, int transport, uint32_t stripe, uint32_t width, uint32_t height, uint32_t format,
             uint64_t* head, uint64_t* out)
{
    gl::Layout l;
    gl::lay_out({nranks, root, transport, stripe, width, height, format}, l);
    head[0] = l.frame_bytes;
    head[1] = l.stage_bytes;
    for (const gl::RankLayout& k : l.rank) {
        const uint64_t v[15] = {k.y0, k.rows, k.bytes, k.frame_off, k.writes_frame, k.whole_frame, k.stage_off,
                                k.copy.dst_off, k.copy.dst_pitch, k.copy.src_pitch, k.copy.span, k.copy.count,
                                k.copy.tail_dst_off, k.copy.tail_src_off, k.copy.tail_bytes};
        for (uint64_t x : v) *out++ = x;
    }
}

double timeout_ms(int option, int nranks) { return gl::timeout_ms(option, nranks); }
double drain_ms(double timeout) { return gl::drain_ms(timeout); }
int issue_threads(int option, int local_ranks, int transport, int spans_devices)
{
    return gl::issue_threads(option, (size_t)local_ranks, transport, spans_devices != 0) ? 1 : 0;
}

}
