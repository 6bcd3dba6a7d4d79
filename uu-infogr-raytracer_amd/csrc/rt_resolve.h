// rt_resolve.h -- per-lane arithmetic of the supersampling resolve (rt_set_supersampling), shared by
// the trace kernels' epilogue (rt_kernel.hip resolve_tile) and host code (tests/native/ss_host.cpp).
//
// An output pixel at factor k = 1 << s (s = 1, 2, 3) is, per 8-bit channel, the round-half-up mean of
// its k x k samples after ShiftColor: (sum + k*k/2) >> 2s.  A sample 0x00RRGGBB is unpacked into two
// words of 16-bit fields -- {R, B} and {G} -- so that a channel's sum of up to 64 samples (64 * 255 =
// 16,320 < 2^14) never carries into its neighbour; sums of unpacked samples are plain 32-bit adds (the
// kernel's cross-lane steps), and the rounding works on both fields of a word at once.
//
// The camera-path shutter (rt_render_shutter_bands) averages m = 1 << t sub-frames of one pixel, m up to
// RT_MAX_SHUTTER = 256, with the same unpacked sums: a field then holds 256 * 255 + 128 = 65,408 < 2^16, rounding
// term included, so resolve_round_n needs no wider word.
#pragma once
#include <stdint.h>

#include "../../include/raytracer_hip.h"

#if defined(__HIPCC__)
#define RT_RESOLVE_FN __host__ __device__ inline
#else
#define RT_RESOLVE_FN inline
#endif

namespace rtk {

struct ResolveSum {
    uint32_t rb;  // R sum in bits 16-31, B sum in bits 0-15
    uint32_t g;   // G sum in bits 0-15
};

RT_RESOLVE_FN ResolveSum resolve_unpack(uint32_t px) { return ResolveSum{px & 0x00ff00ffu, (px >> 8) & 0xffu}; }

RT_RESOLVE_FN ResolveSum resolve_add(ResolveSum a, ResolveSum b) { return ResolveSum{a.rb + b.rb, a.g + b.g}; }

// The sum of (1 << s)^2 unpacked samples -> the output pixel 0x00RRGGBB.
RT_RESOLVE_FN uint32_t resolve_round(ResolveSum sum, int s) {
    const int sh = 2 * s;
    const uint32_t half = (1u << sh) >> 1;  // k*k/2 (s = 0: 0, the sample itself)
    const uint32_t rb = ((sum.rb + (half | (half << 16))) >> sh) & 0x00ff00ffu;  // (R's low bits fall into B's field: masked)
    const uint32_t g = ((sum.g + half) >> sh) & 0xffu;
    return rb | (g << 8);
}

// The sum of 1 << t unpacked sub-frame pixels (t = 0 .. 8) -> the output pixel 0x00RRGGBB, the round-half-up mean
// per channel: (sum + m / 2) >> t.
static_assert(RT_MAX_SHUTTER * 255 + RT_MAX_SHUTTER / 2 < 65536, "a channel's shutter sum and its rounding term fit a 16-bit field");
RT_RESOLVE_FN uint32_t resolve_round_n(ResolveSum sum, int t) {
    const uint32_t half = (1u << t) >> 1;  // m / 2 (t = 0: 0, the pixel itself)
    const uint32_t rb = ((sum.rb + (half | (half << 16))) >> t) & 0x00ff00ffu;  // (R's low bits fall into B's field: masked)
    const uint32_t g = ((sum.g + half) >> t) & 0xffu;
    return rb | (g << 8);
}

// Progressive accumulation (rt_set_progressive): the sum of c unpacked samples, c = 1 .. 64 -> the output pixel
// 0x00RRGGBB, per channel (sum + c / 2) / c in integers (c / 2 floors).  No divide per field: with M = 2^21 / c + 1
// and e = M c - 2^21 in 1..c, (n M) >> 21 = n / c for every n with n e < 2^21, and a field's n = sum + c / 2 is at
// most 255 c + c / 2, so n e <= 255.5 c^2 < 2^20; n M < 256 * 2^21 + 2^14 stays inside 32 bits.  Integer operations
// only, so the host's exhaustive check (tests/native/progressive_host.cpp) is the device's.  For c a power of two
// it is resolve_round_n.
constexpr int RESOLVE_DIV_MAX = 64;
RT_RESOLVE_FN uint32_t resolve_round_div(ResolveSum sum, int c) {
    const uint32_t m = (1u << 21) / (uint32_t)c + 1u, half = (uint32_t)c >> 1;
    const uint32_t r = (((sum.rb >> 16) + half) * m) >> 21, b = (((sum.rb & 0xffffu) + half) * m) >> 21;
    const uint32_t g = (((sum.g & 0xffffu) + half) * m) >> 21;
    return (r << 16) | (g << 8) | b;
}

// Adaptive supersampling (rt_set_adaptive_sampling): do the pixels a and b (0x00RRGGBB) differ by at least thr,
// thr in 1..256, in some 8-bit channel?  Per word of 16-bit fields: with bit 8 of every field of a set, a - b
// borrows from no neighbour and the field holds 256 + (a_c - b_c) in 1..511; b - a likewise; the larger of the
// two is 256 + |a_c - b_c|, compared field by field with 256 + thr (thr = 256: never, a difference is <= 255).
RT_RESOLVE_FN bool adapt_field_ge(uint32_t a, uint32_t b, uint32_t lim) {  // two 16-bit fields of 8-bit values
    const uint32_t one = 0x01000100u, d = (a | one) - b, e = (b | one) - a;
    const uint32_t hi = (d >> 16) > (e >> 16) ? d >> 16 : e >> 16, lo = (d & 0xffffu) > (e & 0xffffu) ? d & 0xffffu : e & 0xffffu;
    return hi >= lim || lo >= lim;
}
RT_RESOLVE_FN bool adapt_differs(uint32_t a, uint32_t b, int thr) {
    const ResolveSum u = resolve_unpack(a), v = resolve_unpack(b);
    const uint32_t lim = 256u + (uint32_t)thr;
    return adapt_field_ge(u.rb, v.rb, lim) || adapt_field_ge(u.g, v.g, lim);
}

}  // namespace rtk
