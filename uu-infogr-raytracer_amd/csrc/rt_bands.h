// rt_bands.h -- the row bands of a frame and the band plan of the Tick hand-off: which bands a worker traces, where
// they lie in its packed band set and in the frame, how a share splits into chunks, and the copies that hand them
// over.  Device-free index arithmetic: rt_api.cpp issues the traces and copies, tests/native/san_host.cpp checks that
// every plan writes every frame word once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/raytracer_hip.h"
#include "rt_internal.h"

namespace rtk {

inline int total_bands(int H, int band_rows) { return (H + band_rows - 1) / band_rows; }
inline int bands_of(int H, int band_rows, int first, int step) {
    int tb = total_bands(H, band_rows);
    return first < tb ? (tb - 1 - first) / step + 1 : 0;
}
// Bytes of one frame's output of a band render in `fmt`.
inline size_t band_output_bytes(int W, int H, int nb, int band_rows, int fmt) {
    return fmt == RT_BANDS_FRAME ? (size_t)W * H * 4 : (size_t)nb * band_rows * W * (fmt == RT_BANDS_RGB24 ? 3 : 4);
}

// The band pipeline of the Tick (the reference's only parallel loop is the row-parallel
// one of RayTracer.cs:898-901).  Worker g of n (a device; RT_CREATE_SHARED_DEVICE: a stream of one
// device) traces the interleaved 8-row bands b = g, g + n, ... of the frame (n == 1: the frame as one
// band) -- balanced however the scene's cost is spread over the rows (the top ~45 % of C2 is sky) --
// packed band after band, and hands them to the caller's frame itself.
constexpr int TICK_BAND_ROWS = 8;
static_assert(TICK_BAND_ROWS % 8 == 0, "the Tick's bands hold whole tiles of an adaptive launch (adaptive_band_ok)");
struct Share {
    int band_rows, first, step, nb;  // bands (first, step) of band_rows rows, nb of them
    size_t words;                    // int32 of the packed band set inside the frame (a cut last band)
};
// The int32 of bands [k0, k1) of a share (the frame's last band may be cut at H).
inline size_t share_words(const Share& sh, int W, int H, int k0, int k1) {
    size_t rows = 0;
    for (int k = k0; k < k1; ++k) {
        const long long y0 = (long long)(sh.first + (long long)k * sh.step) * sh.band_rows;
        rows += (size_t)std::max(0LL, std::min<long long>(sh.band_rows, (long long)H - y0));
    }
    return rows * (size_t)W;
}
inline Share share_of(int W, int H, int g, int n, bool banded) {
    Share sh;
    sh.band_rows = (n == 1 && !banded) ? H : TICK_BAND_ROWS;
    sh.first = g, sh.step = n;
    sh.nb = bands_of(H, sh.band_rows, g, n);
    sh.words = share_words(sh, W, H, 0, sh.nb);
    return sh;
}
// Where band k of a share starts in the frame, in int32.
inline size_t band_word0(const Share& sh, int W, int k) {
    return (size_t)(sh.first + (size_t)k * sh.step) * (size_t)sh.band_rows * (size_t)W;
}
// Bands [k0, k1) of chunk c of nc of a share (none when the share has fewer bands than chunks).
struct Bands {
    int k0, k1;
};
inline Bands chunk_bands(const Share& sh, int c, int nc) {
    return Bands{(int)((long long)sh.nb * c / nc), (int)((long long)sh.nb * (c + 1) / nc)};
}
// The hand-off of bands [k0, k1) of a share, traced at src (packed from band k0), into the frame whose
// row 0 is at `frame` (a device-mapped host address or device memory of this worker).
inline CopyJob share_job(const Share& sh, int W, int H, int k0, int k1, const int32_t* src, int32_t* frame) {
    CopyJob j{};
    const size_t bw = (size_t)sh.band_rows * (size_t)W;
    j.src = src;
    j.dst = frame + band_word0(sh, W, k0);
    j.words = share_words(sh, W, H, k0, k1);
    j.band_words = sh.step == 1 ? 0u : (unsigned)bw;  // one worker: the bands are one contiguous run
    j.dst_stride = (unsigned long long)sh.step * bw;
    return j;
}

// The copies that hand bands [k0, k1) of a share, packed from band 0, to a frame, each as fn(dst, src, width,
// rows, pitch) in int32: `rows` runs of `width`, packed at src, to dst + r * pitch in the frame (pitch 0: one
// run, a plain copy).  One contiguous run (one worker), a pitched copy over the whole bands plus the frame's
// cut last band (a registered, pinned frame: the copy engine writes the rows in place), or one run per band (an
// unregistered frame -- the slow path; callers register Surface.pixels once -- where a pitched copy would be
// staged).  fn returns RT_OK to go on.
template <class Fn>
int for_band_copies(const Share& sh, int W, int H, int k0, int k1, bool pinned, Fn&& fn) {
    if (k1 <= k0) return RT_OK;
    const size_t bw = (size_t)sh.band_rows * (size_t)W;
    auto run = [&](int k, int n) { return fn(band_word0(sh, W, k), (size_t)k * bw, share_words(sh, W, H, k, k + n), 1, 0); };
    if (sh.step == 1) return run(k0, k1 - k0);
    if (pinned) {
        const bool cut = share_words(sh, W, H, k1 - 1, k1) < bw;
        const int full = k1 - k0 - (cut ? 1 : 0);
        if (full > 0) {
            const int rc = fn(band_word0(sh, W, k0), (size_t)k0 * bw, bw, (size_t)full, (size_t)sh.step * bw);
            if (rc != RT_OK) return rc;
        }
        return cut ? run(k1 - 1, 1) : RT_OK;
    }
    for (int k = k0; k < k1; ++k) {
        const int rc = run(k, 1);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

}  // namespace rtk
