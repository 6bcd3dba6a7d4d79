// rt_progressive.h -- progressive accumulation (rt_set_progressive): the order in which a resting camera's Ticks
// take the k x k samples of a pixel, the view key that says whether the camera rested, and the plan of one Tick --
// what it launches, which samples it traces and what it divides by.  Device-free: rt_api.cpp keeps the state and
// issues the launches, tests/native/progressive_host.cpp checks the order against a table and the plan over
// scripted sequences.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/raytracer_hip.h"

namespace rtk {

// log2 of a progressive factor (1, 2, 4, 8), -1 for anything else.
inline int prog_log2(int k) { return k == 1 ? 0 : k == 2 ? 1 : k == 4 ? 2 : k == 8 ? 3 : -1; }

// Sample n (0 .. k^2 - 1, k = 1 << s) of a run: column i and row j of the pixel's k x k block.  n's base-4 digits
// d_0 (least significant) .. d_{s-1}: digit d_t gives bit s - 1 - t of i from its bit 0 and bit s - 1 - t of j from
// its bit 1 -- the coarse sub-grids come first, so the first 4^t samples are the samples of the factor 2^t
// (sample (i, j) of the block at 2^t is the reference's pixel (2^t x + i, 2^t y + j) of the 2^t W x 2^t H frame,
// whose view-plane point is that of pixel (k x + (k >> t) i, k y + (k >> t) j) at k W x k H).
inline void prog_sample(int s, int n, int* i, int* j) {
    int ci = 0, cj = 0;
    for (int t = 0; t < s; ++t) {
        const int d = (n >> (2 * t)) & 3;
        ci |= (d & 1) << (s - 1 - t);
        cj |= (d >> 1) << (s - 1 - t);
    }
    *i = ci, *j = cj;
}
// The pass code of sample n for the trace kernels (rt_kernel.hip sample_pixel): j k + i.
inline int prog_pass(int s, int n) {
    int i, j;
    prog_sample(s, n, &i, &j);
    return (j << s) | i;
}

// What a resting camera leaves unchanged between two Ticks.  The camera's floats are compared as bits (-0 and +0,
// or two NaNs of different payloads, are different views: a restart costs one plain frame, a missed one a wrong
// frame).  `plan` is the worker layout the accumulator follows: the number of band workers -- a worker's packed
// band set holds the same rows in the same order however a Tick chunks its share, so chunking is not part of it.
struct ProgKey {
    uint64_t scene;   // rt_set_scene calls so far
    uint32_t cam[5];  // position x, y, z, yaw, pitch
    int W, H, view_height, k;
    int plan;
};
inline ProgKey prog_key(uint64_t scene, const rt_camera& c, int W, int H, int view_height, int k, int plan) {
    ProgKey key{};
    const float f[5] = {c.position.x, c.position.y, c.position.z, c.yaw, c.pitch};
    static_assert(sizeof f == sizeof key.cam, "five binary32");
    std::memcpy(key.cam, f, sizeof f);
    key.scene = scene, key.W = W, key.H = H, key.view_height = view_height, key.k = k, key.plan = plan;
    return key;
}
inline bool prog_key_equal(const ProgKey& a, const ProgKey& b) {
    return a.scene == b.scene && std::memcmp(a.cam, b.cam, sizeof a.cam) == 0 && a.W == b.W && a.H == b.H &&
           a.view_height == b.view_height && a.k == b.k && a.plan == b.plan;
}

// One Tick.  PROG_PLAIN: the launch the library runs without the feature (the frame P_1; nothing touches the
// accumulator).  PROG_TRACE: a PROG launch that traces `samples` samples from index `first` on.  PROG_EMIT: a PROG
// launch that traces nothing and stores P_{k^2} again from the accumulator.  `divisor` is the c of the frame P_c the
// Tick outputs, and the run's count after it.
enum : int { PROG_PLAIN = 0, PROG_TRACE = 1, PROG_EMIT = 2 };
struct ProgPlan {
    int kind, first, samples, divisor;
};
// The state between Ticks: the key of the last Tick and the c of its frame (0: no run -- before any Tick, after a
// reset, after a failed Tick).
struct ProgRun {
    ProgKey key{};
    int count = 0;
};
// The plan of the Tick with key `now` after the run `run` (k = now.k; k = 1: always the plain launch), and the run
// after it.  The second Tick of a run traces samples 0 and 1 in one launch: sample 0 is the plain frame, which
// the first Tick rendered without the accumulator, so the accumulator starts there and is written without being read.
inline ProgPlan prog_plan(ProgRun* run, const ProgKey& now) {
    const int kk = now.k * now.k;
    const bool rests = now.k > 1 && run->count > 0 && prog_key_equal(run->key, now);
    ProgPlan p;
    if (!rests) p = ProgPlan{PROG_PLAIN, 0, 1, 1};
    else if (run->count == 1) p = ProgPlan{PROG_TRACE, 0, 2, 2};
    else if (run->count < kk) p = ProgPlan{PROG_TRACE, run->count, 1, run->count + 1};
    else p = ProgPlan{PROG_EMIT, kk, 0, kk};
    run->key = now;
    run->count = p.divisor;
    return p;
}

}  // namespace rtk
