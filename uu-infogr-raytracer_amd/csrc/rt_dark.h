// rt_dark.h -- the guard of the dark-tile skip, shared by the host (rt_api.cpp rt_set_scene), the trace
// kernels (rt_kernel.hip shade_direct / shade_bundle) and host code (tests/native/dark_host.cpp).
//
// At a plane hit on a dark checkerboard square (tile == 0) every light adds max(0, ((I' att) ph_c) * 0) per
// component (RayTracer.cs:773-775, I' = I or 0 by the shadow test), which is +0 whenever (I' att) ph_c is
// finite -- and NaN otherwise.  The two functions below prove the product finite without computing ph; where
// both hold the kernels skip the light loop (Phong and shadow scans) of that hit.  DESIGN.md 4 has the proof;
// its steps in short, for a hit point within 2^-5 of the plane (every hit point the kernels shade: fl(o + fl(d t))
// with t = fl(num / den) of that plane and the lane bounds below):
//   |lp - hp| > 2^-4 and every component below 2^13: ldir finite, |ldir| <= 1 + 2^-20;
//   |rs|^2 = |l|^2 + 4 (l.n)^2 (|n|^2 - 1) >= 0.99: normalize(rs) finite; view finite from 0.25 <= d.d <= 4;
//   pow(x <= 1 + 2^-19, 0 < n <= 1024) < 1.01, so |ph_c| < 2^22;  att = 1 / t^2 <= 2^14;
//   |I att ph_c| < 2^60 2^14 2^22 < 2^127.
// Every comparison is written so that a NaN fails it.
#pragma once
#include <stdint.h>

#include "rt_internal.h"

#if defined(__HIPCC__)
#define RT_DARK_FN __host__ __device__ inline
#else
#define RT_DARK_FN inline
#endif

namespace rtk {

// Host part, per plane with the scene's lights, in double on the device records (the values the kernels read);
// rt_set_scene stores the answer as MAT_DARK_OK in the plane material's flags.
RT_DARK_FN bool plane_dark_ok(const DevPlane& pl, const DevMaterial& m, const DevLight* li, int L) {
    const double nx = pl.nx, ny = pl.ny, nz = pl.nz;
    const double nn = nx * nx + ny * ny + nz * nz;
    if (!(__builtin_fabs(nn - 1.0) < 0x1p-10)) return false;
    if (!(__builtin_fabs((double)pl.cn) < 0x1p14)) return false;
    for (int k = 0; k < 3; ++k)
        if (!(__builtin_fabs((double)m.kd[k]) < 0x1p20 && __builtin_fabs((double)m.ks[k]) < 0x1p20)) return false;
    if ((m.flags & MAT_SPEC) && !(m.n > 0.0f && m.n <= 1024.0f)) return false;
    for (int i = 0; i < L; ++i) {
        const DevLight& l = li[i];
        if (!(__builtin_fabs((double)l.intensity) < 0x1p60)) return false;
        if (!(__builtin_fabs((double)l.px) < 0x1p12 && __builtin_fabs((double)l.py) < 0x1p12 &&
              __builtin_fabs((double)l.pz) < 0x1p12))
            return false;
        // the light's clearance from the plane, in the units of n.x - cn (|n| within 2^-10 of 1)
        const double h = (nx * (double)l.px + ny * (double)l.py + nz * (double)l.pz) - (double)pl.cn;
        if (!(__builtin_fabs(h) >= 0x1p-3)) return false;
    }
    return true;
}

// Lane part: the hit's point, distance, d.d of its ray (Vector3.Dot, as normalize(d) computes it) and tile.
RT_DARK_FN bool dark_lane_ok(float hx, float hy, float hz, float t, float dd, float tile) {
    return tile == 0.0f && t >= 0x1p-7f && t < 4096.0f && __builtin_fabsf(hx) < 4096.0f &&
           __builtin_fabsf(hy) < 4096.0f && __builtin_fabsf(hz) < 4096.0f && dd >= 0.25f && dd <= 4.0f;
}

}  // namespace rtk
