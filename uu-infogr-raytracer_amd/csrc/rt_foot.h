// rt_foot.h -- plane footprints of the primary rays, shared by the host (rt_api.cpp view_fill), the direct trace
// kernel (rt_kernel.hip trace_tile_direct) and host code (tests/native/foot_host.cpp).  Culling only.
//
// A footprint is, per view and plane, three floats (a, b, c) with the rule: the binary32 primary plane test
// (plane_take: may = num and den nonzero with equal signs) cannot select the plane at a pixel with view-table values
// (lx, ly) whenever fma(a, lx, fma(b, ly, c)) < 0.  NaN keeps the plane.  A wave whose pixels lie outside every
// sphere's screen box and fail the rule for every plane traces nothing: its pixels are 0 (the sky).
//
// num = ((-o.x nx - o.y ny) - o.z nz) + cn has the camera as o on every lane: one value per view, computed here
// with the kernel's own operations.  +-0 or NaN: may is false everywhere, the footprint is "never" (0, 0, -1).
// Otherwise s = sign(num), and the plane is selectable only where den = fl(dot(d, n)) has the sign s.  With
// D = R lx + U ly + F lz the exact direction of the pixel and w = fl(vp - cam) the kernel's (eps = 2^-24):
//   |w - D| <= E1 = 2^-19 (|cam| + dmax): three products and three sums per component of vp, then the difference
//       (per component below 3 eps |cam| + 5 eps (|lx| + |ly| + |lz|); prim_box takes 2^-20 of the same sum);
//   d_k = sigma w_k (1 + delta), sigma = fl(1 / sqrt(w.w)) > 0, and den = sum_k d_k n_k (1 + theta_k) with three
//       roundings in theta: sign(den) = sign(sum_k w_k n_k (1 + e_k)), |e_k| <= (1 + eps)^4 - 1 < 2^-21, so
//       |sum - n.w| <= 2^-21 |n| (dmax + E1);
//   so den has the sign -s, or is +-0, whenever s n.D < -Merr, Merr = |n| (E1 + 2^-21 (dmax + E1)) + 2^-100 (the
//       last term: underflows in d_k and d_k n_k, below 2^-107 in the ranges required here).
// The rule is evaluated in binary32 from rounded a, b: V = fl(a lx + fl(b ly + c)) < 0 implies a lx + fl(b ly + c)
// < 0 (rounding keeps the sign), hence a lx + b ly + c < Ev = eps (|b| lymax + |c|) + 2^-150.  c therefore carries
// s n.F lz + Merr + |a - s n.R| lxmax + |b - s n.U| lymax + the double evaluation's own slack + Ev, rounded up.
// Preconditions (else no footprints at all, foot_n = -1): at most FOOT_MAX planes; every normal component finite
// and |n| in [2^-20, 2^20]; the camera finite; pw, ph, lz finite, lz in [2^-20, 2^20], pw, ph in (0, 2^20]; the
// basis orthonormal to 2^-18 and the direction error 2^-20 (|cam| + dmax) / lz + 2^-20 <= 2^-12 (prim_box's own).
// margins = false (the host check's teeth): a, b, c rounded to nearest, no Merr and no direction-error bound.
#pragma once
#include <cmath>

#include "rt_internal.h"

#if defined(__HIPCC__)
#define RT_FOOT_FN __host__ __device__ inline
#else
#define RT_FOOT_FN inline
#endif

namespace rtk {

// The lane's part of the rule: false = the plane cannot be selected at (lx, ly).
RT_FOOT_FN bool foot_may_hit(const PlaneFoot& f, float lx, float ly) {
    return !(__builtin_fmaf(f.a, lx, __builtin_fmaf(f.b, ly, f.c)) < 0.0f);
}

// plane_take's numerator at the camera, in its operation order (built without FMA contraction).
inline float foot_num(const float* cam, const DevPlane& q) {
    return ((-cam[0] * q.nx - cam[1] * q.ny) - cam[2] * q.nz) + q.cn;
}

// The footprints of the view in lp (cam .. fwd, pw, ph, nearc) for planes pl[0..P): P, or -1 for none.
inline int foot_build(const LaunchParams& lp, const DevPlane* pl, int P, PlaneFoot* out, bool margins = true) {
    if (P < 0 || P > FOOT_MAX) return -1;
    const double pw = lp.pw, ph = lp.ph, lz = lp.nearc;
    if (!(pw > 0 && pw <= 0x1p20) || !(ph > 0 && ph <= 0x1p20) || !(lz >= 0x1p-20 && lz <= 0x1p20)) return -1;
    const double cam[3] = {lp.cam[0], lp.cam[1], lp.cam[2]};
    const double camlen = std::sqrt(cam[0] * cam[0] + cam[1] * cam[1] + cam[2] * cam[2]);
    if (!std::isfinite(camlen)) return -1;
    auto fdot = [](const float* a, const float* b) { return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]; };
    const double ortho = std::fabs(fdot(lp.right, lp.up)) + std::fabs(fdot(lp.right, lp.fwd)) +
                         std::fabs(fdot(lp.up, lp.fwd)) + std::fabs(fdot(lp.right, lp.right) - 1.0) +
                         std::fabs(fdot(lp.up, lp.up) - 1.0) + std::fabs(fdot(lp.fwd, lp.fwd) - 1.0);
    if (!(ortho < 0x1p-18)) return -1;
    const double lxmax = 0.5 * pw * (1.0 + 0x1p-20), lymax = 0.5 * ph * (1.0 + 0x1p-20);
    const double dmax = std::sqrt(lxmax * lxmax + lymax * lymax + lz * lz) * (1.0 + 0x1p-16);
    const double dir_err = 0x1p-20 * (camlen + dmax) / lz + 0x1p-20;
    if (margins && !(dir_err <= 0x1p-12)) return -1;
    const double E1 = 0x1p-19 * (camlen + dmax);
    for (int i = 0; i < P; ++i) {
        const float n[3] = {pl[i].nx, pl[i].ny, pl[i].nz};
        const double nlen = std::sqrt(fdot(n, n));
        if (!(nlen >= 0x1p-20 && nlen <= 0x1p20)) return -1;  // (a NaN or inf component fails it too)
    }
    for (int i = 0; i < P; ++i) {
        const float n[3] = {pl[i].nx, pl[i].ny, pl[i].nz};
        const float num = foot_num(lp.cam, pl[i]);
        if (!(num > 0.0f || num < 0.0f)) {  // +-0 or NaN: never selectable
            out[i] = PlaneFoot{0.0f, 0.0f, -1.0f};
            continue;
        }
        const double s = num > 0.0f ? 1.0 : -1.0;
        const double nlen = std::sqrt(fdot(n, n));
        const double ad = s * fdot(n, lp.right), bd = s * fdot(n, lp.up), cd = s * fdot(n, lp.fwd) * lz;
        const float a = (float)ad, b = (float)bd;
        if (!margins) {
            out[i] = PlaneFoot{a, b, (float)cd};
            continue;
        }
        const double merr = nlen * (E1 + 0x1p-21 * (dmax + E1)) + 0x1p-100;
        const double dbl = 0x1p-48 * nlen * (lxmax + lymax + lz);
        const double cpre = cd + merr + std::fabs((double)a - ad) * lxmax + std::fabs((double)b - bd) * lymax + dbl;
        const double ev = 0x1p-23 * (std::fabs((double)b) * lymax + std::fabs(cpre)) + 0x1p-140;
        const double cw = cpre + ev;
        float c = (float)cw;
        if ((double)c < cw) c = std::nextafter(c, INFINITY);
        out[i] = PlaneFoot{a, b, c};
    }
    return P;
}

}  // namespace rtk
