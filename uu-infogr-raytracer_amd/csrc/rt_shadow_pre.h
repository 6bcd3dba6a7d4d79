// rt_shadow_pre.h -- the direct kernel's per-lane shadow pre-test, shared by the trace kernels (rt_kernel.hip
// shadow_scan) and host code (tests/native/shadow_group_host.cpp runs these very functions against the records of
// rt_scene.h build_shadow_pre / build_shadow_groups).  Device-free: compiled for host and device.
//
// The pre-test (culling only, FMA allowed): shadow_sphere_cull's line and behind rules for a single ray (R = 0)
// from the lane's hit point, with the margin split into the lane part m_l and the sphere part folded into the
// record (rt_scene.h build_shadow_pre: rules, margins, exactness).  A lane whose |O_f|_1 is 2^38 or more (or
// NaN) keeps every sphere (m_l = +inf).
//
// The group and union records of a light (DevShadowGroups, rt_scene.h build_shadow_groups) are tested by the same
// function with the lane margin enlarged once per scan: shadow_pre_widen(q, SHADOW_GROUP_WIDEN) for the groups and
// shadow_pre_widen(q, SHADOW_UNION_WIDEN) for the union.  The proof that a kept member keeps its group and a kept
// group keeps the union stands above build_shadow_groups.
#pragma once
#include "rt_internal.h"

#if defined(__HIPCC__)
#define RT_SHPRE_FN __host__ __device__ inline
#else
#define RT_SHPRE_FN inline
#endif

namespace rtk {

struct ShadowPreLane {
    float ou, ov, oa, ml;
};
RT_SHPRE_FN ShadowPreLane shadow_pre_lane(float hx, float hy, float hz, const DevLight& l) {
    ShadowPreLane q;
    q.ou = __builtin_fmaf(hz, l.uz, __builtin_fmaf(hy, l.uy, hx * l.ux));
    q.ov = __builtin_fmaf(hz, l.vz, __builtin_fmaf(hy, l.vy, hx * l.vx));
    q.oa = __builtin_fmaf(hz, l.az, __builtin_fmaf(hy, l.ay, hx * l.ax));
    const float l1 = __builtin_fabsf(q.ou) + __builtin_fabsf(q.ov) + __builtin_fabsf(q.oa);
    q.ml = l1 < 0x1p38f ? __builtin_fmaf(l1, 0x1.01p-8f, 0x1p-30f) : __builtin_inff();
    return q;
}
// true: sphere e may block this lane's shadow ray (NaN anywhere: kept)
RT_SHPRE_FN bool shadow_pre_keep(const ShadowPreLane& q, const DevShadowCull& e) {
    const float wu = e.cu - q.ou, wv = e.cv - q.ov;
    const float T = e.rr + q.ml;
    const bool line = __builtin_fmaf(wu, wu, wv * wv) > T * T;
    const bool behind = q.oa - e.ca > q.ml;
    return !(line || behind);
}

// The lane record of the group (k = SHADOW_GROUP_WIDEN) and union (k = SHADOW_UNION_WIDEN) tests: the same hit
// point with the margin m_l k, rounded (+inf stays +inf).  One multiplication per scan and level.
constexpr float SHADOW_GROUP_WIDEN = 1.0f + 0x1p-10f;
constexpr float SHADOW_UNION_WIDEN = 1.0f + 0x1p-9f;
RT_SHPRE_FN ShadowPreLane shadow_pre_widen(const ShadowPreLane& q, float k) {
    ShadowPreLane w = q;
    w.ml = q.ml * k;
    return w;
}

}  // namespace rtk
