// rt_scene.h -- the scene image the kernels read, built on the host: the device records of rt_internal.h packed
// into one blob, with the scene-constant tables that decide what the kernels may skip (shadow thresholds, cull radii,
// shadow-cull frames, shadow grids, sphere clusters, the shadow pre-test, the dark-tile bit).  Device-free: plain
// C++17 that makes no runtime call and reads no environment, shared by the library (rt_api.cpp rt_set_scene uploads
// what scene_build returns) and by host programs that check the tables against the oracle (tests/native).
// Built without FMA contraction (-ffp-contract=off): the binary32 values here are the ones the kernels compare with.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/raytracer_hip.h"
#include "rt_dark.h"
#include "rt_internal.h"

namespace rtk {

// Host-side Vector3 helpers (binary32, no contraction: built with -ffp-contract=off).
struct H3 {
    float x, y, z;
};
inline H3 h3(rt_vec3 v) { return H3{v.x, v.y, v.z}; }
inline float hdot(H3 a, H3 b) { return ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z); }
inline H3 hcross(H3 l, H3 r) {
    return H3{(l.y * r.z) - (l.z * r.y), (l.z * r.x) - (l.x * r.z), (l.x * r.y) - (l.y * r.x)};
}
inline H3 hnormalize(H3 a) {
    float s = 1.0f / std::sqrt(hdot(a, a));
    return H3{a.x * s, a.y * s, a.z * s};
}
inline bool hzero(rt_vec3 v) { return v.x == 0 && v.y == 0 && v.z == 0; }

inline DevMaterial dev_material(const rt_material& m, rt_vec3 ambient) {
    DevMaterial d;
    std::memset(&d, 0, sizeof d);
    d.kd[0] = m.kd.x, d.kd[1] = m.kd.y, d.kd[2] = m.kd.z;
    d.amb[0] = ambient.x * m.ka.x, d.amb[1] = ambient.y * m.ka.y, d.amb[2] = ambient.z * m.ka.z;
    d.ks[0] = m.ks.x, d.ks[1] = m.ks.y, d.ks[2] = m.ks.z;
    d.n = m.n;
    d.km[0] = m.km.x, d.km[1] = m.km.y, d.km[2] = m.km.z;
    d.flags = (hzero(m.km) ? 0u : MAT_MIRROR) | (hzero(m.kd) ? 0u : MAT_DIFFUSE) |
              ((!hzero(m.ks) && m.n > 0.0f) ? MAT_SPEC : 0u);
    d.pow_kind = m.n == 1.0f ? POW_ONE : m.n == 0.5f ? POW_HALF : m.n == 2.0f ? POW_TWO : POW_GENERIC;
    return d;
}

// Shadow rays (IntersectShadowLight, RayTracer.cs:573-582 -> IntersectsSphere with epsilon
// 0.001f, :613-636): with 2a finite and > 0 the ray collides iff fl(fl(n / 2a) - e) > 0, n =
// fl(-b - sqrt(disc)) (the near root decides, rt_kernel.hip shadow_blocked).  For floats q and
// e the sign of fl(q - e) is that of q - e, so the test is fl(n / 2a) > e.  Correct rounding is
// monotonic: fl(z) > e iff z > m, m = e + ulp(e)/2 the midpoint above e, except z == m, which
// rounds to the even neighbour -- succ(e) when e's significand is odd.  So the collision is
// n >= m * 2a (odd e) or n > m * 2a (even e); m has 25 significant bits and 2a 24, so the
// product is exact in double, and for a float n, "n >= T" equals "n >= the smallest float >= T"
// (and "n > T" equals "n >= the smallest float > T").  Returns that float (+inf above FLT_MAX).
inline float shadow_threshold(float a2) {
    const float e = 0.001f;
    int ex = 0;
    (void)std::frexp(e, &ex);                                // e = f * 2^ex, f in [0.5, 1)
    const double m = (double)e + std::ldexp(1.0, ex - 25);  // + ulp(e) / 2 (ulp = 2^(ex - 24))
    uint32_t eb;
    std::memcpy(&eb, &e, sizeof eb);
    const bool odd = (eb & 1u) != 0;
    const double T = m * (double)a2;                         // exact
    float t = (float)T;
    if ((double)t < T || (!odd && (double)t == T)) t = std::nextafter(t, INFINITY);
    return t;
}

struct SceneLayout {
    int S = 0, P = 0, L = 0, limit = 0;
    size_t off_sph = 0, off_mat = 0, off_pl = 0, off_li = 0, off_cull = 0, off_shcull = 0, bytes = 0;
    size_t off_shg = 0, off_shgrid = 0, off_shslab = 0, off_clus = 0, off_shpre = 0;
    bool has_shpre = false;  // the direct kernel's shadow pre-test records (DevShadowCull [L][S + (S & 1)])
    size_t off_shgrp = 0;
    bool has_shgrp = false;  // their group and union records (DevShadowGroups [L]); RT_SHADOW_GROUPS=0: none
    bool mirror_box = true;  // the direct kernel's mirrored screen boxes (view_mirror_boxes); RT_MIRROR_BOX=0: off
    bool prim_foot = true;   // the direct kernel's plane footprints (rt_foot.h, view_build); RT_PRIM_FOOT=0: off
    bool uniform_plane = true;  // the direct kernel's plane-uniform waves (LaunchParams::uniform_plane); RT_UNIFORM_PLANE=0: off
    int n_clus = 0;  // DevCluster records (the bundle kernel's per-lane pre-cull), 0: none
    bool has_shcull = false;
    bool has_shg = false;  // per-light shadow grids (DevShadowGrid) for the merged shadow pass
    std::vector<unsigned char> host_blob;  // the uploaded scene image (host tests read the tables)
    bool generic_pow = false;        // a specular material with n not in {0.5, 1, 2}
    bool lights_a2_ok = true;        // every light's 2a = 2 p.p finite and > 0
    std::vector<DevSphere> host_sph;  // for the per-frame primary constants
    std::vector<DevPlane> host_pl;    // for the single-frame launches' row order (row_order)
};

// What rt_set_scene reads from the environment (the defaults: nothing set), one switch per table (A/B and tests).
struct SceneOptions {
    bool shadow_grid = true;  // RT_SHADOW_GRID=0: no shadow grids (the merged pass keeps the per-level bound)
    bool shadow_pre = true;   // RT_SHADOW_PRE=0: no shadow pre-test records
    bool shadow_groups = true;  // RT_SHADOW_GROUPS=0: no group and union records over them (the flat pair loop)
    bool mirror_box = true;   // RT_MIRROR_BOX=0: no mirrored screen boxes (SceneLayout::mirror_box)
    bool dark_skip = true;    // RT_DARK_SKIP=0: MAT_DARK_OK stays clear
    bool prim_foot = true;    // RT_PRIM_FOOT=0: no plane footprints (SceneLayout::prim_foot)
    bool uniform_plane = true;  // RT_UNIFORM_PLANE=0: no wave is plane-uniform (SceneLayout::uniform_plane)
    int cluster_size = CLUSTER_SIZE;  // RT_TRACE_CLUSTERS=0: no clusters, =2..16: spheres per cluster
};

// Light frame in double (the DevLight frame is its binary32 rounding).
struct Frame3 {
    double U[3], V[3], A[3];
};

// The lowest value x (double) that binary32 fma(x, s, o) can map to a value >= k (k integer): every
// x_f with floor(fl(x_f * s + o)) == k satisfies x_f >= cell_lo(k, s, o), and every x_f with that
// floor <= k - 1 satisfies x_f < cell_lo(k, s, o)... up to the allowance eps_k (a relative 2^-24 of
// the fma result plus double rounding here, taken 4x).  s > 0.
inline double cell_lo(int k, float s, float o) { return ((double)k - 0x1p-22 * (std::fabs((double)k) + 2.0) - (double)o) / (double)s; }
inline double cell_hi(int k, float s, float o) {  // the highest x that can map to k (exclusive bound of k + 1)
    return ((double)(k + 1) + 0x1p-22 * (std::fabs((double)k + 1.0) + 2.0) - (double)o) / (double)s;
}
inline float down(double v) { float f = (float)v; return (double)f > v ? std::nextafter(f, -INFINITY) : f; }
inline float up(double v) { float f = (float)v; return (double)f < v ? std::nextafter(f, INFINITY) : f; }

// The direct kernel's shadow pre-test records (rt_kernel.hip shadow_pre_keep; culling only).  The kernel drops
// sphere i for a lane's shadow ray toward light l only under shadow_sphere_cull's rules for a single ray (R = 0)
// from the lane's hit point O: w = C - O in the light's frame, margin 2^-8 dc + 2^-18 |O| with dc >= |C - O|,
// line miss if w_u^2 + w_v^2 > (r' + 2^-18 |C| + margin)^2, behind if -w_a > margin.  Here dc is bounded by
// |O_f|_1 + |C_f|_1 (frame coordinates), so the margin splits into a lane part m_l = 2^-8 (1 + 2^-8) |O_f|_1 +
// 2^-30 (kernel: it also covers the 2^-18 |O| projection allowance, and its 2^-30 floor makes every cull imply
// |C - O| > 2^-30) and a sphere part m_c = 2^-8 (1 + 2^-20) |C_f|_1, folded in here: ca' = ca + m_c and
// rr' = r' + 2^-18 |C| + m_c, both rounded up.  Records that allow no culling -- a light whose a = p.p is outside
// [2^-40, 2^40] or whose 2a is not finite, a sphere without a usable cull radius (NaN, < 2^-50), |C_f|_1 >= 2^38
// or non-finite -- get ca' = rr' = +inf (no rule can hold); the padding sphere of an odd count gets cu = +inf
// (always dropped: it never hits).
inline void build_shadow_pre(const DevLight* li, int n_lights, const DevSphereCull* cull, int n_spheres, int s_pad,
                      DevShadowCull* out) {
    for (int j = 0; j < n_lights; ++j) {
        const DevLight& d = li[j];
        const bool l_ok = d.a >= 0x1p-40f && d.a <= 0x1p40f && d.a2 > 0.0f && d.a2 < INFINITY;
        for (int i = 0; i < s_pad; ++i) {
            DevShadowCull& e = out[(size_t)j * (size_t)s_pad + (size_t)i];
            if (i >= n_spheres) {
                e = DevShadowCull{INFINITY, 0.0f, 0.0f, 0.0f};
                continue;
            }
            const double c[3] = {cull[i].cx, cull[i].cy, cull[i].cz};
            const double clen = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            const double cu = c[0] * d.ux + c[1] * d.uy + c[2] * d.uz;
            const double cv = c[0] * d.vx + c[1] * d.vy + c[2] * d.vz;
            const double ca = c[0] * d.ax + c[1] * d.ay + c[2] * d.az;
            const double l1 = std::fabs((double)(float)cu) + std::fabs((double)(float)cv) + std::fabs((double)(float)ca);
            const double mc = 0x1p-8 * l1 * (1.0 + 0x1p-20);
            const bool ok = l_ok && cull[i].rr >= 0x1p-50f && l1 < 0x1p38 && std::isfinite(cull[i].rr) && std::isfinite(clen);
            if (!ok) {
                e = DevShadowCull{0.0f, 0.0f, INFINITY, INFINITY};
                continue;
            }
            e.cu = (float)cu;
            e.cv = (float)cv;
            e.ca = std::nextafter((float)((double)(float)ca + mc), INFINITY);
            e.rr = std::nextafter((float)((double)cull[i].rr + 0x1p-18 * clen + mc), INFINITY);
        }
    }
}

// The smallest disc that contains the discs (x[i], y[i], r[i]), i in idx (not empty; finite values), to within
// 2^-30 of their box: centre (*cx, *cy); the caller derives the radius from the centre it stores.  When the disc
// spanned by the pair with the largest span -- or the largest member alone -- contains every member, it is the
// answer; otherwise f(c) = max_i |c - c_i| + r_i is convex in c and a nested ternary search over the box of the
// centres finds its minimum.
inline void enclosing_disc(const double* x, const double* y, const double* r, const std::vector<int>& idx, double* cx, double* cy) {
    auto far = [&](double px, double py) {
        double f = 0.0;
        for (int i : idx) f = std::max(f, std::hypot(x[i] - px, y[i] - py) + r[i]);
        return f;
    };
    double bx = x[idx[0]], by = y[idx[0]], br = r[idx[0]];
    double x0 = bx, x1 = bx, y0 = by, y1 = by;
    for (int i : idx) {
        if (r[i] > br) bx = x[i], by = y[i], br = r[i];
        x0 = std::min(x0, x[i]), x1 = std::max(x1, x[i]), y0 = std::min(y0, y[i]), y1 = std::max(y1, y[i]);
    }
    for (int i : idx)
        for (int j : idx) {
            const double d = std::hypot(x[j] - x[i], y[j] - y[i]);
            const double span = 0.5 * (d + r[i] + r[j]);
            if (j <= i || !(d > 0.0) || span <= br || span <= r[i] || span <= r[j]) continue;
            const double t = (span - r[i]) / d;  // the centre lies span - r_i from c_i toward c_j
            bx = x[i] + (x[j] - x[i]) * t, by = y[i] + (y[j] - y[i]) * t, br = span;
        }
    *cx = bx, *cy = by;
    if (far(bx, by) <= br * (1.0 + 0x1p-40)) return;
    auto best_y = [&](double px, double* py) {
        double lo = y0, hi = y1;
        for (int k = 0; k < 52; ++k) {
            const double a = lo + (hi - lo) / 3.0, b = hi - (hi - lo) / 3.0;
            if (far(px, a) <= far(px, b)) hi = b; else lo = a;
        }
        *py = 0.5 * (lo + hi);
        return far(px, *py);
    };
    double lo = x0, hi = x1, py = by;
    for (int k = 0; k < 52; ++k) {
        const double a = lo + (hi - lo) / 3.0, b = hi - (hi - lo) / 3.0;
        if (best_y(a, &py) <= best_y(b, &py)) hi = b; else lo = a;
    }
    const double px = 0.5 * (lo + hi);
    if (best_y(px, &py) < far(bx, by)) *cx = px, *cy = py;
}

// The record (DevShadowCull-shaped) that contains the records m[0..n) -- members of a group, or the groups of a light:
// centre near the centre of the smallest disc enclosing their discs, rounded to binary32; rr >= max_i (|c - c_i| +
// rr_i) (1 + 2^-16), from the rounded centre, in double, rounded up; ca = max_i ca_i.  A member without a usable
// record (rr or ca not finite) gives {0, 0, +inf, +inf}: always kept; n = 0 gives {+inf, 0, 0, 0}: never kept by a
// lane with a finite margin (the padding sphere's record).
inline DevShadowCull shadow_enclose(const DevShadowCull* m, int n) {
    if (n == 0) return DevShadowCull{INFINITY, 0.0f, 0.0f, 0.0f};
    std::vector<double> x((size_t)n), y((size_t)n), r((size_t)n);
    std::vector<int> idx((size_t)n);
    float ca = -INFINITY;
    for (int i = 0; i < n; ++i) {
        if (!(std::isfinite(m[i].rr) && std::isfinite(m[i].ca) && std::isfinite(m[i].cu) && std::isfinite(m[i].cv)))
            return DevShadowCull{0.0f, 0.0f, INFINITY, INFINITY};
        x[(size_t)i] = m[i].cu, y[(size_t)i] = m[i].cv, r[(size_t)i] = m[i].rr, idx[(size_t)i] = i;
        ca = std::max(ca, m[i].ca);
    }
    double cx = 0.0, cy = 0.0;
    enclosing_disc(x.data(), y.data(), r.data(), idx, &cx, &cy);
    DevShadowCull e;
    e.cu = (float)cx, e.cv = (float)cy, e.ca = ca;
    double rr = 0.0;
    for (int i = 0; i < n; ++i) rr = std::max(rr, std::hypot(x[(size_t)i] - (double)e.cu, y[(size_t)i] - (double)e.cv) + r[(size_t)i]);
    e.rr = std::nextafter(up(rr * (1.0 + 0x1p-16)), INFINITY);
    return e;
}

// The group and union records of the shadow pre-test (DevShadowGroups [L], rt_internal.h; culling only), from each
// light's finished pre-test records `pre` ([L][s_pad], build_shadow_pre).
//
// Groups: the spheres without a usable record (ca' = rr' = +inf) form one group; the others start as one group each
// and the two whose discs span the least (complete linkage on (d_ij + rr_i + rr_j) / 2) merge until at most
// `groups` remain in all.  The padding sphere of an odd count is in no group.  Every group's record is
// shadow_enclose of its members, the union's is shadow_enclose of the group records; a group with an unusable member
// and the union over it are +inf.  The masks are disjoint and cover exactly the spheres 0..S-1.
//
// Soundness.  The kernel skips sphere i for a wave when no lane keeps the union, or no lane keeps i's group; it must
// skip only spheres that shadow_pre_keep(q, member i) drops on every lane.  So for every lane record q that
// shadow_pre_lane makes (m_l = +inf, or every coordinate finite with |O_f|_1 < 2^38 and 2^-30 <= m_l < 2^31):
//     keep(q, member)  =>  keep(widen(q, 1 + 2^-10), its group)  =>  keep(widen(q, 1 + 2^-9), union),
// with keep = !(line || behind); it suffices that each rule of the enclosing record implies the rule of the enclosed.
// m_l = +inf: T = +inf, T T = +inf and nothing exceeds it; oa - ca > +inf never holds: every record is kept.
// A +inf record likewise keeps every lane.  An empty group has mask 0.  Otherwise, with u = 2^-24, records e (inner,
// margin m) and g (outer, margin m' = fl(m k), k >= (1 + 2^-10) m-ratio of the two levels):
//   behind: ca_g >= ca_e, binary32 subtraction is monotonic, so fl(oa - ca_g) <= fl(oa - ca_e); and m' >= m because
//     rounding is monotonic and m k >= m.  fl(oa - ca_g) > m'  =>  fl(oa - ca_e) > m.
//   line: let D be the true distance of (ou, ov) from a record's centre and T^ = rr + m in the reals.  |C_f|_1 and
//     |O_f|_1 are below 2^38 and an enclosing centre lies in the box of its members', so |w| < 2^40, s cannot
//     overflow, and the computed s = fl(fma(wu, wu, fl(wv wv))) lies within D^2 (1 +- u)^4 -+ 2^-149 (the one
//     product that can underflow); T^ >= 2^-30, so fl(fl(T^)^2) lies within T^^2 (1 +- u)^3, or it
//     overflows to +inf (rr' of a huge sphere): then no line rule holds for this record, nor for a record that
//     encloses it, whose fl(T^) is no smaller (rr_g + m' >= rr_e + m, rounding is monotonic).  Hence
//         line  =>  D > T^ (1 - 2^-21)        and        D > T^ (1 + 2^-21)  =>  line
//     (2^-149 is far below 2^-21 T^^2 >= 2^-81).  With d the distance of the two centres, D_e >= D_g - d:
//         line_g  =>  D_e > (rr_g + m')(1 - 2^-21) - d.
//     rr_g >= (d + rr_e)(1 + 2^-16) gives rr_g (1 - 2^-21) >= d + rr_e (1 + 2^-21) -- a relative inflation covers
//     the record's own term -- and m' >= m (1 + 2^-10)(1 - u) gives m' (1 - 2^-21) >= m (1 + 2^-21): the lane
//     margin, which can be large against rr at distant hit points (m_l = 2^-8 |O|_1), is covered by widening it, not
//     by rr.  So D_e > (rr_e + m)(1 + 2^-21): line_e.  (d and rr are evaluated in double from the stored binary32
//     centres: errors of 2^-50 relative, against the 2^-16 allowed.)
//   The union's margin k = 1 + 2^-9 is the group margin times at least (1 + 2^-10)(1 - 2^-11) > 1 + 2^-11, which
//   the same step needs only to exceed (1 + 2^-21)(1 + u)^2 / (1 - 2^-21).
// tests/native/shadow_group_host.cpp checks the chain in binary32 with the kernel's functions.
inline void build_shadow_groups(const DevShadowCull* pre, int n_lights, int n_spheres, int s_pad, DevShadowGroups* out,
                                int groups = SHADOW_GROUPS) {
    groups = std::max(1, std::min(groups, SHADOW_GROUPS));
    for (int j = 0; j < n_lights; ++j) {
        const DevShadowCull* e = pre + (size_t)j * (size_t)s_pad;
        DevShadowGroups& g = out[j];
        std::memset(&g, 0, sizeof g);
        std::vector<std::vector<int>> cl;
        std::vector<int> bad;
        for (int i = 0; i < n_spheres; ++i) {
            if (std::isfinite(e[i].rr) && std::isfinite(e[i].ca)) cl.push_back(std::vector<int>(1, i));
            else bad.push_back(i);
        }
        const size_t room = (size_t)groups - (bad.empty() ? 0 : 1);
        auto span = [&](const std::vector<int>& a, const std::vector<int>& b) {  // complete linkage
            double s = 0.0;
            for (int p : a)
                for (int q : b)
                    s = std::max(s, 0.5 * (std::hypot((double)e[p].cu - (double)e[q].cu, (double)e[p].cv - (double)e[q].cv) +
                                           (double)e[p].rr + (double)e[q].rr));
            return s;
        };
        while (cl.size() > std::max<size_t>(room, 1)) {
            size_t ba = 0, bb = 1;
            double bs = INFINITY;
            for (size_t a = 0; a < cl.size(); ++a)
                for (size_t b = a + 1; b < cl.size(); ++b) {
                    const double s = span(cl[a], cl[b]);
                    if (s < bs) bs = s, ba = a, bb = b;
                }
            cl[ba].insert(cl[ba].end(), cl[bb].begin(), cl[bb].end());
            cl.erase(cl.begin() + (std::ptrdiff_t)bb);
        }
        if (!bad.empty()) {
            if (room == 0 && !cl.empty()) {  // one group in all: the unusable members share it
                bad.insert(bad.end(), cl[0].begin(), cl[0].end());
                cl.clear();
            }
            cl.insert(cl.begin(), bad);
        }
        for (int k = 0; k < SHADOW_GROUPS; ++k) {
            std::vector<DevShadowCull> m;
            if ((size_t)k < cl.size())
                for (int i : cl[(size_t)k]) m.push_back(e[i]), g.mask[k] |= 1u << i;
            g.grp[k] = shadow_enclose(m.data(), (int)m.size());
        }
        const int used = (int)std::min<size_t>(cl.size(), SHADOW_GROUPS);
        g.uni = shadow_enclose(g.grp, used);
    }
}

// The bundle kernel's shadow-cull records (DevShadowCull [L][S]): sphere centres in each light's shadow-cull frame
// (culling only).
inline void build_shadow_cull(const DevLight* li, int n_lights, const DevSphereCull* cull, int n_spheres,
                              DevShadowCull* sc) {
    for (int j = 0; j < n_lights; ++j)
        for (int i = 0; i < n_spheres; ++i) {
            const DevLight& d = li[j];
            const double c[3] = {cull[i].cx, cull[i].cy, cull[i].cz};
            const double clen = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            DevShadowCull& e = sc[(size_t)j * (size_t)n_spheres + (size_t)i];
            e.cu = (float)(c[0] * d.ux + c[1] * d.uy + c[2] * d.uz);
            e.cv = (float)(c[0] * d.vx + c[1] * d.vy + c[2] * d.vz);
            e.ca = (float)(c[0] * d.ax + c[1] * d.ay + c[2] * d.az);
            // r' + 2^-18 |C|, rounded up (NaN / inf stay: the kernel keeps such spheres)
            e.rr = std::nextafter((float)((double)cull[i].rr + 0x1p-18 * clen), INFINITY);
        }
}

// The bundle kernel's sphere clusters (rt_internal.h DevCluster): median splits of the sphere centres along the
// widest axis of their box until a group holds at most `size` spheres; each cluster's centre is the middle of
// its members' box (rounded to float) and R, computed in double from that rounded centre and rounded up, bounds
// |c_i - centre| + r'_i for every member (r' = the DevSphereCull radius, itself >= r (1 + 2^-8)).  A member
// without a usable cull record (NaN / infinite centre or radius) makes its cluster's R NaN: never culled.
// Returns the cluster count (<= MAX_CLUSTERS).
inline int build_clusters(const DevSphereCull* cull, int S, int size, DevCluster* out) {
    std::vector<std::vector<int>> todo(1, std::vector<int>((size_t)S)), groups;
    for (int i = 0; i < S; ++i) todo[0][(size_t)i] = i;
    while (!todo.empty()) {
        std::vector<int> g = std::move(todo.back());
        todo.pop_back();
        if ((int)g.size() <= size) {
            groups.push_back(std::move(g));
            continue;
        }
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i : g) {
            const double c[3] = {cull[i].cx, cull[i].cy, cull[i].cz};
            for (int k = 0; k < 3; ++k) lo[k] = std::fmin(lo[k], c[k]), hi[k] = std::fmax(hi[k], c[k]);
        }
        int ax = 0;
        for (int k = 1; k < 3; ++k)
            if (hi[k] - lo[k] > hi[ax] - lo[ax]) ax = k;
        auto key = [&](int i) {  // (NaN last: a strict weak order for the sort)
            const float k = ax == 0 ? cull[i].cx : ax == 1 ? cull[i].cy : cull[i].cz;
            return std::isnan(k) ? INFINITY : k;
        };
        std::stable_sort(g.begin(), g.end(), [&](int a, int b) { return key(a) < key(b); });
        const size_t h = g.size() / 2;
        todo.emplace_back(g.begin(), g.begin() + (long)h);
        todo.emplace_back(g.begin() + (long)h, g.end());
    }
    if ((int)groups.size() > MAX_CLUSTERS) return 0;
    int n = 0;
    for (const std::vector<int>& g : groups) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool usable = true;
        unsigned long long m = 0;
        for (int i : g) {
            const double c[3] = {cull[i].cx, cull[i].cy, cull[i].cz};
            for (int k = 0; k < 3; ++k) lo[k] = std::fmin(lo[k], c[k]), hi[k] = std::fmax(hi[k], c[k]);
            usable = usable && std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) &&
                     std::isfinite((double)cull[i].rr) && cull[i].rr >= 0x1p-50f;
            m |= 1ull << i;
        }
        DevCluster& c = out[n++];
        c.cx = (float)((lo[0] + hi[0]) / 2), c.cy = (float)((lo[1] + hi[1]) / 2), c.cz = (float)((lo[2] + hi[2]) / 2);
        double R = 0;
        for (int i : g) {
            const double dx = (double)cull[i].cx - c.cx, dy = (double)cull[i].cy - c.cy, dz = (double)cull[i].cz - c.cz;
            R = std::fmax(R, std::sqrt(dx * dx + dy * dy + dz * dz) + (double)cull[i].rr);
        }
        c.R = usable && R < 0x1p40 ? std::nextafter((float)(R * (1.0 + 0x1p-20)), INFINITY) : NAN;
        c.members = m;
        c.pad = 0;
    }
    return n;
}

// Shadow grid of one light (DevShadowGrid; culling only -- a sphere left out of a lane's mask must
// provably not block that lane's shadow ray in binary32).  The argument (rt_kernel.hip cull_mask):
// IntersectsSphere yields disc < 0 when the exact line-to-centre distance D >= r (1 + 3 eps) +
// 9.2e-4 |u| (u = hp - C), and b >= 0 when (hp - C).A >= 4 eps |u|; either makes the ray unblocked.
// For a lane with |hp|_1 <= B: |u| <= |C|_1 + B, and its binary32 projections u_f = hp.U etc. are
// within 2^-21 |hp|_1 <= 2^-21 B of the exact ones in the double frame (U_f rounds U to 2^-24, three
// products and two sums round to 2^-24 each).  So, with T_j = r'_j + 2^-8 (|C_j|_1 + B) + 2^-20 B
// (r' >= r (1 + 2^-8) from DevSphereCull): a sphere whose centre lies farther than T_j from every
// (u, v) a lane of cell (iu, iv) can have -- the cell's interval from the device's own fma/floor
// mapping (cell_lo/cell_hi), grown by 2^-20 B -- has D > r (1 + 3 eps) + 2^-8 |u| (a 4x margin
// over 9.2e-4); cells outside the grid hold no such disc at all.  Axially, sphere j may be ahead of
// slab k only if ca_j + mB_j > a_lo(k), mB_j = 2^-8 (|C_j|_1 + B) + 2^-20 B; otherwise every lane in
// the slab has (hp - C).A >= 2^-8 (|C_j|_1 + B) >> 4 eps |u| (b >= 0).  Lanes beyond B: their own
// margin far_k |hp|_1 (far_k = 2^-8 + 2^-20, rounded up) on the box of all discs, and the slab of
// a_f - (far_k |hp|_1 - 2^-8 B), which raises the slab rule's margin from B to |hp|_1.  Spheres
// without a valid record (NaN/inf, r^2 < 2^-100, |C|_1 >= 2^30) are never culled (`always`); a
// light whose |p|^2 lies outside [2^-40, 2^40] (the analysis' range) culls nothing.
inline void build_shadow_grid(const DevLight& l, const Frame3& f, const DevSphere* sph, const DevSphereCull* cull, int S,
                       DevShadowGrid& g, unsigned long long* grid, unsigned long long* slab) {
    std::memset(&g, 0, sizeof g);
    std::memset(grid, 0, sizeof(unsigned long long) * SHGRID_N * SHGRID_N);
    std::memset(slab, 0, sizeof(unsigned long long) * (SHGRID_SLABS + 2));
    const unsigned long long all = S >= 64 ? ~0ull : ((1ull << S) - 1ull);
    g.bu0 = g.bv0 = INFINITY, g.bu1 = g.bv1 = -INFINITY;  // empty box: every far lane outside
    const bool light_ok = l.a >= 0x1p-40f && l.a <= 0x1p40f && l.a2 < INFINITY;
    std::vector<double> cu(S), cv(S), ca(S), c1(S), rr(S);
    std::vector<bool> ok(S);
    double cmax1 = 0.0;
    for (int j = 0; j < S; ++j) {
        const double c[3] = {sph[j].cx, sph[j].cy, sph[j].cz};
        c1[j] = std::fabs(c[0]) + std::fabs(c[1]) + std::fabs(c[2]);
        rr[j] = cull[j].rr;
        ok[j] = light_ok && std::isfinite(c1[j]) && c1[j] < 0x1p30 && std::isfinite(rr[j]) &&
                (double)sph[j].r2 >= 0x1p-100 && rr[j] > 0.0;
        if (!ok[j]) {
            g.always |= 1ull << j;
            continue;
        }
        cu[j] = c[0] * f.U[0] + c[1] * f.U[1] + c[2] * f.U[2];
        cv[j] = c[0] * f.V[0] + c[1] * f.V[1] + c[2] * f.V[2];
        ca[j] = c[0] * f.A[0] + c[1] * f.A[1] + c[2] * f.A[2];
        cmax1 = std::max(cmax1, c1[j]);
    }
    if (g.always == all) {  // nothing to cull: no lane looks anything up that matters
        g.bound = -1.0f;    // every lane "far"
        g.far_k = 0.0f;
        return;
    }
    const double B = std::min(std::max(8.0, 1.5 * cmax1), 0x1p30);
    g.bound = down(B);
    g.far_k = up(0x1p-8 + 0x1p-20);
    g.far_b = down(0x1p-8 * B);
    double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY, alo = INFINITY, ahi = -INFINITY;
    double bu0 = INFINITY, bu1 = -INFINITY, bv0 = INFINITY, bv1 = -INFINITY;
    std::vector<double> T(S), mB(S);
    for (int j = 0; j < S; ++j) {
        if (!ok[j]) continue;
        T[j] = rr[j] + 0x1p-8 * (c1[j] + B) + 0x1p-20 * B;
        mB[j] = 0x1p-8 * (c1[j] + B) + 0x1p-20 * B;
        ulo = std::min(ulo, cu[j] - T[j]), uhi = std::max(uhi, cu[j] + T[j]);
        vlo = std::min(vlo, cv[j] - T[j]), vhi = std::max(vhi, cv[j] + T[j]);
        alo = std::min(alo, ca[j] + mB[j]), ahi = std::max(ahi, ca[j] + mB[j]);
        const double t0 = rr[j] + 0x1p-8 * c1[j];  // far lanes add their own |hp| term
        bu0 = std::min(bu0, cu[j] - t0), bu1 = std::max(bu1, cu[j] + t0);
        bv0 = std::min(bv0, cv[j] - t0), bv1 = std::max(bv1, cv[j] + t0);
    }
    g.bu0 = down(bu0), g.bu1 = up(bu1), g.bv0 = down(bv0), g.bv1 = up(bv1);
    // grid over [lo, hi] padded by half a cell (lanes mapped outside it see no disc: checked below)
    auto axis = [](double lo, double hi, int n, float& s, float& o) {
        const double cs = (hi - lo) / (n - 1);  // n - 1 cells span the range, half a cell of pad each side
        const double lo2 = lo - 0.5 * cs;
        s = (float)(1.0 / cs);
        o = (float)(-lo2 * (double)s);
    };
    axis(ulo, uhi, SHGRID_N, g.su, g.ou);
    axis(vlo, vhi, SHGRID_N, g.sv, g.ov);
    bool sound = g.su > 0.0f && g.sv > 0.0f && std::isfinite(g.su) && std::isfinite(g.sv) && std::isfinite(g.ou) &&
                 std::isfinite(g.ov);
    // a lane mapped below cell 0 / above cell N-1 lies outside every disc
    sound = sound && cell_hi(-1, g.su, g.ou) + 0x1p-20 * B < ulo && cell_lo(SHGRID_N, g.su, g.ou) - 0x1p-20 * B > uhi &&
            cell_hi(-1, g.sv, g.ov) + 0x1p-20 * B < vlo && cell_lo(SHGRID_N, g.sv, g.ov) - 0x1p-20 * B > vhi;
    if (sound) {
        for (int iv = 0; iv < SHGRID_N; ++iv) {
            const double v0 = cell_lo(iv, g.sv, g.ov) - 0x1p-20 * B, v1 = cell_hi(iv, g.sv, g.ov) + 0x1p-20 * B;
            for (int iu = 0; iu < SHGRID_N; ++iu) {
                const double u0 = cell_lo(iu, g.su, g.ou) - 0x1p-20 * B, u1 = cell_hi(iu, g.su, g.ou) + 0x1p-20 * B;
                unsigned long long m = 0;
                for (int j = 0; j < S; ++j) {
                    if (!ok[j]) continue;
                    const double du = std::max(0.0, std::max(u0 - cu[j], cu[j] - u1));
                    const double dv = std::max(0.0, std::max(v0 - cv[j], cv[j] - v1));
                    if (du * du + dv * dv <= T[j] * T[j] * (1.0 + 0x1p-30)) m |= 1ull << j;
                }
                grid[iv * SHGRID_N + iu] = m;
            }
        }
    } else {  // (degenerate extents) every lane takes every sphere through the far path
        g.bound = -1.0f;
        g.bu0 = -INFINITY, g.bu1 = INFINITY, g.bv0 = -INFINITY, g.bv1 = INFINITY;
    }
    // axial slabs over [alo, ahi]: entry k + 1 for slab k (-1: below the range, every sphere)
    {
        const double cs = std::max((ahi - alo) / SHGRID_SLABS, 1e-30);
        g.sa = (float)(1.0 / cs);
        g.oa = (float)(-alo * (double)g.sa);
        const bool sa_ok = g.sa > 0.0f && std::isfinite(g.sa) && std::isfinite(g.oa);
        slab[0] = all;
        for (int k = 0; k <= SHGRID_SLABS; ++k) {
            const double a_lo = sa_ok ? cell_lo(k, g.sa, g.oa) : -INFINITY;
            unsigned long long m = 0;
            for (int j = 0; j < S; ++j)
                if (ok[j] && ca[j] + mB[j] > a_lo) m |= 1ull << j;
            slab[k + 1] = m;
        }
        if (!sa_ok) g.sa = 0.0f, g.oa = 0.0f;  // every lane in slab 0 (= every valid sphere)
    }
}

// The scene image of rt_set_scene's arguments (checked by the caller): the layout with host_blob the bytes to upload.
inline SceneLayout scene_build(const rt_sphere* spheres, int n_spheres, const rt_plane* planes, int n_planes,
                               const rt_light* lights, int n_lights, rt_vec3 ambient, int recursion_limit,
                               const SceneOptions& opt = SceneOptions{}) {
    SceneLayout L;
    L.S = n_spheres, L.P = n_planes, L.L = n_lights, L.limit = recursion_limit;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    // the sphere table is padded to an even count (the direct kernel's loops take spheres in
    // pairs) with a sphere that never hits: NaN centre and radius^2 make every comparison of
    // IntersectsSphere false (no candidate, t = 0, no shadow)
    const int s_pad = n_spheres + (n_spheres & 1);
    L.off_sph = 0;
    L.off_mat = al(L.off_sph + sizeof(DevSphere) * (size_t)s_pad);
    L.off_pl = al(L.off_mat + sizeof(DevMaterial) * (size_t)(n_spheres + n_planes));
    L.off_li = al(L.off_pl + sizeof(DevPlane) * (size_t)n_planes);
    L.off_cull = al(L.off_li + sizeof(DevLight) * (size_t)n_lights);
    L.off_shcull = al(L.off_cull + sizeof(DevSphereCull) * (size_t)n_spheres);
    L.has_shcull = (long long)n_lights * (long long)n_spheres <= SHADOW_CULL_MAX_ENTRIES;
    // shadow grids: the bundle kernel's merged pass only (merged_class 1 or 2, whatever the lights' 2a);
    // RT_SHADOW_GRID=0 keeps the per-level bound (A/B and fallback tests)
    L.has_shg = merged_class(n_spheres, n_lights, true) != 0 && opt.shadow_grid;
    L.off_shg = al(L.off_shcull + (L.has_shcull ? sizeof(DevShadowCull) * (size_t)n_lights * (size_t)n_spheres : 0));
    L.off_shgrid = al(L.off_shg + (L.has_shg ? sizeof(DevShadowGrid) * (size_t)n_lights : 0));
    L.off_shslab = al(L.off_shgrid + (L.has_shg ? sizeof(unsigned long long) * SHGRID_N * SHGRID_N * (size_t)n_lights : 0));
    L.off_clus = al(L.off_shslab + (L.has_shg ? sizeof(unsigned long long) * (SHGRID_SLABS + 2) * (size_t)n_lights : 0));
    // per-lane cluster pre-cull of the bundle kernel's trace bundles (CULL_MIN_SPHERES <= S <= 64);
    // RT_TRACE_CLUSTERS=0 turns it off, =2..16 sets the cluster size (A/B)
    const int csize = opt.cluster_size;
    const bool want_clus = n_spheres >= CULL_MIN_SPHERES && n_spheres <= 64 && csize >= 1;
    L.off_shpre = al(L.off_clus + (want_clus ? sizeof(DevCluster) * MAX_CLUSTERS : 0));
    // the direct kernel's shadow pre-test (S < CULL_MIN_SPHERES); RT_SHADOW_PRE=0 turns it off (A/B)
    L.has_shpre = n_spheres < CULL_MIN_SPHERES && n_lights >= 1 && opt.shadow_pre;
    // the direct kernel's mirrored screen boxes, built per view (view_mirror_boxes); RT_MIRROR_BOX=0 turns them off (A/B)
    L.mirror_box = opt.mirror_box;
    // the pre-test's group and union records, one DevShadowGroups per light; RT_SHADOW_GROUPS=0 turns them off (A/B)
    L.off_shgrp = al(L.off_shpre + (L.has_shpre ? sizeof(DevShadowCull) * (size_t)n_lights * (size_t)s_pad : 0));
    L.has_shgrp = L.has_shpre && opt.shadow_groups;
    L.bytes = al(L.off_shgrp + (L.has_shgrp ? sizeof(DevShadowGroups) * (size_t)n_lights : 0)) + 256;

    std::vector<unsigned char> blob(L.bytes, 0);
    DevSphere* sph = (DevSphere*)(blob.data() + L.off_sph);
    DevMaterial* mat = (DevMaterial*)(blob.data() + L.off_mat);
    DevPlane* pl = (DevPlane*)(blob.data() + L.off_pl);
    DevLight* li = (DevLight*)(blob.data() + L.off_li);
    DevSphereCull* cull = (DevSphereCull*)(blob.data() + L.off_cull);
    for (int i = 0; i < n_spheres; ++i) {
        const rt_sphere& s = spheres[i];
        sph[i] = DevSphere{s.center.x, s.center.y, s.center.z, s.radius * s.radius};  // :336
        mat[i] = dev_material(s.material, ambient);
        // cull radius: an upper bound of sqrt(r^2) (1 + 2^-8), rounded up (NaN stays NaN)
        const double rr = std::sqrt((double)sph[i].r2) * (1.0 + 0x1p-8);
        cull[i] = DevSphereCull{sph[i].cx, sph[i].cy, sph[i].cz, std::nextafter((float)rr, INFINITY)};
    }
    for (int i = n_spheres; i < s_pad; ++i) sph[i] = DevSphere{NAN, NAN, NAN, NAN};
    L.host_sph.assign(sph, sph + n_spheres);
    for (int i = 0; i < n_planes; ++i) {
        const rt_plane& p = planes[i];
        const H3 n = h3(p.normal);
        DevPlane d;
        std::memset(&d, 0, sizeof d);
        d.cx = p.center.x, d.cy = p.center.y, d.cz = p.center.z;
        d.cn = hdot(h3(p.center), n);  // Vector3.Dot(plane.center, plane.normal), :594
        d.nx = n.x, d.ny = n.y, d.nz = n.z;
        H3 e1 = hnormalize(hcross(n, H3{1.0f, 0.0f, 0.0f}));  // :760-763
        if (e1.x == 0 && e1.y == 0 && e1.z == 0) e1 = hnormalize(hcross(n, H3{0.0f, 0.0f, 1.0f}));
        H3 e2 = hnormalize(hcross(n, e1));  // :765
        d.e1x = e1.x, d.e1y = e1.y, d.e1z = e1.z;
        d.e2x = e2.x, d.e2y = e2.y, d.e2z = e2.z;
        pl[i] = d;
        mat[n_spheres + i] = dev_material(p.material, ambient);
    }
    L.host_pl.assign(pl, pl + n_planes);
    std::vector<Frame3> frames((size_t)n_lights);
    for (int i = 0; i < n_lights; ++i) {
        const rt_light& l = lights[i];
        const H3 p = h3(l.position);
        DevLight d;
        std::memset(&d, 0, sizeof d);
        d.px = p.x, d.py = p.y, d.pz = p.z, d.intensity = l.intensity;
        d.a = hdot(p, p);  // IntersectsSphere's a = Dot(direction, direction), :617
        d.a2 = 2.0f * d.a;
        d.a4 = 4.0f * d.a;
        d.sh_t = shadow_threshold(d.a2);  // used only when a2 is finite and > 0 (wave-uniform per light)
        if (!(d.a2 > 0.0f && d.a2 < INFINITY)) L.lights_a2_ok = false;
        // shadow-cull frame (kernel uses it only when a is in [2^-40, 2^40])
        const double len = std::sqrt((double)p.x * p.x + (double)p.y * p.y + (double)p.z * p.z);
        double A[3] = {0.0, 0.0, 1.0};
        if (len > 0 && std::isfinite(len)) A[0] = p.x / len, A[1] = p.y / len, A[2] = p.z / len;
        const double h[3] = {std::fabs(A[0]) < 0.9 ? 1.0 : 0.0, std::fabs(A[0]) < 0.9 ? 0.0 : 1.0, 0.0};
        double U[3] = {A[1] * h[2] - A[2] * h[1], A[2] * h[0] - A[0] * h[2], A[0] * h[1] - A[1] * h[0]};
        const double ul = std::sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
        for (double& c : U) c /= ul;
        const double V[3] = {A[1] * U[2] - A[2] * U[1], A[2] * U[0] - A[0] * U[2], A[0] * U[1] - A[1] * U[0]};
        d.ax = (float)A[0], d.ay = (float)A[1], d.az = (float)A[2];
        d.ux = (float)U[0], d.uy = (float)U[1], d.uz = (float)U[2];
        d.vx = (float)V[0], d.vy = (float)V[1], d.vz = (float)V[2];
        li[i] = d;
        for (int k = 0; k < 3; ++k) frames[(size_t)i].U[k] = U[k], frames[(size_t)i].V[k] = V[k], frames[(size_t)i].A[k] = A[k];
    }
    // the plane footprints of a view (rt_foot.h, built per view by view_build); RT_PRIM_FOOT=0 turns them off (A/B)
    L.prim_foot = opt.prim_foot;
    // the direct kernel's plane-uniform waves (rt_kernel.hip trace_tile_direct); RT_UNIFORM_PLANE=0 turns them off (A/B)
    L.uniform_plane = opt.uniform_plane;
    // the dark-tile skip (rt_dark.h): planes whose material and the scene's lights pass the host part of its guard;
    // RT_DARK_SKIP=0 leaves the bit clear (A/B)
    if (opt.dark_skip)
        for (int i = 0; i < n_planes; ++i)
            if (plane_dark_ok(pl[i], mat[n_spheres + i], li, n_lights)) mat[n_spheres + i].flags |= MAT_DARK_OK;
    if (L.has_shg)
        for (int j = 0; j < n_lights; ++j)
            build_shadow_grid(li[j], frames[(size_t)j], sph, cull, n_spheres, ((DevShadowGrid*)(blob.data() + L.off_shg))[j],
                              (unsigned long long*)(blob.data() + L.off_shgrid) + (size_t)j * SHGRID_N * SHGRID_N,
                              (unsigned long long*)(blob.data() + L.off_shslab) + (size_t)j * (SHGRID_SLABS + 2));
    if (want_clus) L.n_clus = build_clusters(cull, n_spheres, csize, (DevCluster*)(blob.data() + L.off_clus));
    if (L.has_shcull) build_shadow_cull(li, n_lights, cull, n_spheres, (DevShadowCull*)(blob.data() + L.off_shcull));
    if (L.has_shpre) build_shadow_pre(li, n_lights, cull, n_spheres, s_pad, (DevShadowCull*)(blob.data() + L.off_shpre));
    if (L.has_shgrp)
        build_shadow_groups((const DevShadowCull*)(blob.data() + L.off_shpre), n_lights, n_spheres, s_pad,
                            (DevShadowGroups*)(blob.data() + L.off_shgrp));
    for (int i = 0; i < n_spheres + n_planes; ++i)
        if ((mat[i].flags & MAT_SPEC) && mat[i].pow_kind == POW_GENERIC) L.generic_pow = true;
    L.host_blob = std::move(blob);
    return L;
}

// A scene track (rt_set_scene_track): the scene images of the frames of an animation, back to back at `stride` =
// the layout's bytes.  The layout -- every off_*, every has_*, bytes -- depends on the counts and the options only,
// never on values, so frame f's tables lie at frame 0's offsets inside slice f; track_build checks that instead of
// assuming it.  `common` is that layout with the launch scalars of the whole track: n_clus (equal in every frame, or
// the track is refused), lights_a2_ok the AND and generic_pow the OR over the frames -- sound because the kernels
// picked by a false lights_a2_ok test each light's 2a where they use it, and the GPOW kernels dispatch on each
// material's pow_kind (rt_kernel.hip shade_direct, shade_bundle, shadow_merged): both are exact for every frame.
// `frames` keeps per frame what view building reads (rt_view.h view_build: host_sph, host_pl, the flags, and the
// materials, as host_blob cut behind the material table); common.host_blob is empty.
struct SceneTrack {
    int n_frames = 0;
    size_t stride = 0;
    SceneLayout common;
    std::vector<SceneLayout> frames;
    std::vector<unsigned char> image;  // n_frames * stride bytes (the caller may drop it once uploaded)
};

enum : int { TRACK_OK = 0, TRACK_LAYOUT = 1, TRACK_CLUSTERS = 2 };

inline bool track_same_layout(const SceneLayout& a, const SceneLayout& b) {
    return a.S == b.S && a.P == b.P && a.L == b.L && a.limit == b.limit && a.off_sph == b.off_sph && a.off_mat == b.off_mat &&
           a.off_pl == b.off_pl && a.off_li == b.off_li && a.off_cull == b.off_cull && a.off_shcull == b.off_shcull &&
           a.bytes == b.bytes && a.off_shg == b.off_shg && a.off_shgrid == b.off_shgrid && a.off_shslab == b.off_shslab &&
           a.off_clus == b.off_clus && a.off_shpre == b.off_shpre && a.has_shpre == b.has_shpre && a.off_shgrp == b.off_shgrp &&
           a.has_shgrp == b.has_shgrp && a.mirror_box == b.mirror_box && a.prim_foot == b.prim_foot &&
           a.uniform_plane == b.uniform_plane && a.has_shcull == b.has_shcull && a.has_shg == b.has_shg;
}

// The bytes of one frame's image for these counts and options (no table is built).
inline size_t track_frame_bytes(int n_spheres, int n_planes, int n_lights, const SceneOptions& opt) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t s_pad = (size_t)n_spheres + (size_t)(n_spheres & 1), S = (size_t)n_spheres, P = (size_t)n_planes, L = (size_t)n_lights;
    size_t o = al(sizeof(DevSphere) * s_pad);
    o = al(o + sizeof(DevMaterial) * (S + P));
    o = al(o + sizeof(DevPlane) * P);
    o = al(o + sizeof(DevLight) * L);
    o = al(o + sizeof(DevSphereCull) * S);
    const bool has_shcull = (long long)n_lights * (long long)n_spheres <= SHADOW_CULL_MAX_ENTRIES;
    const bool has_shg = merged_class(n_spheres, n_lights, true) != 0 && opt.shadow_grid;
    o = al(o + (has_shcull ? sizeof(DevShadowCull) * L * S : 0));
    o = al(o + (has_shg ? sizeof(DevShadowGrid) * L : 0));
    o = al(o + (has_shg ? sizeof(unsigned long long) * SHGRID_N * SHGRID_N * L : 0));
    o = al(o + (has_shg ? sizeof(unsigned long long) * (SHGRID_SLABS + 2) * L : 0));
    const bool want_clus = n_spheres >= CULL_MIN_SPHERES && n_spheres <= 64 && opt.cluster_size >= 1;
    o = al(o + (want_clus ? sizeof(DevCluster) * MAX_CLUSTERS : 0));
    const bool has_shpre = n_spheres < CULL_MIN_SPHERES && n_lights >= 1 && opt.shadow_pre;
    o = al(o + (has_shpre ? sizeof(DevShadowCull) * L * s_pad : 0));
    return al(o + (has_shpre && opt.shadow_groups ? sizeof(DevShadowGroups) * L : 0)) + 256;
}

// The track of n_frames frames with these counts (arguments checked by the caller): frame f from spheres[f *
// n_spheres ..], planes[f * n_planes ..], lights[f * n_lights ..] and ambients[f], each through scene_build with the
// same options -- what rt_set_scene builds for that frame.  n_threads > 1: the frames are built by that many
// threads, each frame into its own slice and record (the result does not depend on n_threads).  Returns TRACK_OK,
// TRACK_LAYOUT (a frame's layout differs from frame 0's: a builder broke the rule above) or TRACK_CLUSTERS (cluster
// counts differ between frames).
inline int track_build(const rt_sphere* spheres, int n_spheres, const rt_plane* planes, int n_planes, const rt_light* lights,
                       int n_lights, const rt_vec3* ambients, int recursion_limit, int n_frames, const SceneOptions& opt,
                       int n_threads, SceneTrack* out) {
    SceneTrack& T = *out;
    T = SceneTrack{};
    T.n_frames = n_frames;
    T.stride = track_frame_bytes(n_spheres, n_planes, n_lights, opt);
    T.frames.resize((size_t)n_frames);
    T.image.resize((size_t)n_frames * T.stride);
    std::vector<char> bad((size_t)n_frames, 0);
    auto one = [&](int f) {
        SceneLayout L = scene_build(spheres + (size_t)f * (size_t)n_spheres, n_spheres, planes + (size_t)f * (size_t)n_planes,
                                    n_planes, lights + (size_t)f * (size_t)n_lights, n_lights, ambients[f], recursion_limit, opt);
        if (L.bytes != T.stride || L.host_blob.size() != L.bytes) {
            bad[(size_t)f] = 1;
        } else {
            std::memcpy(T.image.data() + (size_t)f * T.stride, L.host_blob.data(), L.bytes);
            L.host_blob.resize(L.off_mat + sizeof(DevMaterial) * (size_t)(n_spheres + n_planes));  // (view_mirror_boxes, row_order)
            L.host_blob.shrink_to_fit();
        }
        T.frames[(size_t)f] = std::move(L);
    };
    if (n_threads > n_frames) n_threads = n_frames;
    if (n_threads > 1) {
        std::vector<std::thread> pool;
        for (int t = 0; t < n_threads; ++t)
            pool.emplace_back([&, t] {
                for (int f = t; f < n_frames; f += n_threads) one(f);
            });
        for (std::thread& th : pool) th.join();
    } else {
        for (int f = 0; f < n_frames; ++f) one(f);
    }
    const SceneLayout& L0 = T.frames[0];
    bool a2 = true, gp = false;
    for (int f = 0; f < n_frames; ++f) {
        const SceneLayout& L = T.frames[(size_t)f];
        if (bad[(size_t)f] || !track_same_layout(L0, L)) return TRACK_LAYOUT;
        if (L.n_clus != L0.n_clus) return TRACK_CLUSTERS;
        a2 = a2 && L.lights_a2_ok;
        gp = gp || L.generic_pow;
    }
    SceneLayout& C = T.common;
    C = L0;
    C.host_blob.clear(), C.host_sph.clear(), C.host_pl.clear();
    C.lights_a2_ok = a2, C.generic_pow = gp;
    return TRACK_OK;
}

}  // namespace rtk
