// rt_view.h -- everything of a view that depends on the camera, built on the host: the camera basis and view plane
// (camera_view), the spheres' screen boxes (prim_box), the mirrored boxes (mirror_boxes), the plane footprints
// (rt_foot.h), the tile-row and tile orders of a lone frame, the DevView record of a camera-path frame and the
// view-plane tables.  Device-free, like rt_scene.h: rt_api.cpp caches and uploads what these return, and the host
// programs under tests/native check the same functions against the oracle.  Built without FMA contraction.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/raytracer_hip.h"
#include "rt_foot.h"
#include "rt_internal.h"
#include "rt_scene.h"

namespace rtk {

// CameraForwardDirection / CameraRightDirection / CameraUpDirection (RayTracer.cs:511-523):
// double trig of the float yaw/pitch, each component cast to float; Up = Cross(Right, Fwd).
// View params (Tick, :892-896): planeHeight = 0.3f * (float)Math.Tan(30f * (MathF.PI/180f)) * 2,
// planeWidth = planeHeight * ((float)width / height).
// The ABI's rt_camera_view checks its arguments and calls this; width, height > 0 (else RT_ERR_INVALID_ARG).
inline int camera_view(const rt_camera& c, int width, int height, rt_view* out) {
    if (width <= 0 || height <= 0) return RT_ERR_INVALID_ARG;
    const double p = (double)c.pitch, y = (double)c.yaw;
    const H3 f{(float)(std::cos(p) * std::sin(y)), (float)-std::sin(p), (float)(std::cos(p) * std::cos(y))};
    const H3 r{(float)std::cos(y), 0.0f, (float)-std::sin(y)};
    const H3 u = hcross(r, f);
    out->position = c.position;
    out->right = rt_vec3{r.x, r.y, r.z};
    out->up = rt_vec3{u.x, u.y, u.z};
    out->forward = rt_vec3{f.x, f.y, f.z};
    const float near_clip = 0.3f, fov = 60.0f;
    const float deg2rad = (float)M_PI / 180.0f;  // MathHelper.DegreesToRadians: d * (MathF.PI / 180f)
    const float rad = (fov * 0.5f) * deg2rad;
    const float plane_height = near_clip * (float)std::tan((double)rad) * 2;
    const float aspect = (float)width / (float)height;
    out->plane_width = plane_height * aspect;
    out->plane_height = plane_height;
    out->near_clip = near_clip;
    return RT_OK;
}

// Conservative screen box of a sphere for primary rays (culling only; computed in double).
//
// Pixel (x, y) traces the line from the camera along D = R lx + U ly + F lz with
// lx = (x/W - 0.5) pw, ly = (y/H - 0.5) ph, lz = near (TracePixel :963-971).  By the
// cull_mask analysis the binary32 IntersectsSphere cannot select the sphere when that line
// passes at distance >= rho = r (1 + 2^-8) + 2^-8 |u| from its centre (u = C - camera), with
// |u| also scaled by the kernel's direction error (cancellation in vp - cam, bounded by
// 2^-20 (|cam| + |D|) / |D|; no box when that exceeds 2^-12).  The distance to the line is at
// least the distance to the plane through it containing the camera's up (right) axis, so
// in camera coordinates (cx, cy, cz) the x range follows from the 2-D circle (cx, cz; rho):
// lx / lz in [tan(phi - g), tan(phi + g)], phi = atan2(cx, cz), g = asin(rho / |(cx, cz)|),
// valid when cz > rho (sphere strictly in front); same for y with (cy, cz).  Two pixels of
// slack cover the binary32 pixel-to-direction mapping and the basis' non-orthogonality.
// extra: added to rho (the mirrored boxes' allowances, mirror_boxes; 0 for the primary boxes).
inline PrimBox prim_box(const LaunchParams& lp, const DevSphere& s, double extra = 0.0) {
    const PrimBox all{INT_MIN / 2, INT_MAX / 2, INT_MIN / 2, INT_MAX / 2};
    const double pw = lp.pw, ph = lp.ph, lz = lp.nearc;
    if (!(pw > 0) || !(ph > 0) || !(lz > 0) || !std::isfinite(pw) || !std::isfinite(ph) || !std::isfinite(lz))
        return all;
    const double cam[3] = {lp.cam[0], lp.cam[1], lp.cam[2]};
    const double u[3] = {s.cx - cam[0], s.cy - cam[1], s.cz - cam[2]};
    auto dot3 = [](const double* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double ulen = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double camlen = std::sqrt(cam[0] * cam[0] + cam[1] * cam[1] + cam[2] * cam[2]);
    const double dmax = std::sqrt(0.25 * pw * pw + 0.25 * ph * ph + lz * lz);
    const double dir_err = 0x1p-20 * (camlen + dmax) / lz + 0x1p-20;
    const double r = std::sqrt((double)s.r2);
    if (!std::isfinite(ulen) || !std::isfinite(r) || !(dir_err <= 0x1p-12)) return all;
    const double rho = (r * (1.0 + 0x1p-8) + (0x1p-8 + 0x1p-20 + dir_err) * ulen) * (1.0 + 0x1p-16) + 0x1p-60 + extra;
    auto fdot = [](const float* a, const float* b) { return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]; };
    const double ortho = std::fabs(fdot(lp.right, lp.up)) + std::fabs(fdot(lp.right, lp.fwd)) +
                         std::fabs(fdot(lp.up, lp.fwd)) + std::fabs(fdot(lp.right, lp.right) - 1.0) +
                         std::fabs(fdot(lp.up, lp.up) - 1.0) + std::fabs(fdot(lp.fwd, lp.fwd) - 1.0);
    if (!(ortho < 0x1p-18)) return all;  // the camera basis is orthonormal up to rounding
    const double cx = dot3(u, lp.right), cy = dot3(u, lp.up), cz = dot3(u, lp.fwd);
    if (!(cz > rho * (1.0 + 0x1p-10))) return all;
    auto range = [&](double c, double plane, int n, int& lo, int& hi) {
        const double phi = std::atan2(c, cz);
        const double g = std::asin(std::min(1.0, rho / std::sqrt(c * c + cz * cz)));
        const double tlo = std::tan(phi - g), thi = std::tan(phi + g);
        const double flo = n * (0.5 + lz * tlo / plane), fhi = n * (0.5 + lz * thi / plane);
        if (!std::isfinite(flo) || !std::isfinite(fhi)) {
            lo = INT_MIN / 2, hi = INT_MAX / 2;
            return;
        }
        lo = (int)std::max(-1e9, std::floor(flo) - 2.0);
        hi = (int)std::min(1e9, std::ceil(fhi) + 2.0);
    };
    PrimBox b;
    range(cx, pw, lp.W, b.x0, b.x1);
    range(cy, ph, lp.H, b.y0, b.y1);
    return b;
}

// Mirrored screen boxes (LaunchParams::mbox; the direct kernel's first reflected segment; culling only).
//
// A ray reflected by the plane q = {x : n.x = cn} extends backwards through the camera's mirror image, so the
// reflected line of pixel (x, y) passes sphere i (centre C) at the distance at which the pixel's primary line,
// continued through q, passes the mirrored centre C' = C - 2 n (n.C - cn) / n.n.  The box is prim_box of (C', r)
// with rho grown by `extra`, which covers what the binary32 chain adds between the two lines for a lane whose
// primary hit on q has t <= t_max (eps = 2^-24, E the camera, |d| <= 1 + 2^-20, U = |E| + |cn| / |n| + 2 t_max):
//   * hp = fl(E + fl(d t)) lies within dh = 4 eps U of the primary line (two roundings per component);
//   * hp lies within dp = 16 eps U + dh of q: with t = fl(num_f / den_f), n.(E + d t) - cn = t (den - den_f) +
//     (num_f - num) + the quotient's rounding t eps den_f exactly (no first-order step: a grazing den does not
//     matter), num_f and den_f each three products and three sums of terms bounded by |E| |n| + |cn| and |d| |n|;
//     mirroring about the plane through hp instead of q moves C' by 2 dp;
//   * the binary32 reflection d' = fl(d - n fl(2 fl(d.n))) mirrored back differs from d by at most
//     2 |n.n - 1| + 12 eps <= 2^-18 (the reference reflects about the raw normal: |n.n - 1| <= 2^-20 is required),
//     an angle below 2^-16, which moves the line by at most 2^-16 |C' - hp| at C';
//   * the cull rule itself (rt_kernel.hip, "Wave-level ray bundles": not selectable when the line passes C at
//     r (1 + 2^-8) + 2^-8 |C - hp| or more) asks for 2^-8 |C - hp|, and |C - hp| <= |C' - E| + |hp - E| + 2 dp
//     with |hp - E| <= 1.001 t_max; prim_box supplies the 2^-8 |C' - E| part.
// t_max = MIRROR_TMAX_FACTOR max_i (|C'_i - E| + r_i): the 2^-8 t_max term grows every box in proportion to t_max,
// while the lanes beyond it (full test) lie within atan(h / t_max) of the plane's horizon, in inverse proportion.
// A host model of C3's 1080p frame (8x8 tiles, these boxes) counts the sphere pairs a wave's first reflected
// segment runs, 4 without boxes: 0.92 at factor 0.5, 0.78 at 1, 0.75 at 1.5 and at 2, 0.78 at 3, 0.83 at 4, 0.99
// at 8 -- a flat optimum; 2 (two tile rows under the horizon take the full test, rho grows by 0.8 % of the
// farthest mirrored sphere's distance).  No table (the plane's lanes take every sphere) when |n.n - 1| > 2^-20, an input is not finite, or
// no sphere has a usable record; a sphere with r^2 < 2^-100 or |C' - E| + t_max > 2^40 keeps the box "all" (the
// cull rule's own domain), as does one that fails prim_box's preconditions.
// margins = false (the host check's teeth, tests/native/mirror_box_host.cpp): extra = 0 and no t_max.
constexpr double MIRROR_TMAX_FACTOR = 2.0;
inline bool mirror_boxes(const LaunchParams& lp, const DevPlane& q, const std::vector<DevSphere>& sph, PrimBox* box,
                  float* t_max_out, bool margins = true, double tmax_factor = MIRROR_TMAX_FACTOR) {
    const PrimBox all{INT_MIN / 2, INT_MAX / 2, INT_MIN / 2, INT_MAX / 2};
    const size_t S = sph.size();
    for (size_t i = 0; i < S; ++i) box[i] = all;
    const double n[3] = {q.nx, q.ny, q.nz}, E[3] = {lp.cam[0], lp.cam[1], lp.cam[2]}, cn = q.cn;
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    if (!(std::fabs(nn - 1.0) <= 0x1p-20) || !std::isfinite(cn)) return false;
    const double elen = std::sqrt(E[0] * E[0] + E[1] * E[1] + E[2] * E[2]);
    if (!std::isfinite(elen)) return false;
    std::vector<DevSphere> mir(S);
    std::vector<double> ulen(S);
    double far = 0.0;
    for (size_t i = 0; i < S; ++i) {
        const double C[3] = {sph[i].cx, sph[i].cy, sph[i].cz};
        const double k = 2.0 * (n[0] * C[0] + n[1] * C[1] + n[2] * C[2] - cn) / nn;
        const double M[3] = {C[0] - k * n[0], C[1] - k * n[1], C[2] - k * n[2]};
        // the mirrored centre as floats (prim_box reads a DevSphere); its rounding, <= 2 eps |C'|, goes into extra
        mir[i] = DevSphere{(float)M[0], (float)M[1], (float)M[2], sph[i].r2};
        const double u[3] = {M[0] - E[0], M[1] - E[1], M[2] - E[2]};
        ulen[i] = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        const double reach = ulen[i] + std::sqrt((double)sph[i].r2);
        if (std::isfinite(reach)) far = std::max(far, reach);
    }
    const double t_max = margins ? tmax_factor * far : (double)INFINITY;
    if (margins && !(t_max > 0.0 && t_max <= 0x1p40)) return false;
    const double eps = 0x1p-24;
    const double U = elen + std::fabs(cn) / std::sqrt(nn) + 2.0 * t_max;
    const double dh = 4.0 * eps * U, dp = 16.0 * eps * U + dh;
    for (size_t i = 0; i < S; ++i) {
        if (!std::isfinite(ulen[i]) || !(sph[i].r2 >= 0x1p-100f)) continue;
        double extra = 0.0;
        if (margins) {
            if (!(ulen[i] + t_max <= 0x1p40)) continue;
            const double mlen = std::sqrt((double)mir[i].cx * mir[i].cx + (double)mir[i].cy * mir[i].cy + (double)mir[i].cz * mir[i].cz);
            extra = 0x1p-8 * (1.001 * t_max + 2.0 * dp) + dh + 2.0 * dp + 0x1p-16 * (ulen[i] + 1.001 * t_max + 2.0 * dp) +
                    2.0 * eps * mlen * (1.0 + 0x1p-8);
            extra *= 1.0 + 0x1p-10;
        }
        box[i] = prim_box(lp, mir[i], extra);
    }
    // (the largest float not above t_max: a lane compares its binary32 t against it)
    float tm = margins ? (float)t_max : INFINITY;
    if (margins && (double)tm > t_max) tm = std::nextafter(tm, 0.0f);
    *t_max_out = tm;
    return true;
}

// The tables of a view: the first MIRROR_BOX_PLANES planes with a mirror material, those whose table can be built.
inline void view_mirror_boxes(LaunchParams& lp, const SceneLayout& L) {
    lp.mbox_n = 0;
    for (int k = 0; k < MIRROR_BOX_PLANES; ++k) {
        lp.mbox_plane[k] = -1, lp.mbox_tmax[k] = 0.0f;
        for (int i = 0; i < CULL_MIN_SPHERES; ++i) lp.mbox[k][i] = PrimBox{INT_MIN / 2, INT_MAX / 2, INT_MIN / 2, INT_MAX / 2};
    }
    if (!L.mirror_box || !lp.prim_const || L.S < 1 || L.S >= CULL_MIN_SPHERES || L.limit < 1) return;
    if (L.host_blob.size() < L.off_mat + sizeof(DevMaterial) * (size_t)(L.S + L.P)) return;
    const DevMaterial* mat = (const DevMaterial*)(L.host_blob.data() + L.off_mat);
    int mirrors = 0;
    for (int j = 0; j < L.P && mirrors < MIRROR_BOX_PLANES; ++j) {
        if (!(mat[L.S + j].flags & MAT_MIRROR)) continue;
        ++mirrors;
        const int k = lp.mbox_n;
        if (mirror_boxes(lp, L.host_pl[(size_t)j], L.host_sph, lp.mbox[k], &lp.mbox_tmax[k])) {
            lp.mbox_plane[k] = j;
            ++lp.mbox_n;
        }
    }
}

// Order of a single-frame launch's tile rows (LaunchParams::row_order). The launch's last waves set
// its tail, so the expensive rows should start first and the cheap ones come last.  A tile row's cost
// is estimated from eight primary rays through its middle pixel row: 1 for a ray that meets nothing,
// 1 + L when it meets a plane in front of the camera or falls inside a diffuse sphere's screen box
// (prim_box: shaded, with shadow rays), (1 + L)(1 + min(limit, 4)) inside a mirror sphere's box (its
// reflected chain is shaded too).  Rows are sorted by decreasing estimate, ties in natural order.
// The estimate only orders the workgroups: every tile is traced exactly as before.
inline int row_order(const LaunchParams& lp, const SceneLayout& L, uint16_t* order) {
    const int rows = (lp.H + 7) / 8;
    if (rows < 2 || rows > ROW_ORDER_MAX) return 0;
    const DevMaterial* mat = L.host_blob.size() >= L.off_mat + sizeof(DevMaterial) * (size_t)(L.S + L.P)
                                 ? (const DevMaterial*)(L.host_blob.data() + L.off_mat)
                                 : nullptr;
    const double shade = 1.0 + L.L, mirror = shade * (1.0 + std::min(L.limit, 4));
    std::vector<double> cost((size_t)rows, 0.0);
    for (int r = 0; r < rows; ++r) {
        const int y = std::min(lp.H - 1, r * 8 + 4);
        const double ly = ((double)y / lp.H - 0.5) * lp.ph;
        for (int j = 0; j < 8; ++j) {
            const int x = (int)(((2 * j + 1) * (long long)lp.W) / 16);
            const double lx = ((double)x / lp.W - 0.5) * lp.pw;
            double d[3];
            for (int k = 0; k < 3; ++k) d[k] = lp.right[k] * lx + lp.up[k] * ly + lp.fwd[k] * lp.nearc;
            double w = 1.0;
            for (const DevPlane& q : L.host_pl) {
                const double den = d[0] * q.nx + d[1] * q.ny + d[2] * q.nz;
                const double num = q.cn - (lp.cam[0] * q.nx + lp.cam[1] * q.ny + lp.cam[2] * q.nz);
                if (den != 0 && num / den > 0) w = std::max(w, shade);
            }
            if (lp.prim_const)
                for (int i = 0; i < L.S; ++i)
                    if (x >= lp.pbox[i].x0 && x <= lp.pbox[i].x1 && y >= lp.pbox[i].y0 && y <= lp.pbox[i].y1)
                        w = std::max(w, mat && (mat[i].flags & MAT_MIRROR) ? mirror : shade);
            cost[(size_t)r] += w;
        }
    }
    std::vector<int> idx((size_t)rows);
    for (int r = 0; r < rows; ++r) idx[(size_t)r] = r;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return cost[(size_t)a] > cost[(size_t)b]; });
    for (int r = 0; r < rows; ++r) order[r] = (uint16_t)idx[(size_t)r];
    return rows;
}

inline void copy_view(const LaunchParams& from, LaunchParams& to) {
    std::memcpy(to.cam, from.cam, sizeof to.cam);
    std::memcpy(to.right, from.right, sizeof to.right);
    std::memcpy(to.up, from.up, sizeof to.up);
    std::memcpy(to.fwd, from.fwd, sizeof to.fwd);
    to.pw = from.pw, to.ph = from.ph, to.nearc = from.nearc;
    to.W = from.W, to.H = from.H;
    to.prim_const = from.prim_const;
    std::memcpy(to.pc, from.pc, sizeof to.pc);
    std::memcpy(to.pbox, from.pbox, sizeof to.pbox);
    to.mbox_n = from.mbox_n;
    std::memcpy(to.mbox_plane, from.mbox_plane, sizeof to.mbox_plane);
    std::memcpy(to.mbox_tmax, from.mbox_tmax, sizeof to.mbox_tmax);
    std::memcpy(to.mbox, from.mbox, sizeof to.mbox);
    to.foot_n = from.foot_n;
    std::memcpy(to.foot, from.foot, sizeof to.foot);
    to.row_order_n = from.row_order_n;
    to.col_major = from.col_major;
    std::memcpy(to.row_order, from.row_order, sizeof(uint16_t) * (size_t)from.row_order_n);
}

// Everything of a W x VH view that depends on the camera, into the view part of lp: position and basis, the
// view plane (pw, ph, nearc: the same for every camera of one frame size), lp.W / lp.H = the view's size, the
// primary constants and screen boxes (prim_box), the mirrored boxes (view_mirror_boxes) and the plane footprints
// (rt_foot.h foot_build; a DevView record carries none: view_record).  view_params (the
// context's camera, by value in the kernarg block) and the camera-path calls (one DevView per frame,
// view_record) both build their views here, so a path frame carries the values a one-camera launch would.
// Returns RT_ERR_INVALID_ARG for a frame size that is not positive (the only failure), else RT_OK.
inline int view_build(const SceneLayout& L, const rt_camera& cam, int W, int VH, LaunchParams& lp) {
    rt_view v;
    const int rc = camera_view(cam, W, VH, &v);
    if (rc != RT_OK) return rc;
    lp.cam[0] = v.position.x, lp.cam[1] = v.position.y, lp.cam[2] = v.position.z;
    lp.right[0] = v.right.x, lp.right[1] = v.right.y, lp.right[2] = v.right.z;
    lp.up[0] = v.up.x, lp.up[1] = v.up.y, lp.up[2] = v.up.z;
    lp.fwd[0] = v.forward.x, lp.fwd[1] = v.forward.y, lp.fwd[2] = v.forward.z;
    lp.pw = v.plane_width, lp.ph = v.plane_height, lp.nearc = v.near_clip;
    lp.W = W, lp.H = VH;  // (the screen boxes and the row order in the view's pixels)
    // primary-segment sphere constants (origin = camera for every pixel)
    const std::vector<DevSphere>& sph = L.host_sph;
    lp.prim_const = sph.size() <= (size_t)MAX_PRIM_CONST ? 1 : 0;
    if (lp.prim_const)
        for (size_t i = 0; i < sph.size(); ++i) {
            const H3 oc{lp.cam[0] - sph[i].cx, lp.cam[1] - sph[i].cy, lp.cam[2] - sph[i].cz};
            lp.pc[i] = PrimConst{oc.x, oc.y, oc.z, hdot(oc, oc) - sph[i].r2};
            lp.pbox[i] = prim_box(lp, sph[i]);
        }
    view_mirror_boxes(lp, L);  // (lp.H = VH: in the view's pixels, like pbox)
    // plane footprints (rt_foot.h): with the screen boxes they tell a wave that no primary ray of its tile hits anything
    const std::vector<DevPlane>& pl = L.host_pl;
    std::memset(lp.foot, 0, sizeof lp.foot);
    lp.foot_n = L.prim_foot && lp.prim_const && pl.size() <= (size_t)FOOT_MAX
                    ? foot_build(lp, pl.data(), (int)pl.size(), lp.foot)
                    : -1;
    return RT_OK;
}

// The DevView record of a view built by view_build (padding zeroed: records compare bytewise).
inline void view_record(const LaunchParams& lp, DevView& v) {
    std::memset(&v, 0, sizeof v);
    std::memcpy(v.cam, lp.cam, sizeof v.cam);
    std::memcpy(v.right, lp.right, sizeof v.right);
    std::memcpy(v.up, lp.up, sizeof v.up);
    std::memcpy(v.fwd, lp.fwd, sizeof v.fwd);
    v.prim_const = lp.prim_const;
    v.mbox_n = lp.mbox_n;
    std::memcpy(v.mbox_plane, lp.mbox_plane, sizeof v.mbox_plane);
    std::memcpy(v.mbox_tmax, lp.mbox_tmax, sizeof v.mbox_tmax);
    std::memcpy(v.pc, lp.pc, sizeof v.pc);
    std::memcpy(v.pbox, lp.pbox, sizeof v.pbox);
    std::memcpy(v.mbox, lp.mbox, sizeof v.mbox);
}

// Per-column / per-row view-plane coordinates of TracePixel (:963-965), computed with the
// same binary32 operations as the kernel would (-ffp-contract=off, correctly rounded
// division): lx[x] = ((float)x / W - 0.5f) * pw, ly[y] = ((float)y / H - 0.5f) * ph.
// out: lx[0..W) then ly[0..VH).
// (one entry: column or row i of n across a view plane `plane` wide or high -- rt_pick's pixel needs no table)
inline float view_table_value(int i, int n, float plane) {
    const float p = (float)i / (float)n - 0.5f;
    return p * plane;
}
inline void view_table_values(int W, int VH, float pw, float ph, float* out) {
    for (int x = 0; x < W; ++x) out[(size_t)x] = view_table_value(x, W, pw);
    for (int y = 0; y < VH; ++y) out[(size_t)W + (size_t)y] = view_table_value(y, VH, ph);
}

// The measured tile order: tiles 0..n-1 (row-major, tx per row) by decreasing cost, ties in natural order, as
// ty << 16 | tx entries.  A stable counting sort in 16-tick (160 ns) buckets (wider ones past 2^20 ticks): linear
// in the tile count -- an 8K frame's 518,400 tiles sort in a few ms, once per measuring round.
inline void tiles_by_cost(const uint32_t* cost, size_t n, uint32_t tx, uint32_t* order) {
    uint32_t cmax = 0;
    for (size_t i = 0; i < n; ++i) cmax = std::max(cmax, cost[i]);
    const int shift = cmax >> 4 < (1u << 16) ? 4 : 4 + (32 - __builtin_clz(cmax >> 20 | 1u));
    const size_t nb = (size_t)(cmax >> shift) + 1;
    std::vector<uint32_t> start(nb + 1, 0);
    for (size_t i = 0; i < n; ++i) start[nb - (cost[i] >> shift)]++;  // bucket 0 = the longest
    for (size_t b = 1; b <= nb; ++b) start[b] += start[b - 1];
    for (size_t i = 0; i < n; ++i) {
        const uint32_t t = (uint32_t)i;
        order[start[nb - 1 - (cost[i] >> shift)]++] = (t / tx) << 16 | (t % tx);
    }
}

}  // namespace rtk
