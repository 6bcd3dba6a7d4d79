// Host check of the dark-tile skip's guard (csrc/rt_dark.h; tests/test_dark_host.py), TEST INFRASTRUCTURE ONLY.
// Built by the Makefile beside it as host C++ with ASan + UBSan and -ffp-contract=off, run as a plain executable on the CPU.
//
// The per-light term of a plane hit (RayTracer.cs ShapePhongShading :665-695 and TracePlane's addend :752-775) is
// restated here in binary32 and evaluated over a product of edge inputs.
//   1. Wherever both parts of the guard pass, max(0, term * 0) is +0 (the bit pattern) in every component, with the
//      light's intensity and with 0 (a blocked shadow ray).  The guard's precondition is the kernels' own: the hit
//      point lies within 2^-5 of the plane; the sweep offsets its points by up to that.
//   2. The guard passes for the REF / C3 and C4 planes with their lights on a 64 x 64 grid of each plane.
// Inputs the guard refuses are evaluated too and the terms that are not +0 counted: the sweep does hold inputs
// that the skip would get wrong.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_dark.h"

using namespace rtk;

namespace {

struct V3 {
    float x, y, z;
};
V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 mul(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
V3 scale(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
float dot(V3 a, V3 b) { return ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z); }  // Vector3.Dot
V3 normalize(V3 a) {  // Vector3.Normalize
    const float s = 1.0f / std::sqrt(dot(a, a));
    return scale(a, s);
}
// Math.Max(x, 0f): IEEE 754-2019 maximum (NaN propagates, -0 < +0)
float max0(float a) { return a != a ? a : (a > 0.0f ? a : 0.0f); }
bool is_zero(V3 v) { return v.x == 0 && v.y == 0 && v.z == 0; }
uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

struct Mat {
    V3 kd, ks;
    float n;
};
bool is_diffuse(const Mat& m) { return !is_zero(m.kd); }                // Material.IsDiffuse
bool has_spec(const Mat& m) { return !is_zero(m.ks) && m.n > 0.0f; }    // Material.HasSpecularity

// ShapePhongShading, :665-695
V3 phong(V3 hp, V3 d, V3 normal, const Mat& m, V3 lp) {
    const V3 ldir = normalize(sub(lp, hp));
    const V3 view = normalize(d);
    V3 diffuse{0, 0, 0};
    if (is_diffuse(m)) diffuse = scale(m.kd, max0(dot(normal, ldir)));
    V3 spec{0, 0, 0};
    if (has_spec(m)) {
        const V3 rs = sub(ldir, scale(normal, 2.0f * dot(ldir, normal)));
        const float s = dot(view, normalize(rs));
        const float p = (float)std::pow((double)max0(s), (double)m.n);
        spec = mul(m.ks, V3{p, p, p});
    }
    return add(diffuse, spec);
}
// TracePlane's addend, :752-775, for a light intensity after the shadow test and a tile colour
V3 addend(float inten, V3 hp, V3 d, float t, V3 normal, const Mat& m, V3 lp, float tile) {
    const float att = (float)(1.0 / std::pow((double)t, 2.0));
    const V3 ph = phong(hp, d, normal, m, lp);
    V3 term = mul(mul(scale(V3{inten, inten, inten}, att), ph), V3{tile, tile, tile});
    return V3{max0(term.x), max0(term.y), max0(term.z)};
}
bool plus_zero(V3 v) { return bits(v.x) == 0 && bits(v.y) == 0 && bits(v.z) == 0; }

// the device records as rt_set_scene builds them (rt_scene.h dev_material, DevPlane, DevLight)
DevMaterial dev_mat(const Mat& m) {
    DevMaterial d;
    std::memset(&d, 0, sizeof d);
    d.kd[0] = m.kd.x, d.kd[1] = m.kd.y, d.kd[2] = m.kd.z;
    d.ks[0] = m.ks.x, d.ks[1] = m.ks.y, d.ks[2] = m.ks.z;
    d.n = m.n;
    d.flags = (is_diffuse(m) ? MAT_DIFFUSE : 0u) | (has_spec(m) ? MAT_SPEC : 0u);
    return d;
}
DevPlane dev_plane(V3 c, V3 n) {
    DevPlane d;
    std::memset(&d, 0, sizeof d);
    d.cx = c.x, d.cy = c.y, d.cz = c.z;
    d.cn = dot(c, n);
    d.nx = n.x, d.ny = n.y, d.nz = n.z;
    return d;
}
DevLight dev_light(V3 p, float I) {
    DevLight d;
    std::memset(&d, 0, sizeof d);
    d.px = p.x, d.py = p.y, d.pz = p.z, d.intensity = I;
    return d;
}

// A point of the plane n.x = cn (double arithmetic, rounded once): in-plane coordinates (a, b) from the point of
// the plane nearest the origin, then `off` along the unit normal.
V3 plane_point(const DevPlane& pl, double a, double b, double off) {
    const double n[3] = {pl.nx, pl.ny, pl.nz};
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2], len = std::sqrt(nn);
    const int k = std::fabs(n[0]) < 0.9 * len ? 0 : 1;  // a helper axis not along n
    double h[3] = {0, 0, 0};
    h[k] = 1.0;
    double t1[3] = {n[1] * h[2] - n[2] * h[1], n[2] * h[0] - n[0] * h[2], n[0] * h[1] - n[1] * h[0]};
    const double l1 = std::sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
    for (double& c : t1) c /= l1;
    const double t2[3] = {(n[1] * t1[2] - n[2] * t1[1]) / len, (n[2] * t1[0] - n[0] * t1[2]) / len,
                          (n[0] * t1[1] - n[1] * t1[0]) / len};
    const double base = (double)pl.cn / nn;
    double p[3];
    for (int i = 0; i < 3; ++i) p[i] = base * n[i] + a * t1[i] + b * t2[i] + off * n[i] / len;
    return V3{(float)p[0], (float)p[1], (float)p[2]};
}

int failures = 0;
void fail(const char* what) {
    if (++failures <= 20) std::printf("FAIL: %s\n", what);
}

struct Lane {
    V3 hp, d;
    float t;
    bool ok;
};

}  // namespace

int main() {
    const float INF = INFINITY, QNAN = NAN;
    // ---- the sweep's factors -------------------------------------------------------------------------------
    std::vector<V3> normals;
    normals.push_back(V3{0, 1, 0});
    {
        const V3 g = normalize(V3{0.2f, 1.0f, -0.1f});  // a general unit normal
        normals.push_back(g);
        // |n|^2 inside, at both sides of, and outside the 2^-10 band, shorter and longer than unit length
        for (double dl : {0x1p-11, 0.99 * 0x1p-10, 1.0 * 0x1p-10, 1.01 * 0x1p-10, 0x1p-9})
            for (double sg : {-1.0, 1.0}) normals.push_back(V3{0, (float)std::sqrt(1.0 + sg * dl), 0});
        normals.push_back(scale(g, (float)std::sqrt(1.0 - 0x1p-11)));
        // |n|^2 = 0.5: a light along the normal has rs = 0 (exactly, with these components) and normalize(rs) NaN
        normals.push_back(V3{0.5f, 0.5f, 0});
        normals.push_back(V3{0, (float)std::sqrt(0.5), 0});
        normals.push_back(V3{0, 1.01f, 0});
    }
    const float Is[] = {1.0f, -1.0f, 0x1p59f, 0x1p60f, 3e38f, INF, QNAN};
    const float Ks[] = {0.0f, 1.0f, 0x1p19f, 0x1p20f, 1e30f, INF, QNAN};
    const float Ns[] = {0.5f, 1.0f, 2.0f, 3.7f, 1024.0f, 1e6f, 0.0f, -1.0f, QNAN};
    const float Ts[] = {0.0100001f, 1.0f, 4095.0f, 4096.0f, 1e6f, INF, QNAN, 0.005f, 0.0f, -1.0f};
    std::vector<V3> dirs;
    {
        const V3 u = normalize(V3{0.3f, -0.5f, 0.8f});
        for (float s : {1.0f, 0.4f, 2.1f, 0.5f, 1.99f, 0.0f}) dirs.push_back(scale(u, s));
        dirs.push_back(V3{0.6f, QNAN, 0.8f});
        dirs.push_back(V3{0.0f, -1.0f, 0.0f});  // along the floor's normal
    }
    const double ABs[][2] = {{0, 0}, {0.5, 4.5}, {-63.5, 64}, {3, -3}, {4000, -4000}, {4096, 0}, {1e9, 3}, {-3, 1e9}};
    const double OFFs[] = {0.0, 0.99 * 0x1p-5, -0.99 * 0x1p-5};

    long checked = 0, refused_nonzero = 0, accepted_hosts = 0, hosts = 0;
    for (const V3& n : normals) {
        const DevPlane pl = dev_plane(V3{0, -1, 0}, n);
        // hit points: on the plane and within 2^-5 of it
        std::vector<V3> hps;
        for (const auto& ab : ABs)
            for (double off : OFFs) hps.push_back(plane_point(pl, ab[0], ab[1], off));
        // lights: above the plane, on it, at a hit point, above a hit point along the normal, |pos| = 2^12, and
        // at and just below the guard's clearance
        std::vector<V3> lps = {V3{-3, 1, -3},
                               V3{33, 1, 10},
                               plane_point(pl, 2, 5, 0),
                               hps[3],
                               plane_point(pl, 0.5, 4.5, 2.0),
                               plane_point(pl, 4.5, 0, 2.0),
                               V3{4096, 1, 0},
                               plane_point(pl, 1, 3, 0x1p-3 * 1.001),
                               plane_point(pl, 1, 3, 0x1p-3 * 0.96),
                               plane_point(pl, 1, 3, -0x1p-3 * 1.001)};
        hps.push_back(plane_point(pl, 0.5, 4.5, 0));  // (under the lights along the normal)
        hps.push_back(plane_point(pl, 4.5, 0, 0));
        std::vector<Lane> lanes;
        for (const V3& hp : hps)
            for (const V3& d : dirs)
                for (float t : Ts) lanes.push_back(Lane{hp, d, t, dark_lane_ok(hp.x, hp.y, hp.z, t, dot(d, d), 0.0f)});
        for (const V3& lp : lps)
            for (float I : Is)
                for (float kd : Ks)
                    for (float ks : Ks)
                        for (float ex : Ns) {
                            const Mat m{V3{1, kd, 1}, V3{0, ks, 0}, ex};
                            const DevMaterial dm = dev_mat(m);
                            const DevLight dl = dev_light(lp, I);
                            const bool host_ok = plane_dark_ok(pl, dm, &dl, 1);
                            ++hosts;
                            accepted_hosts += host_ok;
                            // refused inputs: a sample of them (every 509th lane input), to count the terms the
                            // skip would get wrong
                            const size_t phase = (size_t)hosts % 509;
                            for (size_t li = host_ok ? 0 : phase; li < lanes.size(); li += host_ok ? 1 : 509) {
                                const Lane& ln = lanes[li];
                                const bool pass = host_ok && ln.ok;
                                if (!pass && li % 509 != phase) continue;
                                bool zero = true;
                                for (float inten : {I, 0.0f})
                                    zero = zero && plus_zero(addend(inten, ln.hp, ln.d, ln.t, n, m, lp, 0.0f));
                                if (pass) {
                                    ++checked;
                                    if (!zero) {
                                        char msg[400];
                                        std::snprintf(msg, sizeof msg,
                                                      "guard passed, term not +0: n (%a %a %a) lp (%a %a %a) I %a kd %a ks %a "
                                                      "ex %a hp (%a %a %a) d (%a %a %a) t %a",
                                                      n.x, n.y, n.z, lp.x, lp.y, lp.z, I, kd, ks, ex, ln.hp.x, ln.hp.y, ln.hp.z,
                                                      ln.d.x, ln.d.y, ln.d.z, ln.t);
                                        fail(msg);
                                    }
                                } else if (!zero) {
                                    ++refused_nonzero;
                                }
                            }
                        }
    }
    // the host part looks at every light: a good light beside a bad one
    {
        const DevPlane pl = dev_plane(V3{0, -1, 0}, V3{0, 1, 0});
        const DevMaterial dm = dev_mat(Mat{V3{1, 1, 1}, V3{1, 1, 1}, 0.5f});
        const DevLight two[2] = {dev_light(V3{-3, 1, -3}, 1.0f), dev_light(V3{2, -1, 5}, 1.0f)};
        if (!plane_dark_ok(pl, dm, two, 1)) fail("one good light refused");
        if (plane_dark_ok(pl, dm, two, 2)) fail("a light on the plane accepted as the second light");
        if (!plane_dark_ok(pl, dm, two, 0)) fail("no lights refused");
        if (dark_lane_ok(1, -1, 2, 3.0f, 1.0f, 1.0f)) fail("a lit square passed the lane part");
        if (!dark_lane_ok(1, -1, 2, 3.0f, 1.0f, 0.0f)) fail("a plain dark hit refused by the lane part");
    }

    // ---- 2. the guard passes on the scenes it is meant for ---------------------------------------------------
    const Mat floor_mat{V3{1, 1, 1}, V3{1, 1, 1}, 0.5f}, wall_mat{V3{0.6f, 0.6f, 0.6f}, V3{0, 0, 0}, 0.0f};
    const DevLight ref_lights[2] = {dev_light(V3{-3, 1, -3}, 1.0f), dev_light(V3{33, 1, 10}, 1.0f)};
    const DevLight c4_lights[4] = {ref_lights[0], ref_lights[1], dev_light(V3{0, 12, 4}, 1.0f),
                                   dev_light(V3{-20, 6, 30}, 0.8f)};
    struct Case {
        const char* name;
        DevPlane pl;
        Mat m;
        const DevLight* li;
        int L;
    };
    const Case cases[] = {{"REF / C3 floor", dev_plane(V3{0, -1, 0}, V3{0, 1, 0}), floor_mat, ref_lights, 2},
                          {"C4 floor", dev_plane(V3{0, -1, 0}, V3{0, 1, 0}), floor_mat, c4_lights, 4},
                          {"C4 wall", dev_plane(V3{0, 0, 48}, V3{0, 0, -1}), wall_mat, c4_lights, 4}};
    long grid_pass = 0;
    for (const Case& c : cases) {
        const DevMaterial dm = dev_mat(c.m);
        if (!plane_dark_ok(c.pl, dm, c.li, c.L)) {
            fail(c.name);
            continue;
        }
        for (int i = 0; i < 64; ++i)
            for (int j = 0; j < 64; ++j) {
                const V3 hp = plane_point(c.pl, -64.0 + 128.0 * i / 63.0, -64.0 + 128.0 * j / 63.0, 0.0);
                const float t = std::sqrt(dot(hp, hp));  // from a camera at the origin along a unit direction
                const V3 d = normalize(hp);
                if (dark_lane_ok(hp.x, hp.y, hp.z, t, dot(d, d), 0.0f)) ++grid_pass;
                else fail(c.name);
            }
    }

    std::printf("dark_host: %ld host inputs, %ld accepted, %ld terms checked, %ld refused terms not +0\n", hosts,
                accepted_hosts, checked, refused_nonzero);
    std::printf("dark_host: grid %ld of %d passed\n", grid_pass, 3 * 64 * 64);
    std::printf("dark_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
