// shadow_group_host.cpp -- host check of the shadow pre-test's group and union records (csrc/rt_scene.h
// build_shadow_groups, DevShadowGroups), TEST INFRASTRUCTURE ONLY.  Plain host C++ against the library's device-free
// builder (rt_scene.h scene_build) and the kernels' own pre-test (rt_shadow_pre.h shadow_pre_lane / shadow_pre_keep /
// shadow_pre_widen) under ASan + UBSan; no device code is compiled or linked.
//
// Scenes: C1-C3, REF, C4's first 11 spheres; 3000 seeded random scenes of 0-11 spheres and 1-4 lights over the scales
// 1e-3, 1, 30 and 1000; degenerate ones (coincident spheres, spheres 2^30 apart, NaN and tiny radii, a centre with
// |C_f|_1 >= 2^38, lights with a = p.p outside [2^-40, 2^40] and at the origin, odd counts).
//
// Structure, per scene and light: the groups' masks are disjoint and cover exactly the spheres 0..S-1 (never the
// padding sphere), a group without members has the never-kept record, a member without a usable record makes its group
// and the union +inf, and RT_SHADOW_GROUPS=0 (SceneOptions::shadow_groups) leaves the layout without records.
//
// Implication, in binary32 with the kernel's functions, for every sampled lane record q, light, group and member:
//     keep(q, member) => keep(widen(q, GROUP), group) => keep(widen(q, UNION), union)
// Samples: hit points at scales 2^-10..2^40 through the light's own frame and near every sphere; through an identity
// frame (so that q's coordinates are chosen exactly) points on the line-rule boundary of every member, group and
// union record -- found by bisection on the function itself -- and up to 4 ulps to either side, in 16 directions and at
// axial positions that make the lane margin small, comparable and large (up to 2^29) against the radius; points on
// the behind-rule boundary likewise; NaN, +-inf and +-0 in every coordinate.  Every sample is evaluated.
//
// Teeth: with every group and union radius shrunk by 1 % the same samples must show violations.
//
// Prints "shadow_group_host: <n> scenes, <l> lights, <s> samples, <c> member checks, <f> failures" and
// "shadow_group_host_shrunk: <g> failures"; exit status 0 iff f == 0 and g > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_scene.h"
#include "rt_shadow_pre.h"

using namespace rtk;

namespace {
uint64_t rng = 0x5AD0F6120ull;
uint64_t next64() {
    uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double unif() { return (double)(next64() >> 40) * 0x1p-24; }
float unif(float lo, float hi) { return lo + (hi - lo) * (float)unif(); }
rt_vec3 v3(float x, float y, float z) { return rt_vec3{x, y, z}; }

rt_material diffuse() {
    rt_material m;
    std::memset(&m, 0, sizeof m);
    m.kd = m.ka = v3(0.6f, 0.6f, 0.6f);
    return m;
}
rt_sphere sphere(float x, float y, float z, float r) { return rt_sphere{v3(x, y, z), r, diffuse()}; }
rt_light light(float x, float y, float z) { return rt_light{v3(x, y, z), 1.0f}; }

// raytracer_hip/scenes.py generated_spheres(count): centres and radii
std::vector<rt_sphere> generated_spheres(int count) {
    std::vector<rt_sphere> s{sphere(2.5f, 0, 8, 1), sphere(3, 0, 5, 1), sphere(-3, 1, 8, 1)};
    s.resize((size_t)std::min(count, 3));
    uint64_t st = 0x5EED;
    auto next = [&]() {
        st += 0x9E3779B97F4A7C15ull;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    auto uni = [&]() { return (double)(next() >> 40) * 0x1p-24; };
    auto q = [](double x) { return std::floor(64.0 * x + 0.5) / 64.0; };
    for (int i = 3; i < count; ++i) {
        const double r = q(0.25 + 0.75 * uni());
        const double x = q(-8.0 + 16.0 * uni());
        const double z = q(4.0 + 28.0 * uni());
        const double y = q(-1.0 + r + 0.5 * uni());
        for (int k = 0; k < 3; ++k) (void)next();  // the colour
        s.push_back(sphere((float)x, (float)y, (float)z, (float)r));
    }
    return s;
}
const std::vector<rt_light> REF_LIGHTS{light(-3, 1, -3), light(33, 1, 10)};
const std::vector<rt_light> C4_LIGHTS{light(-3, 1, -3), light(33, 1, 10), light(0, 12, 4), light(-20, 6, 30)};

struct Totals {
    long scenes = 0, lights = 0, samples = 0, checks = 0, failures = 0, shrunk_failures = 0, structure = 0;
} tot;

void fail(const char* scene, const char* what, int li, int a, int b) {
    if (++tot.failures <= 20) std::fprintf(stderr, "FAIL %s light %d: %s (%d, %d)\n", scene, li, what, a, b);
}

bool never_kept(const DevShadowCull& e) { return e.cu == INFINITY && e.rr == 0.0f && e.ca == 0.0f; }
bool always_kept(const DevShadowCull& e) { return e.rr == INFINITY && e.ca == INFINITY; }

DevLight identity_frame() {
    DevLight l;
    std::memset(&l, 0, sizeof l);
    l.ux = 1.0f, l.vy = 1.0f, l.az = 1.0f;
    return l;
}
const DevLight IDENT = identity_frame();
ShadowPreLane lane_at(float ou, float ov, float oa) { return shadow_pre_lane(ou, ov, oa, IDENT); }

struct LightRecords {
    const char* scene;
    int li, S;
    const DevShadowCull* e;  // [s_pad]
    DevShadowGroups g, shrunk;
};

// One lane record against the whole hierarchy of a light.
void check_lane(const LightRecords& r, const ShadowPreLane& q) {
    ++tot.samples;
    const ShadowPreLane qg = shadow_pre_widen(q, SHADOW_GROUP_WIDEN), qu = shadow_pre_widen(q, SHADOW_UNION_WIDEN);
    for (int pass = 0; pass < 2; ++pass) {
        const DevShadowGroups& g = pass ? r.shrunk : r.g;
        const bool ku = shadow_pre_keep(qu, g.uni);
        for (int k = 0; k < SHADOW_GROUPS; ++k) {
            const bool kg = shadow_pre_keep(qg, g.grp[k]);
            bool bad = kg && g.mask[k] != 0 && !ku;  // group => union
            for (int i = 0; i < r.S; ++i) {
                if (!(g.mask[k] >> i & 1u)) continue;
                if (!pass) ++tot.checks;
                if (shadow_pre_keep(q, r.e[i]) && !(kg && ku)) bad = true;  // member => group, member => union
            }
            if (!bad) continue;
            if (pass) ++tot.shrunk_failures;
            else {
                fail(r.scene, "a kept record whose enclosing record is dropped", r.li, k, 0);
                if (tot.failures <= 20) std::fprintf(stderr, "   q = {%a, %a, %a, %a}\n", q.ou, q.ov, q.oa, q.ml);
            }
        }
    }
}

float step_ulps(float v, int n) {
    for (; n > 0; --n) v = std::nextafter(v, INFINITY);
    for (; n < 0; ++n) v = std::nextafter(v, -INFINITY);
    return v;
}

// Points around the line-rule boundary of record b along direction (cx, sy) at axial coordinate oa; the boundary
// distance comes from bisection on shadow_pre_keep's own answer (the margin varies with the point).
void line_boundary(const LightRecords& r, const DevShadowCull& b, double cx, double sy, float oa, int ulps) {
    if (!std::isfinite(b.rr) || !std::isfinite(b.cu) || !std::isfinite(b.cv)) return;
    auto at = [&](double rho) { return lane_at((float)((double)b.cu + rho * cx), (float)((double)b.cv + rho * sy), oa); };
    auto inside = [&](double rho) {
        const ShadowPreLane q = at(rho);
        const float wu = b.cu - q.ou, wv = b.cv - q.ov, T = b.rr + q.ml;
        return !(__builtin_fmaf(wu, wu, wv * wv) > T * T);
    };
    double lo = 0.0, hi = std::max(4.0 * (double)b.rr, 1.0);
    for (int k = 0; k < 80 && inside(hi); ++k) hi *= 2.0;
    if (inside(hi) || !inside(lo)) {
        check_lane(r, at(hi));
        return;
    }
    for (int k = 0; k < 70; ++k) {
        const double mid = 0.5 * (lo + hi);
        if (inside(mid)) lo = mid; else hi = mid;
    }
    const ShadowPreLane q0 = at(hi);
    for (int du = -ulps; du <= ulps; ++du)
        for (int dv = -ulps; dv <= ulps; dv += 2) check_lane(r, lane_at(step_ulps(q0.ou, du), step_ulps(q0.ov, dv), oa));
}

// Points around the behind-rule boundary of record b at (ou, ov).
void behind_boundary(const LightRecords& r, const DevShadowCull& b, float ou, float ov) {
    if (!std::isfinite(b.ca)) return;
    auto behind = [&](double oa) {
        const ShadowPreLane q = lane_at(ou, ov, (float)oa);
        return q.oa - b.ca > q.ml;
    };
    double lo = (double)b.ca - 1.0, hi = std::max(2.0 * std::fabs((double)b.ca), 1.0) + std::fabs((double)ou) + std::fabs((double)ov);
    for (int k = 0; k < 80 && !behind(hi); ++k) hi *= 2.0;
    if (!behind(hi) || behind(lo)) {
        check_lane(r, lane_at(ou, ov, (float)hi));
        return;
    }
    for (int k = 0; k < 70; ++k) {
        const double mid = 0.5 * (lo + hi);
        if (behind(mid)) hi = mid; else lo = mid;
    }
    for (int d = -4; d <= 4; ++d) check_lane(r, lane_at(ou, ov, step_ulps((float)hi, d)));
}

// dense: the named scenes (16 directions, 6 axial positions, +-4 ulps); the random ones take 4, 3 and +-2
void check_light(const char* name, const SceneLayout& L, int li, const std::vector<rt_sphere>& sph, bool dense) {
    const int S = L.S, s_pad = S + (S & 1);
    LightRecords r;
    r.scene = name, r.li = li, r.S = S;
    r.e = (const DevShadowCull*)(L.host_blob.data() + L.off_shpre) + (size_t)li * (size_t)s_pad;
    r.g = ((const DevShadowGroups*)(L.host_blob.data() + L.off_shgrp))[li];
    r.shrunk = r.g;
    r.shrunk.uni.rr *= 0.99f;
    for (DevShadowCull& e : r.shrunk.grp) e.rr *= 0.99f;
    const DevLight& dl = ((const DevLight*)(L.host_blob.data() + L.off_li))[li];
    ++tot.lights;

    // structure
    uint32_t seen = 0;
    bool any_bad = false;
    for (int k = 0; k < SHADOW_GROUPS; ++k) {
        ++tot.structure;
        if (r.g.mask[k] & seen) fail(name, "the masks overlap", li, k, 0);
        seen |= r.g.mask[k];
        bool bad = false;
        for (int i = 0; i < S; ++i)
            if ((r.g.mask[k] >> i & 1u) && always_kept(r.e[i])) bad = true;
        any_bad |= bad;
        if (r.g.mask[k] == 0 && !never_kept(r.g.grp[k])) fail(name, "an empty group's record can be kept", li, k, 0);
        if (bad && !always_kept(r.g.grp[k])) fail(name, "an unusable member's group is not +inf", li, k, 0);
        if (r.g.mask[k] != 0 && !bad)
            for (int i = 0; i < S; ++i)
                if ((r.g.mask[k] >> i & 1u) && !(r.g.grp[k].ca >= r.e[i].ca && r.g.grp[k].rr > r.e[i].rr))
                    fail(name, "a group record below a member's", li, k, i);
    }
    if (seen != (S ? (1u << S) - 1u : 0u)) fail(name, "the masks do not cover exactly the spheres", li, (int)seen, S);
    if (any_bad && !always_kept(r.g.uni)) fail(name, "an unusable member's union is not +inf", li, 0, 0);
    if (S == 0 && !never_kept(r.g.uni)) fail(name, "the union of no sphere can be kept", li, 0, 0);
    if (S & 1) {
        if (!never_kept(r.e[S])) fail(name, "the padding record", li, S, 0);
        if (seen >> S) fail(name, "the padding sphere is in a group", li, S, 0);
    }

    // hit points through the light's own frame: every scale, and near every sphere
    for (int ex = -10; ex <= 40; ++ex)
        for (int k = 0; k < 6; ++k) {
            const float s = std::ldexp(1.0f, ex);
            check_lane(r, shadow_pre_lane(unif(-s, s), unif(-s, s), unif(-s, s), dl));
        }
    for (const rt_sphere& s : sph)
        for (int k = 0; k < 12; ++k) {
            const float w = 4.0f * std::fabs(s.radius) * (float)unif() + 0.01f;
            check_lane(r, shadow_pre_lane(s.center.x + unif(-w, w), s.center.y + unif(-w, w), s.center.z + unif(-w, w), dl));
        }
    // special values
    const float sp[] = {NAN, INFINITY, -INFINITY, 0.0f, 1.0f, -0.0f, 0x1p38f, -0x1p38f, 0x1p-149f, 0x1.fffffep127f};
    const int n_sp = dense ? 10 : 5;
    for (int ia = 0; ia < n_sp; ++ia)
        for (int ib = 0; ib < n_sp; ++ib)
            for (int ic = 0; ic < n_sp; ++ic) {
                const float a = sp[ia], b = sp[ib], c = sp[ic];
                check_lane(r, shadow_pre_lane(a, b, c, dl));
                check_lane(r, lane_at(a, b, c));
                check_lane(r, ShadowPreLane{a, b, c, INFINITY});
            }
    // boundaries of every record: members, groups, union
    std::vector<DevShadowCull> recs(r.e, r.e + S);
    for (const DevShadowCull& e : r.g.grp) recs.push_back(e);
    recs.push_back(r.g.uni);
    for (const DevShadowCull& b : recs) {
        if (!std::isfinite(b.rr) || !std::isfinite(b.ca) || !std::isfinite(b.cu)) continue;
        // axial positions: just ahead of the sphere (the behind rule silent), and far ahead, where the lane margin
        // 2^-8 |O|_1 outgrows the radius
        float oas[6] = {b.ca - 1.0f, b.ca - (float)unif() * b.rr, -0x1p6f, -0x1p14f, -0x1p22f, -0x1p36f};
        const int n_dir = dense ? 16 : 4, first = dense ? 0 : (int)(next64() % 4);
        for (int a = first; a < (dense ? 6 : first + 3); ++a)
            for (int d = 0; d < n_dir; ++d) {
                const double th = (d + unif()) * (2.0 * M_PI / n_dir);
                line_boundary(r, b, std::cos(th), std::sin(th), oas[a % 6], dense ? 4 : 2);
            }
        for (int k = 0; k < 8; ++k) {
            const float w = k < 2 ? 0.0f : 1.5f * b.rr;
            behind_boundary(r, b, b.cu + unif(-w, w), b.cv + unif(-w, w));
        }
    }
}

void check_scene(const char* name, const std::vector<rt_sphere>& sph, const std::vector<rt_light>& li, bool dense = true) {
    const rt_plane floor{v3(0, -1, 0), v3(0, 1, 0), diffuse()};
    const SceneLayout L = scene_build(sph.data(), (int)sph.size(), &floor, 1, li.data(), (int)li.size(), v3(0.1f, 0.1f, 0.1f), 3);
    ++tot.scenes;
    if (!L.has_shpre || !L.has_shgrp) {
        fail(name, "no records", 0, L.has_shpre, L.has_shgrp);
        return;
    }
    if (L.off_shgrp % 16 != 0 || L.off_shgrp + sizeof(DevShadowGroups) * li.size() > L.host_blob.size())
        fail(name, "the records' place in the scene image", 0, (int)L.off_shgrp, (int)L.host_blob.size());
    for (int j = 0; j < (int)li.size(); ++j) check_light(name, L, j, sph, dense);
    SceneOptions off;
    off.shadow_groups = false;
    const SceneLayout N = scene_build(sph.data(), (int)sph.size(), &floor, 1, li.data(), (int)li.size(), v3(0.1f, 0.1f, 0.1f), 3, off);
    if (N.has_shgrp || !N.has_shpre) fail(name, "shadow_groups = false leaves records", 0, N.has_shgrp, N.has_shpre);
    SceneOptions nopre;
    nopre.shadow_pre = false;
    const SceneLayout M = scene_build(sph.data(), (int)sph.size(), &floor, 1, li.data(), (int)li.size(), v3(0.1f, 0.1f, 0.1f), 3, nopre);
    if (M.has_shgrp || M.has_shpre) fail(name, "no pre-test records, yet group records", 0, M.has_shgrp, M.has_shpre);
}
}  // namespace

int main() {
    check_scene("C1", generated_spheres(3), {REF_LIGHTS[0]});
    check_scene("C2", generated_spheres(8), {REF_LIGHTS[0]});
    check_scene("C3", generated_spheres(8), REF_LIGHTS);
    check_scene("REF", generated_spheres(3), REF_LIGHTS);
    check_scene("C4[:11]", generated_spheres(11), C4_LIGHTS);
    {
        const SceneLayout L = scene_build(nullptr, 0, nullptr, 0, nullptr, 0, v3(0, 0, 0), 0);
        if (L.has_shgrp) fail("empty", "a scene without lights has group records", 0, 0, 0);
        const std::vector<rt_sphere> many = generated_spheres(12);
        const SceneLayout B = scene_build(many.data(), 12, nullptr, 0, REF_LIGHTS.data(), 2, v3(0, 0, 0), 0);
        if (B.has_shgrp || B.has_shpre) fail("S=12", "a bundle-kernel scene has group records", 0, 0, 0);
    }
    // degenerate scenes
    check_scene("coincident", std::vector<rt_sphere>(7, sphere(1, 2, 9, 0.5f)), REF_LIGHTS);
    check_scene("far apart", {sphere(-0x1p29f, 0, 5, 1), sphere(0x1p29f, 0, 5, 1), sphere(0, 0x1p30f, 5, 2), sphere(1, 0, 5, 1)}, C4_LIGHTS);
    check_scene("nan radius", {sphere(2, 0, 8, 1), sphere(0, 0, 6, NAN), sphere(-2, 0, 7, 0.5f)}, REF_LIGHTS);
    check_scene("tiny radius", {sphere(2, 0, 8, 1), sphere(0, 0, 6, 0x1p-60f), sphere(-2, 0, 7, 0.5f), sphere(4, 1, 9, 0.25f)}, REF_LIGHTS);
    check_scene("huge radius", {sphere(2, 0, 8, 0x1p60f), sphere(0, 0, 6, 1), sphere(-2, 0, 7, 0x1p63f)}, REF_LIGHTS);
    check_scene("centre 2^38", {sphere(0x1p38f, 0, 8, 1), sphere(0, 0, 6, 1), sphere(-2, 0, 7, 0.5f)}, REF_LIGHTS);
    check_scene("centre nan", {sphere(NAN, 0, 8, 1), sphere(0, INFINITY, 6, 1), sphere(-2, 0, 7, 0.5f)}, REF_LIGHTS);
    check_scene("every sphere unusable", {sphere(0, 0, 6, NAN), sphere(1, 0, 6, NAN)}, REF_LIGHTS);
    check_scene("light a 2^42", generated_spheres(5), {light(0x1p21f, 0, 0), REF_LIGHTS[0]});
    check_scene("light a 2^-42", generated_spheres(5), {light(0, 0x1p-21f, 0), REF_LIGHTS[1]});
    check_scene("light at the origin", generated_spheres(8), {light(0, 0, 0), REF_LIGHTS[0]});
    check_scene("light nan", generated_spheres(4), {light(NAN, 0, 0)});
    check_scene("no spheres", {}, REF_LIGHTS);
    check_scene("one sphere", generated_spheres(1), REF_LIGHTS);
    check_scene("odd count", generated_spheres(7), REF_LIGHTS);
    // random scenes
    const float scales[] = {1e-3f, 1.0f, 30.0f, 1000.0f};
    for (int n = 0; n < 3000; ++n) {
        const int S = (int)(next64() % 12), nl = 1 + (int)(next64() % 4);
        const float sc = scales[next64() % 4];
        std::vector<rt_sphere> sph;
        for (int i = 0; i < S; ++i) {
            // clustered or spread centres; radii from a sliver to the scene's size
            const float spread = (next64() & 1) ? sc : 0.1f * sc;
            sph.push_back(sphere(unif(-spread, spread), unif(-spread, spread), unif(-spread, spread) + 2.0f * sc,
                                 sc * std::ldexp(1.0f, -(int)(next64() % 10))));
        }
        std::vector<rt_light> li;
        for (int j = 0; j < nl; ++j) li.push_back(light(unif(-4 * sc, 4 * sc), unif(-4 * sc, 4 * sc), unif(-4 * sc, 4 * sc)));
        char name[64];
        std::snprintf(name, sizeof name, "random %d (S %d, L %d, scale %g)", n, S, nl, (double)sc);
        check_scene(name, sph, li, n % 100 == 0);
    }
    std::printf("shadow_group_host: %ld scenes, %ld lights, %ld samples, %ld member checks, %ld failures\n", tot.scenes, tot.lights,
                tot.samples, tot.checks, tot.failures);
    std::printf("shadow_group_host_shrunk: %ld failures\n", tot.shrunk_failures);
    return tot.failures == 0 && tot.shrunk_failures > 0 ? 0 : 1;
}
