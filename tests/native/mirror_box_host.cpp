// mirror_box_host.cpp -- host check of the direct kernel's mirrored screen boxes (csrc/rt_view.h mirror_boxes /
// view_mirror_boxes, LaunchParams::mbox), TEST INFRASTRUCTURE ONLY.  Plain host C++ against the library's device-free
// builders (rt_scene.h scene_build, rt_view.h view_build) under ASan + UBSan; no device code is compiled or linked.
//
// Random scenes of 1-11 spheres over the scales of san_host.cpp's check_shadow_pre (1e-3, 1, 30, 1000) with 1-3
// mirror planes -- floors, tilted planes, planes just under or over the camera, the camera on either side,
// normals that are unit only up to rounding, off by 2^-22 (table kept) and off by 1e-3 (no table) -- spheres
// touching, cutting and behind a plane, and cameras far from the origin (where the binary32 hit point is coarse
// against the scene).  For every sampled pixel, boxed plane k and sphere i such that the pixel lies outside
// mbox[k][i] and the pixel's primary ray meets the plane at 0 < t <= mbox_tmax[k], the oracle's binary32 chain --
// primary ray (TracePixel), IntersectPlane, hit point, CalculateReflectionRay, IntersectsSphere with epsilon 0 --
// must report no collision: the sphere's distance is then not selectable under TraceSecondaryRay's rule either.
// Pixels are sampled over the frame and on the rows and columns just outside every box.
//
// Teeth: the same boxes built without the added allowances (mirror_boxes(..., margins = false): prim_box of the
// mirrored sphere alone, no t_max) must fail that check somewhere.
//
// Prints "mirror_box: <n> (pixel, plane, sphere) triples outside a box, <f> failures" and
// "mirror_box_nomargin: <m> triples, <g> failures"; exit status 0 iff f == 0 and g > 0.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_view.h"

#include "../../oracle/oracle.h"

using namespace rtk;

namespace {
uint64_t rng = 0xB0C5ED5EEDull;
uint64_t next64() {
    uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float unif(float lo, float hi) { return lo + (hi - lo) * (float)((next64() >> 40) * (1.0 / 16777216.0)); }
rt_vec3 v3(float x, float y, float z) { return rt_vec3{x, y, z}; }
rt_vec3 vec(H3 a) { return rt_vec3{a.x, a.y, a.z}; }
H3 hadd(H3 a, H3 b) { return H3{a.x + b.x, a.y + b.y, a.z + b.z}; }
H3 hsub(H3 a, H3 b) { return H3{a.x - b.x, a.y - b.y, a.z - b.z}; }
H3 hscale(H3 a, float s) { return H3{a.x * s, a.y * s, a.z * s}; }

rt_material mirror_material(bool diffuse) {
    rt_material m;
    std::memset(&m, 0, sizeof m);
    m.km = v3(0.5f, 0.5f, 0.5f);
    if (diffuse) m.kd = m.ka = v3(0.6f, 0.6f, 0.6f);
    return m;
}

struct Counts {
    long triples = 0, failures = 0;
};

// TracePixel's primary direction (RayTracer.cs:963-971) from the view the library derived.
H3 primary_dir(const LaunchParams& lp, int W, int H, int x, int y) {
    const float lx = ((float)x / (float)W - 0.5f) * lp.pw, ly = ((float)y / (float)H - 0.5f) * lp.ph, lz = 1.0f * lp.nearc;
    const H3 cam{lp.cam[0], lp.cam[1], lp.cam[2]};
    const H3 vp = hadd(hadd(hadd(cam, hscale(H3{lp.right[0], lp.right[1], lp.right[2]}, lx)),
                            hscale(H3{lp.up[0], lp.up[1], lp.up[2]}, ly)),
                       hscale(H3{lp.fwd[0], lp.fwd[1], lp.fwd[2]}, lz));
    return hnormalize(hsub(vp, cam));
}

// One pixel against one plane's table.
void check_pixel(const LaunchParams& lp, int W, int H, int x, int y, const rt_plane& pl, const PrimBox* box, float t_max,
                 const std::vector<rt_sphere>& sph, Counts& c, bool report, int scene) {
    const H3 cam{lp.cam[0], lp.cam[1], lp.cam[2]};
    const H3 d = primary_dir(lp, W, H, x, y);
    int col = 0;
    const float t = oracle_intersect_plane(vec(cam), vec(d), pl.center, pl.normal, &col);
    if (!col || !(t <= t_max)) return;  // the lane's conditions: a hit on this plane, not beyond t_max
    const H3 hp = hadd(cam, hscale(d, t));
    const H3 n = h3(pl.normal);
    const H3 rd = hsub(d, hscale(n, 2.0f * hdot(d, n)));  // CalculateReflectionRay :718-720
    for (size_t i = 0; i < sph.size(); ++i) {
        const PrimBox& b = box[i];
        if (x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1) continue;
        ++c.triples;
        int hit = 0;
        const float dist = oracle_intersect_sphere(vec(hp), vec(rd), sph[i].center, sph[i].radius, 0.0f, &hit);
        if (hit) {
            ++c.failures;
            if (report && c.failures <= 20)
                std::fprintf(stderr, "FAIL scene %d pixel (%d, %d) of %dx%d: sphere %zu outside its mirrored box but hit at %a (t %a)\n",
                             scene, x, y, W, H, i, dist, t);
        }
    }
}

void check_table(const LaunchParams& lp, int W, int H, const rt_plane& pl, const PrimBox* box, float t_max,
                 const std::vector<rt_sphere>& sph, Counts& c, bool report, int scene) {
    // over the frame
    for (int k = 0; k < 1500; ++k)
        check_pixel(lp, W, H, (int)(next64() % (uint64_t)W), (int)(next64() % (uint64_t)H), pl, box, t_max, sph, c, report, scene);
    // the columns and rows just outside every box (inside the frame)
    for (size_t i = 0; i < sph.size(); ++i) {
        const PrimBox& b = box[i];
        if (b.x0 <= INT_MIN / 2) continue;  // "all"
        const long long bw = (long long)b.x1 - b.x0 + 1, bh = (long long)b.y1 - b.y0 + 1;
        for (int k = 0; k < 200; ++k) {
            const int side = k & 3, off = 1 + (int)(next64() % 3 == 0 ? next64() % 8 : 0);
            long long x, y;
            if (side < 2) {
                x = side == 0 ? (long long)b.x0 - off : (long long)b.x1 + off;
                y = b.y0 - 2 + (long long)(next64() % (uint64_t)(bh + 4));
            } else {
                y = side == 2 ? (long long)b.y0 - off : (long long)b.y1 + off;
                x = b.x0 - 2 + (long long)(next64() % (uint64_t)(bw + 4));
            }
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            check_pixel(lp, W, H, (int)x, (int)y, pl, box, t_max, sph, c, report, scene);
        }
    }
}

void run(Counts& with, Counts& without) {
    long tables = 0, no_tables = 0, boxed = 0;
    for (int it = 0; it < 320; ++it) {
        const float scale = it % 4 == 3 ? 1000.0f : it % 4 == 2 ? 30.0f : it % 8 == 1 ? 1e-3f : 1.0f;
        const int S = 1 + (int)(next64() % (CULL_MIN_SPHERES - 1)), P = 1 + (int)(next64() % 3);
        // far cameras: the whole scene and the camera moved away from the origin
        const bool coarse = it % 6 == 1 || it >= 240;  // (the last 80 scenes: all of this kind)
        const float far = coarse ? 60.0f : it % 6 == 4 ? 20.0f * scale : 0.0f;
        const rt_vec3 shift = v3(far * 0.6f, far * 0.2f, far * 0.77f);
        std::vector<rt_sphere> sph((size_t)S);
        std::vector<rt_plane> pl((size_t)P);
        rt_camera cam{v3(shift.x + unif(-1, 1) * scale, shift.y + unif(0.2f, 2.5f) * scale, shift.z + unif(-1, 1) * scale),
                      unif(-0.5f, 0.5f), unif(-0.2f, 0.7f)};
        for (int j = 0; j < P; ++j) {
            rt_plane& q = pl[(size_t)j];
            q.material = mirror_material(j != 1);
            float h = unif(-2.0f, -0.3f) * scale;  // below the camera ...
            if (it % 5 == 1) h = -unif(1e-3f, 1e-2f) * scale;  // ... or just under it
            H3 n{0.0f, 1.0f, 0.0f};
            if (j == 1 || it % 3 == 1) n = hnormalize(H3{unif(-0.4f, 0.4f), 1.0f, unif(-0.4f, 0.4f)});  // tilted
            if (j == 2) n = hnormalize(H3{unif(-1, 1), unif(-0.3f, 0.3f), unif(-1, -0.2f)});         // a wall
            if (it % 7 == 2) n = hscale(n, 1.0f + 0x1p-22f);  // not unit, within the gate
            if (it % 7 == 5 && j == 0) n = hscale(n, 1.001f);  // not a mirror for the reference: no table
            const bool flip = it % 4 == 1 && j == 0;  // the camera on the other side (the normal away from it)
            if (flip) n = hscale(n, -1.0f);
            q.normal = vec(n);
            if (j == 2) q.center = v3(cam.position.x - 30.0f * scale * n.x, cam.position.y, cam.position.z - 30.0f * scale * n.z);
            else q.center = v3(cam.position.x + unif(-3, 3) * scale, cam.position.y + h, cam.position.z + unif(0, 10) * scale);
            if (it % 9 == 4 && j == 0) q.center.y = cam.position.y + unif(0.3f, 2.0f) * scale;  // a ceiling: pitch up sees it
        }
        if (it % 9 == 4) cam.pitch = unif(-0.7f, 0.0f);
        for (int i = 0; i < S; ++i) {
            rt_sphere& s = sph[(size_t)i];
            s.center = v3(cam.position.x + unif(-8, 8) * scale, cam.position.y + unif(-2, 2) * scale,
                          cam.position.z + unif(2, 40) * scale);
            s.radius = unif(0.05f, 1.5f) * scale;
            s.material = mirror_material(true);
            if (i % 3 == 1) {  // touching, cutting or behind plane 0 (a point of the plane below / above the sphere)
                const rt_plane& q = pl[0];
                const double nd = ((double)q.normal.x * (s.center.x - q.center.x) + (double)q.normal.y * (s.center.y - q.center.y) +
                                   (double)q.normal.z * (s.center.z - q.center.z));
                const double want = (double)s.radius * unif(-1.5f, 1.5f) * (i % 2 ? 1.0 : 0.0) + (i % 2 ? 0.0 : (double)s.radius);
                s.center = v3((float)(s.center.x - (nd - want) * q.normal.x), (float)(s.center.y - (nd - want) * q.normal.y),
                              (float)(s.center.z - (nd - want) * q.normal.z));
            }
        }
        if (it % 8 == 1 || coarse) {  // tiny spheres close to the camera: the binary32 chain's error counts most
            // (with the camera 60 from the origin a binary32 coordinate is a multiple of 2^-18 = 3.8e-6: spheres at
            // 1e-4 .. 6e-4 from it are where the boxes without allowances must fail)
            const float ts = !coarse ? 1e-3f : it % 2 ? 1e-4f : 4e-5f;
            for (int i = 0; i < S; i += 2) {
                sph[(size_t)i].radius = unif(0.02f, 0.2f) * ts;
                sph[(size_t)i].center = v3(cam.position.x + unif(-2, 2) * ts, cam.position.y + unif(-1, 1) * ts,
                                           cam.position.z + unif(1, 6) * ts);
            }
            pl[0].center.y = cam.position.y - unif(0.5f, 2.0f) * ts;
        }
        rt_light li{v3(0, 10, 0), 1.0f};
        const SceneLayout layout = scene_build(sph.data(), S, pl.data(), P, &li, 1, v3(0.1f, 0.1f, 0.1f), 3);
        const int W = it % 3 == 0 ? 1920 : it % 3 == 1 ? 4001 : 333, H = it % 3 == 0 ? 1080 : it % 3 == 1 ? 3001 : 250;
        LaunchParams lp;
        std::memset(&lp, 0, sizeof lp);
        if (view_build(layout, cam, W, H, lp) != RT_OK) {
            std::fprintf(stderr, "FAIL scene %d: view_build\n", it);
            ++with.failures;
            continue;
        }
        if (lp.mbox_n < 0 || lp.mbox_n > MIRROR_BOX_PLANES) {
            std::fprintf(stderr, "FAIL scene %d: mbox_n %d\n", it, lp.mbox_n);
            ++with.failures;
            continue;
        }
        if (it % 7 == 5 && ((lp.mbox_n > 0 && lp.mbox_plane[0] == 0) || (lp.mbox_n > 1 && lp.mbox_plane[1] == 0))) {
            std::fprintf(stderr, "FAIL scene %d: a table for a plane whose normal is not unit\n", it);
            ++with.failures;
        }
        for (int k = 0; k < lp.mbox_n; ++k) {
            const int j = lp.mbox_plane[k];
            if (j < 0 || j >= P || j >= MIRROR_BOX_PLANES) {  // (every plane is a mirror: the first two get the tables)
                std::fprintf(stderr, "FAIL scene %d: table %d for plane %d\n", it, k, j);
                ++with.failures;
                continue;
            }
            ++tables;
            for (int i = 0; i < S; ++i) boxed += lp.mbox[k][i].x0 > INT_MIN / 2;
            check_table(lp, W, H, pl[(size_t)j], lp.mbox[k], lp.mbox_tmax[k], sph, with, true, it);
            // teeth: the same plane's boxes without the allowances
            PrimBox bare[CULL_MIN_SPHERES];
            float tm = 0.0f;
            if (mirror_boxes(lp, layout.host_pl[(size_t)j], layout.host_sph, bare, &tm, false))
                check_table(lp, W, H, pl[(size_t)j], bare, tm, sph, without, false, it);
        }
        no_tables += std::min(P, MIRROR_BOX_PLANES) - lp.mbox_n;
    }
    std::printf("mirror_box: %ld tables (%ld sphere boxes), %ld planes without one\n", tables, boxed, no_tables);
}
}  // namespace

int main() {
    Counts with, without;
    run(with, without);
    std::printf("mirror_box: %ld (pixel, plane, sphere) triples outside a box, %ld failures\n", with.triples, with.failures);
    std::printf("mirror_box_nomargin: %ld triples, %ld failures\n", without.triples, without.failures);
    return with.failures == 0 && with.triples > 0 && without.failures > 0 ? 0 : 1;
}
