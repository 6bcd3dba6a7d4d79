// Host check of the plane footprints (csrc/rt_foot.h; tests/test_foot_host.py), TEST INFRASTRUCTURE ONLY.
// Built by the Makefile beside it (its pure rule) as host C++ with ASan + UBSan and -ffp-contract=off, run as a plain
// executable on the CPU.  The views, screen boxes and view-table values are the library's own (csrc/rt_view.h).
//
// The kernel's primary direction (trace_tile_direct: the view-plane point, vp - cam, Vector3.Normalize) and
// plane_take's `may` are restated here in binary32, in the kernel's operation order, and evaluated at every pixel of
// small frames for a sweep of views and planes.
//   1. Soundness: wherever a footprint's rule says "cannot hit", may is false.  Zero failures.
//   2. Teeth: the same sweep with the footprints built without margins (foot_build(..., margins = false)) has
//      failures -- the cameras far from the origin are there for that.
//   3. Effect: on C3's 1920 x 1080 view the rule and the spheres' screen boxes (rt_view.h prim_box) leave at
//      least 12,500 of the 32,400 tiles with nothing to trace, and none on a view that looks straight down.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_view.h"

using namespace rtk;

namespace {

struct V3 {
    float x, y, z;
};
V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 scale(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
float dot(V3 a, V3 b) { return ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z); }  // Vector3.Dot
V3 normalize(V3 a) {  // Vector3.Normalize
    const float s = 1.0f / std::sqrt(dot(a, a));
    return scale(a, s);
}

// The library's view of a camera on a W x H frame (rt_view.h view_build; no scene: the sweep brings its own planes)
void view_of(V3 pos, double yaw, double pitch, int W, int H, LaunchParams& lp) {
    std::memset(&lp, 0, sizeof lp);
    const rt_camera cam{rt_vec3{pos.x, pos.y, pos.z}, (float)yaw, (float)pitch};
    if (view_build(SceneLayout{}, cam, W, H, lp) != RT_OK) std::abort();
}

// trace_tile_direct's primary direction
V3 primary_dir(const LaunchParams& lp, float lx, float ly) {
    const V3 cam{lp.cam[0], lp.cam[1], lp.cam[2]}, R{lp.right[0], lp.right[1], lp.right[2]};
    const V3 U{lp.up[0], lp.up[1], lp.up[2]}, F{lp.fwd[0], lp.fwd[1], lp.fwd[2]};
    const float lz = 1.0f * lp.nearc;
    const V3 vp = add(add(add(cam, scale(R, lx)), scale(U, ly)), scale(F, lz));
    return normalize(sub(vp, cam));
}
// plane_take's may, o = the camera
bool plane_may(const LaunchParams& lp, V3 d, const DevPlane& q) {
    const V3 o{lp.cam[0], lp.cam[1], lp.cam[2]};
    const float num = ((-o.x * q.nx - o.y * q.ny) - o.z * q.nz) + q.cn;
    const float den = dot(d, V3{q.nx, q.ny, q.nz});
    return (num > 0.0f && den > 0.0f) || (num < 0.0f && den < 0.0f);
}

DevPlane plane(V3 c, V3 n) {  // rt_set_scene's record (the checkerboard basis is not read here)
    DevPlane d;
    std::memset(&d, 0, sizeof d);
    d.cx = c.x, d.cy = c.y, d.cz = c.z;
    d.cn = dot(c, n);
    d.nx = n.x, d.ny = n.y, d.nz = n.z;
    return d;
}

uint64_t rng_state = 0x1234567;
double unif() {  // splitmix64
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}
V3 unit() {
    for (;;) {
        const double x = 2 * unif() - 1, y = 2 * unif() - 1, z = 2 * unif() - 1, l = std::sqrt(x * x + y * y + z * z);
        if (l > 0.1 && l <= 1.0) return V3{(float)(x / l), (float)(y / l), (float)(z / l)};
    }
}

// raytracer_hip/scenes.py generated_spheres(8): the C2 / C3 spheres (centres and radii)
std::vector<DevSphere> c3_spheres() {
    std::vector<DevSphere> s{{2.5f, 0, 8, 1.0f}, {3, 0, 5, 1.0f}, {-3, 1, 8, 1.0f}};
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
    for (int i = 3; i < 8; ++i) {
        const double r = q(0.25 + 0.75 * uni());
        const double x = q(-8.0 + 16.0 * uni());
        const double z = q(4.0 + 28.0 * uni());
        const double y = q(-1.0 + r + 0.5 * uni());
        for (int k = 0; k < 3; ++k) (void)next();  // the colour
        const float rf = (float)r;
        s.push_back(DevSphere{(float)x, (float)y, (float)z, rf * rf});
    }
    return s;
}

// Tiles of the view with nothing to trace, as the kernel decides it: no sphere's box overlaps the tile (box_mask:
// the tile's first and last pixel, valid or not) and every valid pixel fails every plane's rule.
int sky_tiles(const LaunchParams& lp, const std::vector<DevSphere>& sph, const std::vector<DevPlane>& pl) {
    PlaneFoot foot[FOOT_MAX];
    const int n = foot_build(lp, pl.data(), (int)pl.size(), foot);
    if (n < 0) return 0;
    std::vector<PrimBox> box;
    for (const DevSphere& s : sph) box.push_back(prim_box(lp, s));
    std::vector<float> tab((size_t)lp.W + (size_t)lp.H);  // lx[W] then ly[H]
    view_table_values(lp.W, lp.H, lp.pw, lp.ph, tab.data());
    int count = 0;
    for (int ty = 0; ty < (lp.H + 7) / 8; ++ty)
        for (int tx = 0; tx < (lp.W + 7) / 8; ++tx) {
            const int x_lo = tx * 8, x_hi = tx * 8 + 7, y_lo = ty * 8, y_hi = ty * 8 + 7;
            bool cand = false;
            for (const PrimBox& b : box) cand |= b.x0 <= x_hi && b.x1 >= x_lo && b.y0 <= y_hi && b.y1 >= y_lo;
            for (int y = y_lo; y <= y_hi && y < lp.H && !cand; ++y)
                for (int x = x_lo; x <= x_hi && x < lp.W && !cand; ++x)
                    for (int i = 0; i < n; ++i) cand |= foot_may_hit(foot[i], tab[(size_t)x], tab[(size_t)lp.W + (size_t)y]);
            count += !cand;
        }
    return count;
}

}  // namespace

int main() {
    // planes: the floor, arbitrary normals, scaled normals, a large cn, the far wall, and normals outside the domain
    std::vector<DevPlane> pool;
    pool.push_back(plane(V3{0, -1, 0}, V3{0, 1, 0}));                                   // 0 the floor
    for (int i = 0; i < 4; ++i) {                                                        // 1-4 arbitrary
        const V3 c{(float)(6 * unif() - 3), (float)(6 * unif() - 3), (float)(6 * unif() - 3)};
        pool.push_back(plane(c, unit()));
    }
    pool.push_back(plane(V3{1, -2, 3}, scale(unit(), 1e-3f)));                          // 5 |n| = 1e-3
    pool.push_back(plane(V3{-2, 1, 4}, scale(unit(), 1e3f)));                           // 6 |n| = 1e3
    pool.push_back(plane(V3{0, -1e6f, 0}, V3{0, 1, 0}));                                // 7 cn = -1e6
    pool.push_back(plane(V3{3e5f, -8e5f, 5e5f}, unit()));                               // 8 |cn| up to 1e6
    pool.push_back(plane(V3{0, 0, 48}, V3{0, 0, -1}));                                  // 9 the C4 wall
    const int good = (int)pool.size();
    pool.push_back(plane(V3{0, -1, 0}, V3{0, 0, 0}));                                   // 10 zero normal
    pool.push_back(plane(V3{0, -1, 0}, V3{0, NAN, 0}));                                 // 11 NaN normal
    pool.push_back(plane(V3{0, -1, 0}, V3{0, INFINITY, 0}));                            // 12 inf normal
    const std::vector<std::vector<int>> sets{{}, {0}, {0, 9}, {1, 2, 3, 4}, {0, 1, 2, 3, 4}, {5, 6, 7}, {8}, {3, 5, 7, 9},
                                             {10}, {0, 11}, {12, 1}, {2}, {4, 6, 8, 0}};
    const double pitches[] = {-1.6, -1.5707963, -1.1, -0.5, -0.26, -1e-3, 0.0, 1e-7, 0.02, 0.26, 0.52, 1.0, 1.5707963, 3.0};
    const double yaws[] = {0.0, 0.4, 1.5707963, 2.5, 3.14159265, -2.0, 6.5};
    const V3 cams[] = {{0, 0, 0},       {0.3f, 2, -1},    {0, -5, 0},     {0, -1, 0} /* on the floor */,
                       {1, -1.0000001f, 2}, {10, 3, -4},  {-20, 40, 30},  {50, -30, 35},
                       {100, 20, -50},  {-1e3f, 500, 300}, {6e3f, -5e3f, 6e3f}};
    const int sizes[][2] = {{64, 40}, {37, 23}, {100, 60}};

    long long views = 0, checked = 0, excluded = 0, failures = 0, off = 0, teeth_excluded = 0, teeth_failures = 0;
    std::vector<V3> dir;
    std::vector<float> tab;  // the view tables: lx[W] then ly[H]
    for (const V3& cam : cams)
        for (double pitch : pitches)
            for (double yaw : yaws) {
                const int* sz = sizes[views % 3];
                ++views;
                LaunchParams lp;
                view_of(cam, yaw, pitch, sz[0], sz[1], lp);
                const int W = sz[0], H = sz[1];
                dir.resize((size_t)W * H), tab.resize((size_t)W + (size_t)H);
                view_table_values(W, H, lp.pw, lp.ph, tab.data());
                const float *lxs = tab.data(), *lys = tab.data() + W;
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) dir[(size_t)y * W + x] = primary_dir(lp, lxs[(size_t)x], lys[(size_t)y]);
                auto sweep = [&](const DevPlane& q, const PlaneFoot& f, long long& n_excl, long long& n_fail) {
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x) {
                            ++checked;
                            if (foot_may_hit(f, lxs[(size_t)x], lys[(size_t)y])) continue;
                            ++n_excl;
                            if (plane_may(lp, dir[(size_t)y * W + x], q)) {
                                if (&n_fail == &failures && n_fail < 10)
                                    std::printf("FAIL cam (%g %g %g) pitch %g yaw %g pixel (%d, %d) plane n (%g %g %g) cn %g\n", cam.x,
                                                cam.y, cam.z, pitch, yaw, x, y, q.nx, q.ny, q.nz, q.cn);
                                ++n_fail;
                            }
                        }
                };
                for (const std::vector<int>& set : sets) {
                    std::vector<DevPlane> pl;
                    for (int i : set) pl.push_back(pool[(size_t)i]);
                    PlaneFoot foot[FOOT_MAX + 1];
                    const int n = foot_build(lp, pl.data(), (int)pl.size(), foot);
                    if (n < 0) {
                        ++off;
                        continue;
                    }
                    if (n != (int)pl.size()) ++failures;
                    for (int i = 0; i < n; ++i) sweep(pl[(size_t)i], foot[i], excluded, failures);
                }
                for (int i = 0; i < good; ++i) {  // the teeth: no margins
                    PlaneFoot f;
                    if (foot_build(lp, &pool[(size_t)i], 1, &f, false) == 1) sweep(pool[(size_t)i], f, teeth_excluded, teeth_failures);
                }
            }
    std::printf("foot_host: %lld views, %lld plane sets without footprints, %lld rules checked, %lld excluded\n", views, off,
                checked, excluded);
    std::printf("foot_host: teeth without margins: %lld failures of %lld excluded\n", teeth_failures, teeth_excluded);

    // the effect on C3's view, and on a view that looks straight down at the floor
    const std::vector<DevSphere> sph = c3_spheres();
    const std::vector<DevPlane> floor{pool[0]};
    LaunchParams lp;
    view_of(V3{0, 0, 0}, 0.0, 0.0, 1920, 1080, lp);
    std::printf("foot_host: C3 1920x1080: %d of %d tiles skippable\n", sky_tiles(lp, sph, floor), 240 * 135);
    view_of(V3{0, 0, 0}, 0.0, 1.5707963267948966, 1920, 1080, lp);
    std::printf("foot_host: straight down 1920x1080: %d of %d tiles skippable\n", sky_tiles(lp, sph, floor), 240 * 135);
    std::printf("foot_host: %lld failures\n", failures);
    return failures == 0 ? 0 : 1;
}
