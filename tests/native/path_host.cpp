// path_host.cpp -- host check of the camera-path view records (rt_api.cpp view_fill over rt_view.h view_build / view_record, DevView in
// rt_internal.h), TEST INFRASTRUCTURE ONLY.  rt_api.cpp is compiled into this translation unit (its helpers have
// internal linkage) with host-side ASan + UBSan; no device call is reached (contexts without devices).
//
// A camera-path launch reads frame f's view from a DevView record where a one-camera launch reads it from the
// by-value LaunchParams.  For random scenes -- S = 0, 1, 11, 12, 64 and 65 spheres (65: no primary constants),
// with and without mirror planes (the mirrored screen boxes), with and without a view height -- and random
// cameras, the record built for camera c must equal, byte for byte, the fields view_params puts into
// LaunchParams after rt_set_camera(c): cam / right / up / fwd, prim_const, pc[], pbox[], mbox_n, mbox_plane[],
// mbox_tmax[], mbox[][]; and pw / ph / nearc / W, which a path launch shares between its frames, must not
// depend on the camera.  The context's camera and view cache must come out of the record building untouched.
// Teeth: the records of two different cameras differ.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstdint>
#include <cstdio>

namespace {
uint64_t rng = 0xCA3E7A9A7Bull;
uint64_t next64() {
    uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float unif(float lo, float hi) { return lo + (hi - lo) * (float)((next64() >> 40) * (1.0 / 16777216.0)); }
rt_vec3 v3(float x, float y, float z) { return rt_vec3{x, y, z}; }

rt_material material(bool mirror) {
    rt_material m;
    std::memset(&m, 0, sizeof m);
    m.kd = m.ka = v3(0.6f, 0.6f, 0.6f);
    if (mirror) m.km = v3(0.5f, 0.5f, 0.5f);
    return m;
}

rt_camera random_camera() {
    rt_camera c;
    std::memset(&c, 0, sizeof c);
    c.position = v3(unif(-3, 3), unif(0.2f, 3), unif(-3, 3));
    c.yaw = unif(-3.2f, 3.2f);
    c.pitch = unif(-0.8f, 0.8f);
    return c;
}

long failures = 0, records = 0, boxed_records = 0, mirror_records = 0, differing = 0;

#define EXPECT(cond, ...)                  \
    do {                                   \
        if (!(cond)) {                     \
            std::fprintf(stderr, "FAIL "); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");    \
            ++failures;                    \
        }                                  \
    } while (0)

bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

// The record against the LaunchParams of a one-camera launch, field by field, and as a whole (padding zero).
void compare(const DevView& v, const LaunchParams& lp, int scene, int cam) {
    EXPECT(same(v.cam, lp.cam, sizeof v.cam) && same(v.right, lp.right, sizeof v.right) &&
               same(v.up, lp.up, sizeof v.up) && same(v.fwd, lp.fwd, sizeof v.fwd),
           "scene %d camera %d: position / basis", scene, cam);
    EXPECT(v.prim_const == lp.prim_const, "scene %d camera %d: prim_const", scene, cam);
    EXPECT(same(v.pc, lp.pc, sizeof v.pc), "scene %d camera %d: pc", scene, cam);
    EXPECT(same(v.pbox, lp.pbox, sizeof v.pbox), "scene %d camera %d: pbox", scene, cam);
    EXPECT(v.mbox_n == lp.mbox_n && same(v.mbox_plane, lp.mbox_plane, sizeof v.mbox_plane) &&
               same(v.mbox_tmax, lp.mbox_tmax, sizeof v.mbox_tmax) && same(v.mbox, lp.mbox, sizeof v.mbox),
           "scene %d camera %d: mirrored boxes", scene, cam);
    DevView w;
    std::memset(&w, 0, sizeof w);
    std::memcpy(w.cam, lp.cam, sizeof w.cam), std::memcpy(w.right, lp.right, sizeof w.right);
    std::memcpy(w.up, lp.up, sizeof w.up), std::memcpy(w.fwd, lp.fwd, sizeof w.fwd);
    w.prim_const = lp.prim_const, w.mbox_n = lp.mbox_n;
    std::memcpy(w.mbox_plane, lp.mbox_plane, sizeof w.mbox_plane), std::memcpy(w.mbox_tmax, lp.mbox_tmax, sizeof w.mbox_tmax);
    std::memcpy(w.pc, lp.pc, sizeof w.pc), std::memcpy(w.pbox, lp.pbox, sizeof w.pbox), std::memcpy(w.mbox, lp.mbox, sizeof w.mbox);
    EXPECT(same(&v, &w, sizeof v), "scene %d camera %d: the whole record (padding)", scene, cam);
}

void run() {
    static const int counts[] = {0, 1, 11, 12, 64, 65};
    int scene = 0;
    for (int S : counts)
        for (int mirrors = 0; mirrors < 2; ++mirrors)
            for (int vh = 0; vh < 2; ++vh, ++scene) {
                std::vector<rt_sphere> sph((size_t)S);
                for (rt_sphere& s : sph) {
                    s.center = v3(unif(-8, 8), unif(-1, 3), unif(-8, 8));
                    s.radius = unif(0.05f, 1.2f);
                    s.material = material((next64() & 3) == 0);
                }
                rt_plane pl[3];
                const int P = 1 + (scene % 3);
                for (int j = 0; j < P; ++j) {
                    pl[j].material = material(mirrors != 0);
                    pl[j].normal = j == 0 ? v3(0, 1, 0) : j == 1 ? v3(0, 0, -1) : v3(1, 0, 0);
                    pl[j].center = j == 0 ? v3(0, unif(-2.0f, -0.5f), 0) : j == 1 ? v3(0, 0, 12) : v3(-12, 0, 0);
                }
                rt_light li[2] = {{v3(0, 10, 0), 1.0f}, {v3(4, 8, -3), 0.7f}};
                rt_ctx ctx;
                if (rt_set_scene(&ctx, sph.data(), S, pl, P, li, 2, v3(0.1f, 0.1f, 0.1f), scene % 4) != RT_OK) {
                    EXPECT(false, "scene %d: rt_set_scene: %s", scene, ctx.last_error.c_str());
                    continue;
                }
                const int W = scene % 2 ? 1920 : 333, H = scene % 2 ? 1080 : 250;
                if (vh) rt_set_view_height(&ctx, H + 37);
                const int VH = vh ? H + 37 : H;
                const rt_camera own = random_camera();
                rt_set_camera(&ctx, &own);
                LaunchParams own_lp;
                std::memset(&own_lp, 0, sizeof own_lp);
                EXPECT(view_params(&ctx, W, H, own_lp) == RT_OK, "scene %d: view_params", scene);

                // the records of a path, built the way trace_path builds them: one LaunchParams reused
                constexpr int N = 6;
                rt_camera cams[N];
                DevView rec[N];
                LaunchParams scratch;
                std::memset(&scratch, 0, sizeof scratch);
                for (int f = 0; f < N; ++f) {
                    cams[f] = f == N - 1 ? cams[0] : random_camera();
                    EXPECT(view_fill(&ctx, cams[f], W, VH, scratch) == RT_OK, "scene %d camera %d: view_fill", scene, f);
                    view_record(scratch, rec[f]);
                    EXPECT(scratch.pw == own_lp.pw && scratch.ph == own_lp.ph && scratch.nearc == own_lp.nearc &&
                               scratch.W == own_lp.W,
                           "scene %d camera %d: the shared view plane depends on the camera", scene, f);
                }
                // the context is untouched: its camera, and the cached view of its own camera
                rt_camera now;
                rt_get_camera(&ctx, &now);
                EXPECT(same(&now, &own, sizeof now), "scene %d: the context's camera changed", scene);
                LaunchParams again;
                std::memset(&again, 0, sizeof again);
                EXPECT(view_params(&ctx, W, H, again) == RT_OK && same(&again, &own_lp, sizeof again),
                       "scene %d: the context's view changed", scene);

                for (int f = 0; f < N; ++f) {
                    rt_set_camera(&ctx, &cams[f]);
                    LaunchParams lp;
                    std::memset(&lp, 0, sizeof lp);
                    EXPECT(view_params(&ctx, W, H, lp) == RT_OK, "scene %d camera %d: view_params", scene, f);
                    EXPECT(lp.H == H, "scene %d camera %d: rows traced", scene, f);
                    compare(rec[f], lp, scene, f);
                    ++records;
                    EXPECT(rec[f].prim_const == (S <= MAX_PRIM_CONST ? 1 : 0), "scene %d: prim_const at S = %d", scene, S);
                    for (int i = 0; i < S && rec[f].prim_const; ++i)
                        if (rec[f].pbox[i].x0 > INT_MIN / 2) {
                            ++boxed_records;
                            break;
                        }
                    mirror_records += rec[f].mbox_n > 0;
                }
                EXPECT(same(&rec[0], &rec[N - 1], sizeof rec[0]), "scene %d: equal cameras, different records", scene);
                for (int f = 1; f < N - 1; ++f) differing += !same(&rec[0], &rec[f], sizeof rec[0]);
            }
    std::printf("path_host: %d scenes, %ld records, %ld with screen boxes, %ld with mirrored boxes\n", scene, records,
                boxed_records, mirror_records);
    std::printf("path_host: %ld record pairs of different cameras differ\n", differing);
}
}  // namespace

int main() {
    run();
    std::printf("path_host: %ld failures\n", failures);
    return failures == 0 && records > 0 && boxed_records > 0 && mirror_records > 0 && differing > 0 ? 0 : 1;
}
