// ss_host.cpp -- host sanitizer driver for the supersampling additions (rt_set_supersampling), TEST
// INFRASTRUCTURE ONLY.  Like san_host.cpp it compiles rt_api.cpp into this translation unit with host-side
// AddressSanitizer + UndefinedBehaviorSanitizer (built by tests/test_supersample_host.py) and drives, on
// contexts without a device:
//   * the accepted and rejected factors and the getter;
//   * the k W x k H <= 2^31 - 1 rejection of the render entry points, their argument checks with k > 1, and
//     the two RT_ERR_UNSUPPORTED paths (no device call is reached);
//   * view_params at k > 1 against rt_camera_view(k W, k H) bit for bit, and the claim the exactness of the
//     feature rests on: the view plane of the k W x k H sample frame is the W x H frame's;
//   * the shared resolve arithmetic (csrc/rt_resolve.h: unpack, add, round -- what the kernels' epilogue does
//     per lane) against a plain per-channel loop, on random 64-sample tiles.
// Exit status 0 = all checks passed; any sanitizer report aborts the process.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstdint>
#include <cstdio>

#include "../../uu-infogr-raytracer_amd/csrc/rt_resolve.h"

namespace {
int failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                   \
            std::fputc('\n', stderr);                            \
            ++failures;                                          \
        }                                                        \
    } while (0)

uint64_t rng = 0x5A3B1E5EEDull;
uint64_t next64() {
    uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float unif(float lo, float hi) { return lo + (hi - lo) * (float)((next64() >> 40) * (1.0 / 16777216.0)); }
bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void set_scene(rt_ctx& ctx) {
    rt_sphere s{};
    s.center = rt_vec3{0, 0, 5}, s.radius = 1;
    rt_light l{rt_vec3{-3, 1, -3}, 1.0f};
    CHECK(rt_set_scene(&ctx, &s, 1, nullptr, 0, &l, 1, rt_vec3{0, 0, 0}, 0) == RT_OK, "scene");
}

void check_factor() {
    rt_ctx ctx;  // no devices
    int k = -1;
    CHECK(rt_get_supersampling(&ctx, &k) == RT_OK && k == 1, "default factor %d", k);
    const int good[] = {1, 2, 4, 8, 1};
    for (int g : good) {
        CHECK(rt_set_supersampling(&ctx, g) == RT_OK, "factor %d accepted", g);
        CHECK(rt_get_supersampling(&ctx, &k) == RT_OK && k == g, "getter after %d: %d", g, k);
    }
    CHECK(rt_set_supersampling(&ctx, 4) == RT_OK, "factor 4");
    const int bad[] = {0, -1, -2, 3, 5, 6, 7, 9, 16, 64, INT_MAX, INT_MIN};
    for (int b : bad) {
        CHECK(rt_set_supersampling(&ctx, b) == RT_ERR_INVALID_ARG, "factor %d rejected", b);
        CHECK(!ctx.last_error.empty() && std::strstr(rt_last_error(&ctx), "rt_set_supersampling") != nullptr,
              "message for factor %d", b);
        CHECK(rt_get_supersampling(&ctx, &k) == RT_OK && k == 4, "a rejected factor changes nothing (%d)", k);
    }
    CHECK(rt_set_supersampling(nullptr, 2) == RT_ERR_INVALID_ARG, "NULL ctx");
    CHECK(std::strstr(rt_last_error(nullptr), "NULL") != nullptr, "NULL ctx message");
    CHECK(rt_get_supersampling(nullptr, &k) == RT_ERR_INVALID_ARG, "getter NULL ctx");
    CHECK(rt_get_supersampling(&ctx, nullptr) == RT_ERR_INVALID_ARG, "getter NULL out");
}

void check_entry_points() {
    rt_ctx ctx;
    int32_t px[4];
    rt_work work;
    CHECK(rt_set_supersampling(&ctx, 2) == RT_OK, "factor 2");
    CHECK(rt_render_device(&ctx, 2, 2, px, nullptr) == RT_ERR_NO_SCENE, "render before a scene");
    set_scene(ctx);
    // k W * k H > 2^31 - 1: 46342^2 = 2,147,580,964; 23170 * 2 = 46340 passes the size check (NULL pixels next)
    CHECK(rt_render_device(&ctx, 23171, 23171, px, nullptr) == RT_ERR_INVALID_ARG, "23171^2 at k = 2");
    CHECK(std::strstr(rt_last_error(&ctx), "supersampling") != nullptr, "overflow message: %s", rt_last_error(&ctx));
    CHECK(rt_render(&ctx, 23171, 23171, px) == RT_ERR_INVALID_ARG, "rt_render 23171^2 at k = 2");
    CHECK(rt_render_async(&ctx, 23171, 23171, px) == RT_ERR_INVALID_ARG, "rt_render_async 23171^2 at k = 2");
    CHECK(rt_render_bands_ex(&ctx, 23171, 23171, 8, 0, 1, px, RT_BANDS_INT32, nullptr, nullptr) == RT_ERR_INVALID_ARG,
          "rt_render_bands_ex 23171^2 at k = 2");
    CHECK(rt_render_bands_batch(&ctx, 23171, 23171, 8, 0, 1, 2, px, 1u << 31, RT_BANDS_INT32, nullptr, nullptr) ==
              RT_ERR_INVALID_ARG,
          "rt_render_bands_batch 23171^2 at k = 2");
    CHECK(rt_render_device(&ctx, 23170, 23170, nullptr, nullptr) == RT_ERR_INVALID_ARG &&
              std::strstr(rt_last_error(&ctx), "NULL d_pixels") != nullptr,
          "23170^2 at k = 2 passes the size check: %s", rt_last_error(&ctx));
    CHECK(rt_set_supersampling(&ctx, 8) == RT_OK, "factor 8");
    // k = 8: 8192 x 4096 is 65536 x 32768 = 2^31 samples (one too many); 4096 x 4096 is 2^30 and passes
    CHECK(rt_render_device(&ctx, 8192, 4096, px, nullptr) == RT_ERR_INVALID_ARG, "8192x4096 at k = 8");
    CHECK(std::strstr(rt_last_error(&ctx), "supersampling") != nullptr, "overflow message at k = 8");
    CHECK(rt_render_device(&ctx, 5793, 5793, px, nullptr) == RT_ERR_INVALID_ARG, "5793^2 at k = 8: 46344^2 samples");
    CHECK(rt_render_device(&ctx, 1 << 28, 1, px, nullptr) == RT_ERR_INVALID_ARG, "2^28 x 1 at k = 8: 2^34 samples");
    CHECK(rt_render_device(&ctx, 4096, 4096, nullptr, nullptr) == RT_ERR_INVALID_ARG &&
              std::strstr(rt_last_error(&ctx), "NULL d_pixels") != nullptr,
          "4096^2 at k = 8 (2^30 samples) passes the size check");
    CHECK(rt_set_supersampling(&ctx, 1) == RT_OK, "factor 1");
    CHECK(rt_render_device(&ctx, 23171, 23171, nullptr, nullptr) == RT_ERR_INVALID_ARG &&
              std::strstr(rt_last_error(&ctx), "NULL d_pixels") != nullptr,
          "k = 1: the plain size limit");
    // the argument checks as at k = 1
    CHECK(rt_set_supersampling(&ctx, 4) == RT_OK, "factor 4");
    CHECK(rt_render_device(&ctx, 0, 2, px, nullptr) == RT_ERR_INVALID_ARG, "zero width");
    CHECK(rt_render(&ctx, 2, 2, nullptr) == RT_ERR_INVALID_ARG, "rt_render NULL pixels");
    CHECK(rt_render_async(&ctx, 2, 2, nullptr) == RT_ERR_INVALID_ARG, "rt_render_async NULL pixels");
    CHECK(rt_render_bands_ex(&ctx, 8, 8, 0, 0, 1, px, RT_BANDS_INT32, nullptr, nullptr) == RT_ERR_INVALID_ARG, "band_rows 0");
    CHECK(rt_render_bands_ex(&ctx, 8, 8, 8, 0, 1, px, 7, nullptr, nullptr) == RT_ERR_INVALID_ARG, "bad format");
    CHECK(rt_render_bands(&ctx, 8, 8, 8, -1, 1, px, nullptr, nullptr) == RT_ERR_INVALID_ARG, "negative band_first");
    CHECK(rt_render_bands_batch(&ctx, 8, 8, 8, 0, 1, 0, px, 256, RT_BANDS_INT32, nullptr, nullptr) == RT_ERR_INVALID_ARG,
          "zero frames");
    CHECK(rt_render_bands_batch(&ctx, 8, 8, 8, 0, 1, 2, px, 255, RT_BANDS_INT32, nullptr, nullptr) == RT_ERR_INVALID_ARG,
          "frame stride in output pixels: 8 x 8 x 4 bytes needed");
    // out of scope while k > 1
    alignas(8) unsigned char wire[64];
    CHECK(rt_render_bands_tiles(&ctx, 8, 8, 8, 0, 1, 0, 1, 1, wire, nullptr) == RT_ERR_UNSUPPORTED, "tiles at k = 4");
    CHECK(std::strstr(rt_last_error(&ctx), "rt_render_bands_tiles") != nullptr, "tiles message");
    CHECK(rt_count_work(&ctx, 8, 8, &work) == RT_ERR_UNSUPPORTED, "rt_count_work at k = 4");
    CHECK(std::strstr(rt_last_error(&ctx), "rt_count_work") != nullptr, "count_work message");
    CHECK(rt_render_bands_tiles(nullptr, 8, 8, 8, 0, 1, 0, 1, 1, wire, nullptr) == RT_ERR_INVALID_ARG, "tiles NULL ctx");
    CHECK(rt_count_work(&ctx, 0, 8, &work) == RT_ERR_INVALID_ARG, "rt_count_work zero width");
    CHECK(rt_count_work(&ctx, 8, 8, nullptr) == RT_ERR_UNSUPPORTED, "the factor is refused before the other arguments");
}

// The view of a supersampled render: trace_bands asks view_params for the k W x k H frame (view height scaled
// too).  It must be rt_camera_view(k W, k H) bit for bit -- and its view plane the W x H frame's, since
// (float)kW / (float)kH and (float)W / (float)H are the correctly rounded quotient of the same rational
// (both operands exact in binary32 below 2^24).
void check_view() {
    rt_ctx ctx;
    set_scene(ctx);
    for (int it = 0; it < 3000; ++it) {
        const int ss = 1 + it % 3, k = 1 << ss;
        const int W = 1 + (int)(next64() % 2000), H = 1 + (int)(next64() % 1200);
        rt_camera cam{rt_vec3{unif(-3, 3), unif(-1, 2), unif(-4, 2)}, unif(-3.2f, 3.2f), unif(-1.5f, 1.5f)};
        rt_set_camera(&ctx, &cam);
        const int vh = it % 4 == 3 ? H + (int)(next64() % 50) : 0;
        CHECK(rt_set_view_height(&ctx, vh) == RT_OK, "view height");
        const int VH = vh ? vh : H;
        LaunchParams lp;
        std::memset(&lp, 0, sizeof lp);
        CHECK(view_params(&ctx, W << ss, H << ss, lp, ss) == RT_OK, "view_params: %s", ctx.last_error.c_str());
        rt_view a, b;
        CHECK(rt_camera_view(&cam, W * k, VH * k, &a) == RT_OK && rt_camera_view(&cam, W, VH, &b) == RT_OK, "views");
        const float* v[4] = {lp.cam, lp.right, lp.up, lp.fwd};
        const rt_vec3 w[4] = {a.position, a.right, a.up, a.forward};
        for (int i = 0; i < 4; ++i)
            CHECK(same_bits(v[i][0], w[i].x) && same_bits(v[i][1], w[i].y) && same_bits(v[i][2], w[i].z), "basis %d", i);
        CHECK(same_bits(lp.pw, a.plane_width) && same_bits(lp.ph, a.plane_height) && same_bits(lp.nearc, a.near_clip),
              "view plane of %dx%d at k = %d", W, VH, k);
        CHECK(same_bits(a.plane_width, b.plane_width) && same_bits(a.plane_height, b.plane_height),
              "the sample frame's view plane is the output frame's (%dx%d, k = %d)", W, VH, k);
        CHECK(lp.W == W * k && lp.H == H * k, "sample frame %dx%d", lp.W, lp.H);
    }
    // rows above the view height are refused in output pixels
    CHECK(rt_set_view_height(&ctx, 10) == RT_OK, "view height 10");
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    CHECK(view_params(&ctx, 16 << 1, 11 << 1, lp, 1) == RT_ERR_INVALID_ARG, "11 rows above a view height of 10");
    CHECK(std::strstr(ctx.last_error.c_str(), "height 11 above the view height 10") != nullptr, "%s", ctx.last_error.c_str());
    CHECK(view_params(&ctx, 16 << 1, 10 << 1, lp, 1) == RT_OK, "10 rows of a view height of 10");
}

// resolve_unpack / resolve_add / resolve_round over a tile of 64 samples (lane = ry * 8 + rx), every k x k
// block summed in any order (the kernels' butterfly is one), against the definition per channel.
void check_resolve() {
    long checked = 0;
    for (int ss = 1; ss <= 3; ++ss) {
        const int k = 1 << ss;
        for (int it = 0; it < 100000; ++it) {
            uint32_t px[64];
            const int kind = it % 8;
            for (int i = 0; i < 64; ++i) {
                const uint32_t r = (uint32_t)next64();
                px[i] = kind == 0   ? 0xffffffu                               // saturated: 64 * 255 per field
                        : kind == 1 ? ((r & 1u) ? 0x00ff00u : 0xff00ffu)        // neighbours at the extremes
                        : kind == 2 ? ((r & 0x010101u) * 0xffu)                 // each channel 0 or 255
                        : kind == 3 ? (0xfefefeu + (r & 0x010101u))             // 254 / 255
                        : kind == 4 ? (r & 0x010101u)                           // 0 / 1: ties
                                    : (r & 0xffffffu);
            }
            for (int by = 0; by < 8; by += k)
                for (int bx = 0; bx < 8; bx += k) {
                    rtk::ResolveSum sum = rtk::resolve_unpack(px[by * 8 + bx]);
                    uint32_t ch[3] = {0, 0, 0};
                    for (int j = 0; j < k; ++j)
                        for (int i = 0; i < k; ++i) {
                            const uint32_t q = px[(by + j) * 8 + bx + i];
                            if (i | j) sum = rtk::resolve_add(sum, rtk::resolve_unpack(q));
                            ch[0] += (q >> 16) & 255u, ch[1] += (q >> 8) & 255u, ch[2] += q & 255u;
                        }
                    uint32_t want = 0;
                    for (int c = 0; c < 3; ++c) want = (want << 8) | ((ch[c] + (uint32_t)(k * k / 2)) / (uint32_t)(k * k));
                    const uint32_t got = rtk::resolve_round(sum, ss);
                    CHECK(got == want, "k = %d tile %d block (%d, %d): %06x, expected %06x", k, it, bx, by, got, want);
                    ++checked;
                }
        }
    }
    for (uint32_t q : {0u, 0xffffffu, 0x123456u, 0x00ff00u})
        CHECK(rtk::resolve_round(rtk::resolve_unpack(q), 0) == q, "k = 1 is the sample itself (%06x)", q);
    std::printf("resolve: %ld blocks\n", checked);
}
}  // namespace

int main() {
    check_factor();
    check_entry_points();
    check_view();
    check_resolve();
    std::printf("ss_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
