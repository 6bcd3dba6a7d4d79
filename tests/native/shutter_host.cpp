// shutter_host.cpp -- host checks of the camera-path shutter (rt_render_shutter_bands / rt_render_shutter), TEST
// INFRASTRUCTURE ONLY.  rt_api.cpp is compiled into this translation unit (its helpers have internal linkage) with
// host-side ASan + UBSan, as path_host.cpp beside it is; no device call is reached (contexts without devices).
//
//  1. resolve_round_n (rt_resolve.h) against plain per-channel integer arithmetic: t = 1..8, every channel sum at
//     and next to the rounding boundaries and the field's maximum, all three channels at once.
//  2. The variant selection (rt_internal.h pick_trace_variant): variant_host's enumeration extended by
//     shutter_log2 in {0, 1, 8, 9}, against the rules restated below; 444 descriptors, the 60 of the new mode
//     mirroring PATH's field for field; with shutter_log2 == 0 nothing but the 384 earlier ones.
//  3. The argument checks of both entry points on a context without devices: each refusal comes before any device
//     call (the context has no device to call: going on would index an empty vector, which ASan reports).
//  4. The view table (rt_api.cpp view_table_fill, the code trace_path fills a launch's table with): record
//     f * m + s is the view of cameras[f * m + s], byte for byte, for m = 4 and a random scene with mirror planes.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>

#include "../../uu-infogr-raytracer_amd/csrc/rt_resolve.h"

namespace {
long failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            if (failures++ < 30) {             \
                std::fprintf(stderr, "FAIL "); \
                std::fprintf(stderr, __VA_ARGS__); \
                std::fprintf(stderr, "\n");    \
            }                                  \
        }                                      \
    } while (0)

// ---- 1. resolve_round_n ------------------------------------------------------------------------------------
long resolve_cases = 0;
void check_resolve() {
    for (int t = 1; t <= 8; ++t) {
        const int m = 1 << t, half = m / 2, top = m * 255;
        std::set<int> sums = {0, 1, top - 1, top};
        for (int q : {0, 1, 2, 127, 128, 253, 254, 255})  // the sums that round to q from below: q * m - half .. + half - 1
            for (int d = -1; d <= 1; ++d)
                for (int edge : {q * m - half, q * m + half, q * m}) {
                    const int s = edge + d;
                    if (s >= 0 && s <= top) sums.insert(s);
                }
        for (int r : sums) for (int g : sums) for (int b : sums) {
            const ResolveSum sum{(uint32_t)r << 16 | (uint32_t)b, (uint32_t)g};
            const uint32_t want = (uint32_t)((r + half) / m) << 16 | (uint32_t)((g + half) / m) << 8 | (uint32_t)((b + half) / m);
            const uint32_t got = resolve_round_n(sum, t);
            EXPECT(got == want, "resolve_round_n t %d sums %d %d %d: %06x, expected %06x", t, r, g, b, got, want);
            ++resolve_cases;
        }
        // sums of real pixels: m copies of one pixel come back as that pixel, and the mean of unpacked adds is exact
        ResolveSum acc{0u, 0u};
        for (int i = 0; i < m; ++i) acc = resolve_add(acc, resolve_unpack(0x00ff80ffu));
        EXPECT(resolve_round_n(acc, t) == 0x00ff80ffu, "t %d: %d equal pixels", t, m);
    }
    EXPECT(resolve_round_n(resolve_unpack(0x00123456u), 0) == 0x00123456u, "t 0 is the pixel itself");
}

// ---- 2. variant selection ----------------------------------------------------------------------------------
using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// The rules, restated with the thresholds as literals: false = refused.  `sl` = 0 is the selection as it was
// before the shutter existed.
bool expect(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    const bool tiles = p.out_fmt == 3;
    const int sl = p.shutter_log2;
    if (sl != 0 && p.views == nullptr) return false;
    if (sl < 0 || sl > 8) return false;
    int mode;
    if (p.views != nullptr) {
        if (p.ss_log2 > 0) return false;
        if (tiles) return false;
        if (stats) return false;
        if (p.tile_order != nullptr) return false;
        if (p.tile_cost != nullptr) return false;
        if (p.copy_z != 0) return false;
        if (p.row_order_n != 0) return false;
        if (p.col_major != 0) return false;
        mode = sl > 0 ? 5 : 4;  // SHUTTER : PATH
    } else if (p.ss_log2 > 0) {
        if (p.ss_log2 > 3) return false;
        if (tiles) return false;
        if (stats) return false;
        if (p.tile_order != nullptr) return false;
        if (p.tile_cost != nullptr) return false;
        mode = 3;  // SS
    } else if (tiles) {
        mode = 2;
    } else if (stats) {
        mode = 1;
    } else {
        mode = 0;
    }
    int K;
    if (p.limit <= 0) K = 1;
    else if (p.limit == 1) K = 2;
    else if (p.limit <= 3) K = 4;
    else if (p.limit <= 5) K = 6;
    else if (p.limit <= 7) K = 8;
    else K = 64;
    int family, cls, wpg = 1, tord = 0;
    if (p.S >= 12) {
        family = 1;  // bundle
        if (p.S <= 64 && p.L >= 1 && p.L <= 4 && p.lights_a2_ok) cls = 2;
        else if (p.S <= 64 && p.L >= 1 && p.L <= 4) cls = 1;
        else cls = 0;
        if (cls == 2 && mode == 0 && !gpow) {
            if (p.tile_cost != nullptr) tord = 2;
            else if (p.tile_order != nullptr) tord = 1;
        }
    } else {
        family = 0;  // direct
        cls = p.S <= 8 ? 8 : 0;
        if (mode == 0 && p.n_frames <= 1 && p.copy_z == 0) {
            wpg = 4;
            if (p.tile_cost != nullptr) tord = 2;
            else if (p.tile_order != nullptr) tord = 1;
        }
    }
    *v = TraceVariant{family, gpow ? 1 : 0, mode, cls, K, wpg, tord};
    return true;
}

long long variant_cases = 0, variant_refused = 0;
size_t n_descriptors = 0, n_shutter = 0, n_before = 0;
int n_built = 0;
void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 8, 9};
    static uint32_t cell[2];
    static DevView view;
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    long long mismatches = 0;
    std::set<Key> seen, seen0;  // every shutter_log2; shutter_log2 == 0 alone
    std::map<unsigned, Key> word_of;
    for (int sl : sls)
    for (int S : Ss) for (int L : Ls) for (int a2 = 0; a2 < 2; ++a2) for (int limit : limits)
    for (int gpow = 0; gpow < 2; ++gpow) for (int stats = 0; stats < 2; ++stats) for (int fmt = 0; fmt < 2; ++fmt)
    for (int ss = 0; ss <= 4; ++ss) for (int views = 0; views < 2; ++views) for (int nf = 1; nf <= 2; ++nf)
    for (int cz = 0; cz < 2; ++cz) for (int to = 0; to < 2; ++to) for (int tc = 0; tc < 2; ++tc)
    for (int ro = 0; ro < 2; ++ro) for (int cm = 0; cm < 2; ++cm) {
        p.S = S, p.L = L, p.lights_a2_ok = a2, p.limit = limit;
        p.out_fmt = fmt ? OUT_TILES : 0;
        p.ss_log2 = ss;
        p.views = views ? &view : nullptr;
        p.shutter_log2 = sl;
        p.n_frames = nf, p.copy_z = cz;
        p.tile_order = to ? &cell[0] : nullptr, p.tile_cost = tc ? &cell[1] : nullptr;
        p.row_order_n = ro ? 2 : 0, p.col_major = cm;
        TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
        const bool w = expect(p, gpow != 0, stats != 0, &want), g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
        ++variant_cases;
        if (!w) ++variant_refused;
        // the refusals the shutter adds, stated on their own
        if (sl == 9) EXPECT(!g, "shutter_log2 9 is refused");
        if (sl > 0 && !views) EXPECT(!g, "a shutter without a view table is refused");
        if (sl > 0 && (ss > 0 || fmt || stats || to || tc || cz || ro || cm)) EXPECT(!g, "a shutter refuses what PATH refuses");
        if (w != g || (w && key_of(want) != key_of(got))) {
            if (mismatches++ < 10)
                std::fprintf(stderr, "shutter_host: MISMATCH sl %d S %d L %d a2 %d limit %d gpow %d stats %d fmt %d ss %d views %d "
                             "nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d %d %d %d}\n",
                             sl, S, L, a2, limit, gpow, stats, fmt, ss, views, nf, cz, to, tc, ro, cm, (int)w, want.family,
                             want.gpow, want.mode, want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow,
                             got.mode, got.cls, got.K, got.wpg, got.tord);
            continue;
        }
        if (!g) continue;
        EXPECT((got.mode == TM_SHUTTER) == (sl > 0), "the SHUTTER mode exactly when shutter_log2 > 0");
        seen.insert(key_of(got));
        if (sl == 0) seen0.insert(key_of(got));
        EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
        const unsigned word = variant_word(got);
        const Key nok{got.family, got.gpow, got.mode, got.cls, 0, got.wpg, got.tord};
        const auto it = word_of.emplace((unsigned)got.family << 31 | word, nok).first;
        EXPECT(it->second == nok, "one variant word per descriptor");
        EXPECT(((word & VF_SHUTTER) != 0) == (got.mode == TM_SHUTTER) && ((word & VF_PATH) != 0) == (got.mode == TM_PATH),
               "the variant word reads back");
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_descriptors = seen.size(), n_before = seen0.size();
    EXPECT(seen.size() == 444, "444 distinct descriptors, got %zu", seen.size());
    EXPECT(seen0.size() == 384, "384 descriptors with shutter_log2 == 0, got %zu", seen0.size());
    for (const Key& k : seen0) EXPECT(std::get<2>(k) != TM_SHUTTER, "no SHUTTER descriptor without a shutter");
    // the new descriptors mirror PATH's, field for field but the mode
    size_t n_path = 0;
    for (const Key& k : seen) {
        Key twin = k;
        if (std::get<2>(k) == TM_SHUTTER) {
            ++n_shutter;
            std::get<2>(twin) = TM_PATH;
            EXPECT(seen.count(twin) == 1, "a SHUTTER descriptor without its PATH twin");
        } else if (std::get<2>(k) == TM_PATH) {
            ++n_path;
            std::get<2>(twin) = TM_SHUTTER;
            EXPECT(seen.count(twin) == 1, "a PATH descriptor without its SHUTTER twin");
        }
    }
    EXPECT(n_shutter == 60 && n_path == 60, "60 SHUTTER and 60 PATH descriptors, got %zu and %zu", n_shutter, n_path);
    // trace_variant_built admits exactly these, over every value a field takes
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m < 6; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built == 444, "444 built descriptors, got %d", n_built);
}

// ---- 3. argument checks, 4. the view table -----------------------------------------------------------------
uint64_t rng = 0x5A077E4ull;
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
// A random scene of 7 spheres over a mirror floor and a mirror wall (the mirrored screen boxes are built).
bool random_scene(rt_ctx* ctx) {
    rt_sphere sph[7];
    for (rt_sphere& s : sph) {
        s.center = v3(unif(-8, 8), unif(-1, 3), unif(-8, 8));
        s.radius = unif(0.05f, 1.2f);
        s.material = material((next64() & 3) == 0);
    }
    rt_plane pl[2];
    pl[0].material = pl[1].material = material(true);
    pl[0].normal = v3(0, 1, 0), pl[0].center = v3(0, unif(-2.0f, -0.5f), 0);
    pl[1].normal = v3(0, 0, -1), pl[1].center = v3(0, 0, 12);
    rt_light li[2] = {{v3(0, 10, 0), 1.0f}, {v3(4, 8, -3), 0.7f}};
    return rt_set_scene(ctx, sph, 7, pl, 2, li, 2, v3(0.1f, 0.1f, 0.1f), 3) == RT_OK;
}

long arg_checks = 0;
void check_arguments() {
    rt_ctx ctx;  // no devices: whatever passes the checks would index ctx.dev[0]
    EXPECT(random_scene(&ctx), "rt_set_scene: %s", ctx.last_error.c_str());
    static rt_camera cams[8];
    for (rt_camera& c : cams) c = random_camera();
    static int32_t out[8 * 8 * 4];
    int nb = 77;
    auto bands = [&](const rt_camera* c, int n, int shutter) {
        ++arg_checks;
        return rt_render_shutter_bands(&ctx, 8, 8, c, n, shutter, 8, 0, 1, out, 8 * 8 * 4, RT_BANDS_INT32, nullptr, &nb);
    };
    auto whole = [&](const rt_camera* c, int n, int shutter, int32_t* px) {
        ++arg_checks;
        return rt_render_shutter(&ctx, 8, 8, c, n, shutter, px);
    };
    for (int shutter : {0, -1, -2, 3, 5, 6, 12, 255, 257, 512, 1 << 20, INT_MIN, INT_MAX}) {
        EXPECT(bands(cams, 1, shutter) == RT_ERR_INVALID_ARG, "rt_render_shutter_bands: shutter %d", shutter);
        EXPECT(whole(cams, 1, shutter, out) == RT_ERR_INVALID_ARG, "rt_render_shutter: shutter %d", shutter);
    }
    // n_frames * shutter above RT_MAX_PATH_FRAMES (65,535): 256 x 256 = 65,536, and products that overflow an int
    static const int over[][2] = {{256, 256}, {32768, 2}, {65535, 2}, {16384, 4}, {INT_MAX, 256}, {1 << 24, 256}};
    for (const auto& o : over) {
        const int n = o[0], shutter = o[1];
        EXPECT(bands(cams, n, shutter) == RT_ERR_INVALID_ARG, "rt_render_shutter_bands: %d frames x %d", n, shutter);
        EXPECT(whole(cams, n, shutter, out) == RT_ERR_INVALID_ARG, "rt_render_shutter: %d frames x %d", n, shutter);
    }
    // what check_path and check_band_args refuse, through the new entry points (every valid shutter, 1 included)
    for (int shutter : {1, 2, 256}) {
        EXPECT(bands(nullptr, 1, shutter) == RT_ERR_INVALID_ARG, "NULL cameras");
        EXPECT(bands(cams, 0, shutter) == RT_ERR_INVALID_ARG && bands(cams, -3, shutter) == RT_ERR_INVALID_ARG, "no frames");
        EXPECT(whole(nullptr, 1, shutter, out) == RT_ERR_INVALID_ARG && whole(cams, 0, shutter, out) == RT_ERR_INVALID_ARG,
               "rt_render_shutter: NULL cameras / no frames");
        EXPECT(whole(cams, 1, shutter, nullptr) == RT_ERR_INVALID_ARG, "NULL pixels");
        ++arg_checks;
        EXPECT(rt_render_shutter_bands(&ctx, 8, 8, cams, 1, shutter, 8, 0, 1, nullptr, 256, RT_BANDS_INT32, nullptr, &nb) ==
                   RT_ERR_INVALID_ARG, "NULL d_out");
        ++arg_checks;
        EXPECT(rt_render_shutter_bands(&ctx, 8, 8, cams, 1, shutter, 0, 0, 1, out, 256, RT_BANDS_INT32, nullptr, &nb) ==
                   RT_ERR_INVALID_ARG, "band_rows 0");
        ++arg_checks;
        EXPECT(rt_render_shutter_bands(&ctx, 8, 8, cams, 2, shutter, 8, 0, 1, out, 8 * 8 * 4 - 4, RT_BANDS_INT32, nullptr, &nb) ==
                   RT_ERR_INVALID_ARG, "a frame stride below a frame's output");
        ++arg_checks;
        EXPECT(rt_render_shutter_bands(nullptr, 8, 8, cams, 1, shutter, 8, 0, 1, out, 256, RT_BANDS_INT32, nullptr, &nb) ==
                   RT_ERR_INVALID_ARG, "NULL context");
        ++arg_checks;
        EXPECT(rt_render_shutter(nullptr, 8, 8, cams, 1, shutter, out) == RT_ERR_INVALID_ARG, "NULL context");
    }
    // supersampling: unsupported, as for paths; back at k = 1 the refusal is gone (checked on the GPU)
    EXPECT(rt_set_supersampling(&ctx, 2) == RT_OK, "rt_set_supersampling");
    for (int shutter : {1, 2, 256}) {
        EXPECT(bands(cams, 2, shutter) == RT_ERR_UNSUPPORTED, "supersampling, shutter %d", shutter);
        EXPECT(whole(cams, 2, shutter, out) == RT_ERR_UNSUPPORTED, "supersampling, shutter %d", shutter);
    }
    EXPECT(bands(cams, 1, 3) == RT_ERR_INVALID_ARG, "a bad shutter is an invalid argument whatever the supersampling");
    EXPECT(rt_set_supersampling(&ctx, 1) == RT_OK, "rt_set_supersampling");
    // contexts of several workers
    ctx.n_gpus = 2;
    for (int shutter : {1, 2, 256}) {
        EXPECT(bands(cams, 2, shutter) == RT_ERR_INVALID_ARG, "two workers, shutter %d", shutter);
        EXPECT(whole(cams, 2, shutter, out) == RT_ERR_INVALID_ARG, "two workers, shutter %d", shutter);
    }
    ctx.n_gpus = 1;
    EXPECT(nb == 77, "a refused call leaves out_n_bands alone");
    for (int32_t v : out) EXPECT(v == 0, "a refused call writes nothing");
}

long table_records = 0, table_differing = 0;
bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }
void check_view_table() {
    for (int round = 0; round < 4; ++round) {
        rt_ctx ctx;
        EXPECT(random_scene(&ctx), "rt_set_scene: %s", ctx.last_error.c_str());
        const int W = round % 2 ? 1920 : 333, H = round % 2 ? 1080 : 250, VH = round >= 2 ? H + 37 : H;
        if (round >= 2) rt_set_view_height(&ctx, VH);
        constexpr int M = 4, F = 3, N = F * M;
        rt_camera cams[N];
        for (rt_camera& c : cams) c = random_camera();
        DevView table[N];
        std::memset(table, 0xA5, sizeof table);
        LaunchParams lp;
        std::memset(&lp, 0, sizeof lp);
        EXPECT(view_table_fill(&ctx, cams, N, W, VH, lp, table) == RT_OK, "view_table_fill: %s", ctx.last_error.c_str());
        for (int f = 0; f < F; ++f)
            for (int s = 0; s < M; ++s) {
                // view_record of cameras[f * m + s], built on its own ...
                LaunchParams one;
                std::memset(&one, 0, sizeof one);
                DevView rec;
                std::memset(&rec, 0x5A, sizeof rec);
                EXPECT(view_fill(&ctx, cams[f * M + s], W, VH, one) == RT_OK, "view_fill");
                view_record(one, rec);
                EXPECT(same(&table[f * M + s], &rec, sizeof rec), "round %d: record %d x %d + %d", round, f, M, s);
                // ... and the view a one-camera launch of that camera carries
                rt_set_camera(&ctx, &cams[f * M + s]);
                LaunchParams own;
                std::memset(&own, 0, sizeof own);
                EXPECT(view_params(&ctx, W, H, own) == RT_OK, "view_params");
                const DevView& v = table[f * M + s];
                EXPECT(same(v.cam, own.cam, sizeof v.cam) && same(v.fwd, own.fwd, sizeof v.fwd) && same(v.pc, own.pc, sizeof v.pc) &&
                           same(v.pbox, own.pbox, sizeof v.pbox) && v.mbox_n == own.mbox_n && same(v.mbox, own.mbox, sizeof v.mbox),
                       "round %d: record %d against the one-camera launch", round, f * M + s);
                ++table_records;
                if (f * M + s > 0) table_differing += !same(&table[0], &v, sizeof v);
            }
    }
}
}  // namespace

int main() {
    check_resolve();
    check_variants();
    check_arguments();
    check_view_table();
    std::printf("shutter_host: %ld resolve cases\n", resolve_cases);
    std::printf("shutter_host: %lld variant cases, %lld refused, %zu descriptors (%zu without a shutter, %zu SHUTTER), %d built\n",
                variant_cases, variant_refused, n_descriptors, n_before, n_shutter, n_built);
    std::printf("shutter_host: %ld argument checks\n", arg_checks);
    std::printf("shutter_host: %ld table records, %ld differ from record 0\n", table_records, table_differing);
    std::printf("shutter_host: %ld failures\n", failures);
    return failures == 0 && resolve_cases > 0 && arg_checks > 0 && table_records == 48 && table_differing == 44 ? 0 : 1;
}
