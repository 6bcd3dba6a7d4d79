// adaptive_host.cpp -- host checks of adaptive supersampling (rt_set_adaptive_sampling), TEST INFRASTRUCTURE ONLY.
// rt_api.cpp is compiled into this translation unit (its helpers have internal linkage) with host-side ASan + UBSan,
// as shutter_host.cpp beside it is; no device call is reached (contexts without devices).
//
//  1. adapt_differs (rt_resolve.h, the function the kernels decide with) against plain integer code: all 256^2 byte
//     pairs in each channel position, and in all three at once, at T = 1, 2, 255, 256.
//  2. The argument checks of rt_set_adaptive_sampling / rt_get_adaptive_sampling.
//  3. The band-row rule on a context without devices: a refused band render comes back before any device is touched
//     (going on would index an empty vector, which ASan reports), whatever else is set.
//  4. The variant selection (rt_internal.h pick_trace_variant): shutter_host's enumeration extended by adapt_thr in
//     {0, 1, 256}, against the rules restated below; 504 descriptors, the 60 of the new mode mirroring SS's field
//     for field; with adapt_thr == 0 nothing but the 444 earlier ones, each selected as before.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// ---- 1. the difference / threshold function -------------------------------------------------------------------
long differ_cases = 0;
void check_differs() {
    static const int Ts[] = {1, 2, 255, 256};
    for (int T : Ts)
        for (int a = 0; a < 256; ++a)
            for (int b = 0; b < 256; ++b) {
                const bool want = std::abs(a - b) >= T;
                for (int sh : {16, 8, 0}) {
                    // the other two channels equal (and not zero: nothing leaks in from a neighbour)
                    const uint32_t rest = 0x00a55aa5u & ~(0xffu << sh);
                    const uint32_t pa = rest | (uint32_t)a << sh, pb = rest | (uint32_t)b << sh;
                    EXPECT(adapt_differs(pa, pb, T) == want, "adapt_differs T %d channel shift %d: %d against %d", T, sh, a, b);
                    // ... or at opposite ends with a difference of T - 1: still only this channel decides
                    const int lo = (a * 7 + b) & 255, hi = lo + T - 1 <= 255 ? lo + T - 1 : lo - (T - 1);
                    uint32_t qa = (uint32_t)a << sh, qb = (uint32_t)b << sh;
                    if (hi >= 0)
                        for (int o : {16, 8, 0})
                            if (o != sh) qa |= (uint32_t)lo << o, qb |= (uint32_t)hi << o;
                    EXPECT(adapt_differs(qa, qb, T) == want, "adapt_differs T %d shift %d beside T - 1: %d against %d", T, sh, a, b);
                    differ_cases += 2;
                }
                const uint32_t ga = (uint32_t)a * 0x010101u, gb = (uint32_t)b * 0x010101u;  // all three at once
                EXPECT(adapt_differs(ga, gb, T) == want, "adapt_differs T %d grey: %d against %d", T, a, b);
                ++differ_cases;
            }
    // bits 24-31 of a pixel play no part
    EXPECT(!adapt_differs(0xff102030u, 0x00102030u, 1), "the top byte is ignored");
}

// ---- 2. / 3. the calls and the band-row rule ------------------------------------------------------------------
rt_vec3 v3(float x, float y, float z) { return rt_vec3{x, y, z}; }
bool small_scene(rt_ctx* ctx) {
    rt_material m;
    std::memset(&m, 0, sizeof m);
    m.kd = m.ka = v3(0.6f, 0.6f, 0.6f);
    rt_sphere sph[2];
    sph[0].center = v3(0, 0, 6), sph[0].radius = 1.0f, sph[0].material = m;
    sph[1].center = v3(2, 0.5f, 7), sph[1].radius = 0.5f, sph[1].material = m;
    rt_plane pl[1];
    pl[0].material = m, pl[0].normal = v3(0, 1, 0), pl[0].center = v3(0, -1, 0);
    rt_light li[1] = {{v3(0, 10, 0), 1.0f}};
    return rt_set_scene(ctx, sph, 2, pl, 1, li, 1, v3(0.1f, 0.1f, 0.1f), 2) == RT_OK;
}

long arg_checks = 0, band_checks = 0;
void check_calls() {
    rt_ctx ctx;
    int t = -7;
    EXPECT(rt_get_adaptive_sampling(&ctx, &t) == RT_OK && t == 0, "the default is 0 (off)");
    for (int bad : {-1, 257, 258, 1000, INT_MIN, INT_MAX}) {
        ++arg_checks;
        EXPECT(rt_set_adaptive_sampling(&ctx, bad) == RT_ERR_INVALID_ARG, "threshold %d", bad);
        EXPECT(std::strstr(rt_last_error(&ctx), "rt_set_adaptive_sampling") != nullptr, "the error names the call");
        EXPECT(rt_get_adaptive_sampling(&ctx, &t) == RT_OK && t == 0, "a refused threshold changes nothing");
    }
    for (int ok : {1, 16, 255, 256, 0}) {
        ++arg_checks;
        EXPECT(rt_set_adaptive_sampling(&ctx, ok) == RT_OK, "threshold %d", ok);
        EXPECT(rt_get_adaptive_sampling(&ctx, &t) == RT_OK && t == ok, "threshold %d reads back", ok);
    }
    arg_checks += 3;
    EXPECT(rt_set_adaptive_sampling(nullptr, 16) == RT_ERR_INVALID_ARG, "NULL context");
    EXPECT(std::strstr(rt_last_error(nullptr), "rt_set_adaptive_sampling") != nullptr, "the error names the call");
    t = 9;
    EXPECT(rt_get_adaptive_sampling(nullptr, &t) == RT_ERR_INVALID_ARG && t == 9, "NULL context");
    EXPECT(std::strstr(rt_last_error(nullptr), "rt_get_adaptive_sampling") != nullptr, "the error names the call");
    EXPECT(rt_get_adaptive_sampling(&ctx, nullptr) == RT_ERR_INVALID_ARG, "NULL out");
    // the setting is independent of the factor: stored at k = 1, kept across a change of k
    EXPECT(rt_set_adaptive_sampling(&ctx, 48) == RT_OK && rt_set_supersampling(&ctx, 4) == RT_OK &&
               rt_set_supersampling(&ctx, 1) == RT_OK && rt_get_adaptive_sampling(&ctx, &t) == RT_OK && t == 48,
           "the threshold survives a change of the factor");

    // the rule itself
    for (int H : {1, 7, 8, 9, 30, 1080})
        for (int br = 1; br <= 1100; ++br) {
            const bool want = br % 8 == 0 || br >= H;
            EXPECT(adaptive_band_ok(br, H) == want, "adaptive_band_ok(%d, %d)", br, H);
            ++band_checks;
        }
    // through the band renders, on a context with a scene and no device
    EXPECT(small_scene(&ctx), "rt_set_scene: %s", ctx.last_error.c_str());
    static int32_t out[64];
    int nb = 77;
    auto ex = [&](int band_rows, int H, int fmt) {
        ++band_checks;
        return rt_render_bands_ex(&ctx, 8, H, band_rows, 0, 1, out, fmt, nullptr, &nb);
    };
    auto batch = [&](int band_rows, int H, int fmt) {
        ++band_checks;
        return rt_render_bands_batch(&ctx, 8, H, band_rows, 0, 1, 2, out, 1 << 20, fmt, nullptr, &nb);
    };
    for (int k : {2, 4, 8})
        for (int T : {1, 16, 256}) {
            EXPECT(rt_set_supersampling(&ctx, k) == RT_OK && rt_set_adaptive_sampling(&ctx, T) == RT_OK, "k %d T %d", k, T);
            for (int fmt : {RT_BANDS_INT32, RT_BANDS_RGB24, RT_BANDS_FRAME})
                for (int br : {1, 3, 7, 9, 12, 15, 17, 29}) {
                    EXPECT(ex(br, 30, fmt) == RT_ERR_UNSUPPORTED, "rt_render_bands_ex band_rows %d of 30 rows, k %d T %d", br, k, T);
                    EXPECT(batch(br, 30, fmt) == RT_ERR_UNSUPPORTED, "rt_render_bands_batch band_rows %d of 30 rows", br);
                    EXPECT(std::strstr(rt_last_error(&ctx), "adaptive") != nullptr, "the error says why");
                }
            // what is an invalid argument stays one
            EXPECT(ex(0, 30, RT_BANDS_INT32) == RT_ERR_INVALID_ARG && ex(12, 30, 99) == RT_ERR_INVALID_ARG, "bad band arguments");
        }
    EXPECT(nb == 77, "a refused call leaves out_n_bands alone");
    for (int32_t v : out) EXPECT(v == 0, "a refused call writes nothing");
    // several workers: the refusal of a band render on such a context comes first or second, never a launch
    ctx.n_gpus = 2;
    EXPECT(ex(12, 30, RT_BANDS_INT32) != RT_OK, "two workers");
    ctx.n_gpus = 1;
}

// ---- 4. variant selection -------------------------------------------------------------------------------------
using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// The selection as it was before the adaptive mode (shutter_host's restatement, thresholds as literals).
bool expect_before(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    const bool tiles = p.out_fmt == 3;
    const int sl = p.shutter_log2;
    if (sl != 0 && p.views == nullptr) return false;
    if (sl < 0 || sl > 8) return false;
    int mode;
    if (p.views != nullptr) {
        if (p.ss_log2 > 0 || tiles || stats || p.tile_order != nullptr || p.tile_cost != nullptr || p.copy_z != 0 ||
            p.row_order_n != 0 || p.col_major != 0)
            return false;
        mode = sl > 0 ? 5 : 4;  // SHUTTER : PATH
    } else if (p.ss_log2 > 0) {
        if (p.ss_log2 > 3 || tiles || stats || p.tile_order != nullptr || p.tile_cost != nullptr) return false;
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
// With the threshold: a launch that selected SS selects ADAPT (6) when adapt_thr > 0; nothing else changes.
bool expect(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (!expect_before(p, gpow, stats, v)) return false;
    if (v->mode == 3 && p.adapt_thr > 0) v->mode = 6;
    return true;
}

long long variant_cases = 0, variant_refused = 0;
size_t n_descriptors = 0, n_adapt = 0, n_before = 0;
int n_built = 0;
void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 8, 9}, thrs[] = {0, 1, 256};
    static uint32_t cell[2];
    static DevView view;
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    long long mismatches = 0;
    std::set<Key> seen, seen0;  // every adapt_thr; adapt_thr == 0 alone
    std::map<unsigned, Key> word_of;
    for (int thr : thrs) for (int sl : sls)
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
        p.adapt_thr = thr;
        p.n_frames = nf, p.copy_z = cz;
        p.tile_order = to ? &cell[0] : nullptr, p.tile_cost = tc ? &cell[1] : nullptr;
        p.row_order_n = ro ? 2 : 0, p.col_major = cm;
        TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
        const bool w = expect(p, gpow != 0, stats != 0, &want), g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
        ++variant_cases;
        if (!w) ++variant_refused;
        if (w != g || (w && key_of(want) != key_of(got))) {
            if (mismatches++ < 10)
                std::fprintf(stderr, "adaptive_host: MISMATCH thr %d sl %d S %d L %d a2 %d limit %d gpow %d stats %d fmt %d ss %d "
                             "views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d %d %d %d}\n",
                             thr, sl, S, L, a2, limit, gpow, stats, fmt, ss, views, nf, cz, to, tc, ro, cm, (int)w, want.family,
                             want.gpow, want.mode, want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow,
                             got.mode, got.cls, got.K, got.wpg, got.tord);
            continue;
        }
        // the threshold changes no refusal, and nothing but the mode of a supersampling launch
        TraceVariant at0{-3, -3, -3, -3, -3, -3, -3};
        p.adapt_thr = 0;
        const bool g0 = pick_trace_variant(p, gpow != 0, stats != 0, &at0);
        p.adapt_thr = thr;
        EXPECT(g0 == g, "the threshold changes no refusal");
        if (!g) continue;
        EXPECT((got.mode == TM_ADAPT) == (thr > 0 && ss > 0 && !views), "the ADAPT mode exactly when ss_log2 > 0 and adapt_thr > 0");
        if (got.mode != TM_ADAPT) EXPECT(key_of(at0) == key_of(got), "any other launch selects what it selects at threshold 0");
        else EXPECT(at0.mode == TM_SS, "an ADAPT launch is an SS launch at threshold 0");
        seen.insert(key_of(got));
        if (thr == 0) seen0.insert(key_of(got));
        EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
        const unsigned word = variant_word(got);
        const Key nok{got.family, got.gpow, got.mode, got.cls, 0, got.wpg, got.tord};
        const auto it = word_of.emplace((unsigned)got.family << 31 | word, nok).first;
        EXPECT(it->second == nok, "one variant word per descriptor");
        EXPECT(((word & VF_ADAPT) != 0) == (got.mode == TM_ADAPT) && ((word & VF_SS) != 0) == (got.mode == TM_SS) &&
                   vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg && vf_tord_of(word) == got.tord,
               "the variant word reads back");
    }
    // thresholds outside 0..256 on a supersampling launch: refused
    p.views = nullptr, p.shutter_log2 = 0, p.out_fmt = 0, p.tile_order = nullptr, p.tile_cost = nullptr, p.ss_log2 = 1;
    for (int bad : {-1, 257, INT_MIN, INT_MAX}) {
        TraceVariant v;
        p.adapt_thr = bad;
        EXPECT(!pick_trace_variant(p, false, false, &v), "adapt_thr %d is refused", bad);
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_descriptors = seen.size(), n_before = seen0.size();
    EXPECT(seen.size() == 504, "504 distinct descriptors, got %zu", seen.size());
    EXPECT(seen0.size() == 444, "444 descriptors with adapt_thr == 0, got %zu", seen0.size());
    for (const Key& k : seen0) EXPECT(std::get<2>(k) != TM_ADAPT, "no ADAPT descriptor without a threshold");
    for (const Key& k : seen) EXPECT(std::get<2>(k) == TM_ADAPT || seen0.count(k) == 1, "a threshold adds ADAPT descriptors only");
    // the new descriptors mirror SS's, field for field but the mode
    size_t n_ss = 0;
    int per_entry[2][2] = {};
    for (const Key& k : seen) {
        Key twin = k;
        if (std::get<2>(k) == TM_ADAPT) {
            ++n_adapt;
            per_entry[std::get<0>(k)][std::get<1>(k)]++;
            std::get<2>(twin) = TM_SS;
            EXPECT(seen.count(twin) == 1, "an ADAPT descriptor without its SS twin");
        } else if (std::get<2>(k) == TM_SS) {
            ++n_ss;
            std::get<2>(twin) = TM_ADAPT;
            EXPECT(seen.count(twin) == 1, "an SS descriptor without its ADAPT twin");
        }
    }
    EXPECT(n_adapt == 60 && n_ss == 60, "60 ADAPT and 60 SS descriptors, got %zu and %zu", n_adapt, n_ss);
    EXPECT(per_entry[0][0] == 12 && per_entry[0][1] == 12 && per_entry[1][0] == 18 && per_entry[1][1] == 18,
           "direct 12 + 12 GPOW, bundle 18 + 18 GPOW");
    // trace_variant_built admits exactly these, over every value a field takes
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m < 7; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built == 504, "504 built descriptors, got %d", n_built);
}
}  // namespace

int main() {
    check_differs();
    check_calls();
    check_variants();
    std::printf("adaptive_host: %ld difference cases\n", differ_cases);
    std::printf("adaptive_host: %ld argument checks, %ld band checks\n", arg_checks, band_checks);
    std::printf("adaptive_host: %lld variant cases, %lld refused, %zu descriptors (%zu without a threshold, %zu ADAPT), %d built\n",
                variant_cases, variant_refused, n_descriptors, n_before, n_adapt, n_built);
    std::printf("adaptive_host: %ld failures\n", failures);
    return failures == 0 && differ_cases > 0 && arg_checks > 0 && band_checks > 0 ? 0 : 1;
}
