// anim_host.cpp -- host check of scene tracks (rt_set_scene_track / rt_render_anim*), TEST
// INFRASTRUCTURE ONLY.  rt_api.cpp is compiled into this translation unit (its helpers have internal linkage) with
// host-side ASan + UBSan; no device call is reached (contexts without devices).
//  1. Variant selection (rt_internal.h pick_trace_variant) against a restatement: the grid of progressive_host with
//     scene_stride = 0 -- 564 descriptors, each selected as before -- and with the stride set: the launches that
//     selected PATH select ANIM, 60 descriptors split over the four entry points as PATH's are, 624 in all, 624 built;
//     a stride with a shutter, without views or off the 256-byte grid is refused.
//  2. rt_scene.h track_build on three tracks (S = 8 direct; S = 64 bundle with grids and clusters; S = 3, P = 2 with an
//     odd sphere count): slice f of the image equals scene_build(frame f)'s host_blob byte for byte, the layout fields
//     equal its layout, and the build by a thread pool equals the serial one.
//  3. The launch scalars of mixed tracks: a light at the origin in one frame clears lights_a2_ok for the track, a
//     general exponent in one frame sets generic_pow.
//  4. Every refusal of rt_set_scene_track and of the renders, in the documented order.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>

namespace {
long failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, "FAIL ");     \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
            ++failures;                        \
        }                                      \
    } while (0)

uint64_t rng = 0xA171A7EDull;
uint64_t next64() {
    uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float unif(float lo, float hi) { return lo + (hi - lo) * (float)((next64() >> 40) * (1.0 / 16777216.0)); }
rt_vec3 v3(float x, float y, float z) { return rt_vec3{x, y, z}; }

// ---- 1. variant selection ------------------------------------------------------------------------------------------
using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// The selection restated, thresholds and mode numbers as literals: as it was (the stride ignored) ...
bool expect_before(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    const bool tiles = p.out_fmt == 3, ordered = p.tile_order != nullptr || p.tile_cost != nullptr;
    const int sl = p.shutter_log2;
    if (sl != 0 && (p.views == nullptr || sl < 0 || sl > 8)) return false;
    if (p.prog_acc != nullptr) {
        if (p.views != nullptr || p.ss_log2 < 1 || p.ss_log2 > 3 || p.adapt_thr != 0) return false;
        if (p.prog_first < 0 || p.prog_n < 0 || p.prog_n > 2) return false;
        const int total = p.prog_first + p.prog_n;
        if (total < 1 || total > 1 << (2 * p.ss_log2)) return false;
    }
    int mode;
    if (p.views != nullptr) {
        if (p.ss_log2 > 0 || tiles || stats || ordered || p.copy_z != 0 || p.row_order_n != 0 || p.col_major != 0) return false;
        mode = sl > 0 ? 5 : 4;
    } else if (p.ss_log2 > 0) {
        if (p.ss_log2 > 3 || tiles || stats || ordered || p.adapt_thr < 0 || p.adapt_thr > 256) return false;
        mode = p.prog_acc != nullptr ? 7 : p.adapt_thr > 0 ? 6 : 3;
    } else {
        mode = tiles ? 2 : stats ? 1 : 0;
    }
    const int K = p.limit <= 0 ? 1 : p.limit == 1 ? 2 : p.limit <= 3 ? 4 : p.limit <= 5 ? 6 : p.limit <= 7 ? 8 : 64;
    int family, cls, wpg = 1, tord = 0;
    const int want_tord = mode != 0 ? 0 : p.tile_cost != nullptr ? 2 : p.tile_order != nullptr ? 1 : 0;
    if (p.S >= 12) {
        family = 1;
        cls = !(p.S <= 64 && p.L >= 1 && p.L <= 4) ? 0 : p.lights_a2_ok ? 2 : 1;
        if (cls == 2 && !gpow) tord = want_tord;
    } else {
        family = 0;
        cls = p.S <= 8 ? 8 : 0;
        if (mode == 0 && p.n_frames <= 1 && p.copy_z == 0) wpg = 4, tord = want_tord;
    }
    *v = TraceVariant{family, gpow ? 1 : 0, mode, cls, K, wpg, tord};
    return true;
}
// ... and with the stride: only a path launch without a shutter, on the 256-byte grid; PATH (4) becomes ANIM (8).
bool expect_now(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.scene_stride != 0 && (p.views == nullptr || p.shutter_log2 != 0 || p.scene_stride % 256 != 0)) return false;
    if (!expect_before(p, gpow, stats, v)) return false;
    if (p.scene_stride != 0) {
        if (v->mode != 4) return false;
        v->mode = 8;
    }
    return true;
}

long long zero_cases = 0, set_cases = 0, refused_shutter = 0, refused_no_views = 0, refused_unaligned = 0;
size_t n_zero = 0, n_all = 0, n_anim = 0;
int n_built = 0;
void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 8, 9}, thrs[] = {0, 1, 256};
    static const unsigned long long strides[] = {0, 0, 256, 1ull << 20, 255, 1000};
    static uint32_t cell[2];
    static DevView view;
    static ResolveSum acc[4];
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    long long mismatches = 0;
    std::set<Key> seen_zero, seen;
    // passes 0 and 1: progressive_host's grid (without and with an accumulator), the stride 0; passes 2..5: the grid
    // without an accumulator and with a stride -- two aligned ones, two that are not
    for (int pass = 0; pass < 6; ++pass)
    for (int thr : thrs) for (int sl : sls)
    for (int S : Ss) for (int L : Ls) for (int a2 = 0; a2 < 2; ++a2) for (int limit : limits)
    for (int gpow = 0; gpow < 2; ++gpow) for (int stats = 0; stats < 2; ++stats) for (int fmt = 0; fmt < 2; ++fmt)
    for (int ss = 0; ss <= 4; ++ss) for (int views = 0; views < 2; ++views) for (int nf = 1; nf <= 2; ++nf)
    for (int cz = 0; cz < 2; ++cz) for (int to = 0; to < 2; ++to) for (int tc = 0; tc < 2; ++tc)
    for (int ro = 0; ro < 2; ++ro) for (int cm = 0; cm < 2; ++cm) {
        if (pass >= 2 && (thr != 0 || ss > 1)) continue;  // (neither matters to a launch with views: refused alike)
        p.S = S, p.L = L, p.lights_a2_ok = a2, p.limit = limit;
        p.out_fmt = fmt ? OUT_TILES : 0;
        p.ss_log2 = ss;
        p.views = views ? &view : nullptr;
        p.shutter_log2 = sl;
        p.adapt_thr = thr;
        p.n_frames = nf, p.copy_z = cz;
        p.tile_order = to ? &cell[0] : nullptr, p.tile_cost = tc ? &cell[1] : nullptr;
        p.row_order_n = ro ? 2 : 0, p.col_major = cm;
        p.prog_acc = pass == 1 ? acc : nullptr;
        p.prog_first = 0, p.prog_n = pass == 1 ? 2 : 0;
        p.prog_pass[0] = 0, p.prog_pass[1] = pass == 1 ? 1 : 0;
        p.scene_stride = strides[pass];
        TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
        const bool w = expect_now(p, gpow != 0, stats != 0, &want);
        const bool g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
        ++(pass >= 2 ? set_cases : zero_cases);
        if (pass >= 2 && !g) {
            if (views && sl != 0) ++refused_shutter;
            else if (!views) ++refused_no_views;
            else if (strides[pass] % 256 != 0) ++refused_unaligned;
        }
        if (w != g || (w && key_of(want) != key_of(got))) {
            if (mismatches++ < 10)
                std::fprintf(stderr, "anim_host: MISMATCH pass %d thr %d sl %d S %d L %d a2 %d limit %d gpow %d stats %d fmt %d ss %d "
                             "views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d %d %d %d}\n",
                             pass, thr, sl, S, L, a2, limit, gpow, stats, fmt, ss, views, nf, cz, to, tc, ro, cm, (int)w, want.family,
                             want.gpow, want.mode, want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow,
                             got.mode, got.cls, got.K, got.wpg, got.tord);
            continue;
        }
        if (!g) continue;
        EXPECT((got.mode == TM_ANIM) == (pass >= 2), "the ANIM mode exactly with a stride");
        EXPECT(pass < 4, "an unaligned stride selects nothing");
        if (pass < 2) seen_zero.insert(key_of(got));
        seen.insert(key_of(got));
        EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
        const unsigned word = variant_word(got);
        EXPECT(((word & VF_ANIM) != 0) == (got.mode == TM_ANIM) && ((word & VF_PATH) != 0) == (got.mode == TM_PATH) &&
                   vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg && vf_tord_of(word) == got.tord &&
                   ((word & VF_GPOW) != 0) == (got.gpow != 0),
               "the variant word reads back");
        if (pass >= 2) {  // the PATH twin: the same launch without the stride
            LaunchParams q = p;
            q.scene_stride = 0;
            TraceVariant twin{-3, -3, -3, -3, -3, -3, -3};
            EXPECT(pick_trace_variant(q, gpow != 0, stats != 0, &twin) && twin.mode == TM_PATH, "the PATH twin exists");
            twin.mode = TM_ANIM;
            EXPECT(key_of(twin) == key_of(got), "an ANIM descriptor mirrors its PATH twin field for field");
        }
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_zero = seen_zero.size(), n_all = seen.size();
    EXPECT(n_zero == 564, "564 distinct descriptors with the stride 0, got %zu", n_zero);
    EXPECT(n_all == 624, "624 distinct descriptors in all, got %zu", n_all);
    int per_entry[2][2] = {}, path_entry[2][2] = {};
    for (const Key& k : seen) {
        if (std::get<2>(k) == TM_PATH) path_entry[std::get<0>(k)][std::get<1>(k)]++;
        if (std::get<2>(k) != TM_ANIM) continue;
        ++n_anim;
        per_entry[std::get<0>(k)][std::get<1>(k)]++;
        EXPECT(std::get<5>(k) == 1 && std::get<6>(k) == 0, "an ANIM launch has one tile per workgroup in grid order");
        EXPECT(seen_zero.count(k) == 0, "no ANIM descriptor without a stride");
    }
    EXPECT(n_anim == 60, "60 ANIM descriptors, got %zu", n_anim);
    EXPECT(per_entry[0][0] == 12 && per_entry[0][1] == 12 && per_entry[1][0] == 18 && per_entry[1][1] == 18,
           "direct 12 + 12 GPOW, bundle 18 + 18 GPOW");
    EXPECT(std::memcmp(per_entry, path_entry, sizeof per_entry) == 0, "ANIM's split over the entry points is PATH's");
    EXPECT(refused_shutter > 0 && refused_no_views > 0 && refused_unaligned > 0, "each refusal of a stride was reached");
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m <= TM_ANIM; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built == 624, "624 built descriptors, got %d", n_built);
    static_assert(sizeof(LaunchParams) < 4096, "the kernarg block");
    static_assert(TM_ANIM == 8 && VF_ANIM >= (1u << 18), "the new mode follows the earlier ones, its flag above vf_tord");
    static_assert(offsetof(LaunchParams, scene_stride) > offsetof(LaunchParams, shgrp), "the stride is the last field");
}

// ---- 2. and 3. track_build -----------------------------------------------------------------------------------------
rt_material material(int kind, float n = 2.0f) {
    rt_material m;
    std::memset(&m, 0, sizeof m);
    if (kind == 0) m.kd = m.ka = v3(0.6f, 0.5f, 0.4f);
    if (kind == 1) m.kd = m.ka = m.ks = v3(0.3f, 0.6f, 0.9f), m.n = n;
    if (kind == 2) m.km = v3(0.8f, 0.8f, 0.8f);
    if (kind == 3) m.kd = m.ka = v3(1, 1, 1), m.km = v3(0.5f, 0.5f, 0.5f);
    return m;
}

struct TrackArgs {
    int S, P, L, limit, n;
    std::vector<rt_sphere> sph;
    std::vector<rt_plane> pl;
    std::vector<rt_light> li;
    std::vector<rt_vec3> amb;
};
TrackArgs random_track(int S, int P, int L, int limit, int n) {
    TrackArgs t{S, P, L, limit, n, {}, {}, {}, {}};
    t.sph.resize((size_t)S * n), t.pl.resize((size_t)P * n), t.li.resize((size_t)L * n), t.amb.resize((size_t)n);
    for (int f = 0; f < n; ++f) {
        for (int i = 0; i < S; ++i) {
            rt_sphere& s = t.sph[(size_t)f * S + i];
            s.center = v3(unif(-8, 8), unif(-1, 3), unif(2, 14));
            s.radius = unif(0.05f, 1.2f);
            s.material = f ? t.sph[(size_t)i].material : material((int)(next64() % 3));
        }
        for (int j = 0; j < P; ++j) {
            rt_plane& q = t.pl[(size_t)f * P + j];
            q.material = material(3);
            q.normal = j == 0 ? v3(0, 1, 0) : v3(0, 0, -1);
            q.center = j == 0 ? v3(0, unif(-2.0f, -0.5f), 0) : v3(0, 0, unif(14, 20));
        }
        for (int k = 0; k < L; ++k) t.li[(size_t)f * L + k] = rt_light{v3(unif(-9, 9), unif(3, 9), unif(-6, 6)), unif(0.3f, 1.0f)};
        t.amb[(size_t)f] = v3(unif(0, 0.3f), unif(0, 0.3f), unif(0, 0.3f));
    }
    return t;
}
int build(const TrackArgs& t, const SceneOptions& opt, int threads, SceneTrack* T) {
    return track_build(t.sph.data(), t.S, t.pl.data(), t.P, t.li.data(), t.L, t.amb.data(), t.limit, t.n, opt, threads, T);
}

long slices = 0, pooled = 0;
void check_track(const char* name, const TrackArgs& t, const SceneOptions& opt) {
    SceneTrack T;
    EXPECT(build(t, opt, 1, &T) == TRACK_OK, "%s: track_build", name);
    EXPECT(T.n_frames == t.n && T.stride % 256 == 0 && T.image.size() == (size_t)t.n * T.stride && T.frames.size() == (size_t)t.n,
           "%s: sizes", name);
    EXPECT(T.stride == track_frame_bytes(t.S, t.P, t.L, opt), "%s: the stride is the layout's bytes", name);
    bool a2 = true, gp = false, differ = false;
    for (int f = 0; f < t.n; ++f) {
        const SceneLayout L = scene_build(t.sph.data() + (size_t)f * t.S, t.S, t.pl.data() + (size_t)f * t.P, t.P,
                                          t.li.data() + (size_t)f * t.L, t.L, t.amb[(size_t)f], t.limit, opt);
        EXPECT(L.bytes == T.stride && L.host_blob.size() == T.stride, "%s frame %d: bytes", name, f);
        if (L.host_blob.size() != T.stride) continue;
        EXPECT(std::memcmp(T.image.data() + (size_t)f * T.stride, L.host_blob.data(), T.stride) == 0, "%s frame %d: the slice", name, f);
        differ = differ || std::memcmp(T.image.data(), L.host_blob.data(), T.stride) != 0;
        const SceneLayout& R = T.frames[(size_t)f];
        EXPECT(track_same_layout(L, R) && track_same_layout(L, T.common) && L.n_clus == R.n_clus && L.n_clus == T.common.n_clus,
               "%s frame %d: the layout", name, f);
        EXPECT(L.lights_a2_ok == R.lights_a2_ok && L.generic_pow == R.generic_pow, "%s frame %d: the frame's flags", name, f);
        EXPECT(R.host_sph.size() == (size_t)t.S && R.host_pl.size() == (size_t)t.P &&
                   (t.S == 0 || std::memcmp(R.host_sph.data(), L.host_sph.data(), sizeof(DevSphere) * (size_t)t.S) == 0) &&
                   (t.P == 0 || std::memcmp(R.host_pl.data(), L.host_pl.data(), sizeof(DevPlane) * (size_t)t.P) == 0),
               "%s frame %d: the host records", name, f);
        const size_t mats = L.off_mat + sizeof(DevMaterial) * (size_t)(t.S + t.P);
        EXPECT(R.host_blob.size() == mats && std::memcmp(R.host_blob.data(), L.host_blob.data(), mats) == 0,
               "%s frame %d: the materials behind the host records", name, f);
        a2 = a2 && L.lights_a2_ok, gp = gp || L.generic_pow;
        ++slices;
    }
    EXPECT(differ, "%s: the frames' images differ (teeth)", name);
    EXPECT(T.common.lights_a2_ok == a2 && T.common.generic_pow == gp, "%s: AND of lights_a2_ok, OR of generic_pow", name);
    EXPECT(T.common.host_blob.empty(), "%s: the common layout carries no image", name);
    for (int threads : {2, 3, 16}) {
        SceneTrack U;
        EXPECT(build(t, opt, threads, &U) == TRACK_OK && U.stride == T.stride && U.image == T.image, "%s: %d threads, the image", name, threads);
        for (int f = 0; f < t.n && U.frames.size() == T.frames.size(); ++f)
            EXPECT(U.frames[(size_t)f].host_blob == T.frames[(size_t)f].host_blob && U.frames[(size_t)f].n_clus == T.frames[(size_t)f].n_clus,
                   "%s: %d threads, frame %d", name, threads, f);
        ++pooled;
    }
}

long mixed = 0;
void check_tracks() {
    const SceneOptions opt;
    check_track("direct S=8", random_track(8, 1, 2, 3, 5), opt);
    {
        const TrackArgs t = random_track(64, 2, 4, 5, 4);
        check_track("bundle S=64", t, opt);
        SceneTrack T;
        build(t, opt, 1, &T);
        EXPECT(T.common.has_shg && T.common.n_clus == 8 && T.common.has_shcull && !T.common.has_shpre, "bundle S=64: grids and 8 clusters");
        SceneOptions off;
        off.shadow_grid = false, off.cluster_size = 0;
        check_track("bundle S=64, grids and clusters off", t, off);
    }
    check_track("odd S=3 P=2", random_track(3, 2, 1, 1, 3), opt);
    {
        SceneOptions off;
        off.shadow_pre = false;
        check_track("direct S=8, pre-test off", random_track(8, 1, 2, 3, 3), off);
    }
    // a light at the origin in one frame (2a = 0): the track is not a2-ok, and the frames keep their own flag
    for (int S : {8, 64}) {
        TrackArgs t = random_track(S, 1, 2, 2, 4);
        t.li[(size_t)2 * 2 + 1].position = v3(0, 0, 0);
        SceneTrack T;
        EXPECT(build(t, opt, 1, &T) == TRACK_OK, "origin light: track_build");
        EXPECT(!T.common.lights_a2_ok && T.frames[0].lights_a2_ok && !T.frames[2].lights_a2_ok && !T.common.generic_pow, "origin light: the AND");
        check_track("origin light", t, opt);
        ++mixed;
    }
    // a general exponent in one frame
    for (int S : {8, 64}) {
        TrackArgs t = random_track(S, 1, 2, 2, 4);
        for (int f = 0; f < t.n; ++f) t.sph[(size_t)f * S].material = material(1, f == 1 ? 7.3f : 2.0f);
        SceneTrack T;
        EXPECT(build(t, opt, 1, &T) == TRACK_OK, "generic exponent: track_build");
        EXPECT(T.common.generic_pow && !T.frames[0].generic_pow && T.frames[1].generic_pow && T.common.lights_a2_ok, "generic exponent: the OR");
        check_track("generic exponent", t, opt);
        ++mixed;
    }
}

// ---- 4. refusals ---------------------------------------------------------------------------------------------------
long refusals = 0;
void refuse(int got, int want, const rt_ctx* ctx, const char* text, const char* what) {
    const char* msg = rt_last_error(ctx);
    EXPECT(got == want, "%s: status %d, expected %d (%s)", what, got, want, msg ? msg : "");
    EXPECT(msg && std::strstr(msg, text), "%s: error text \"%s\" lacks \"%s\"", what, msg ? msg : "", text);
    ++refusals;
}
void check_refusals() {
    const TrackArgs t = random_track(8, 1, 2, 3, 6);
    rt_ctx ctx;  // (no devices: nothing below may reach one)
    const rt_sphere* S = t.sph.data();
    const rt_plane* P = t.pl.data();
    const rt_light* L = t.li.data();
    const rt_vec3* A = t.amb.data();
    // rt_set_scene_track, each refusal with everything later in the order wrong as well
    refuse(rt_set_scene_track(nullptr, S, 8, P, 1, L, 2, A, 3, 0), RT_ERR_INVALID_ARG, nullptr, "NULL context", "NULL context");
    refuse(rt_set_scene_track(&ctx, S, 8, P, 1, L, 2, nullptr, 3, 0), RT_ERR_INVALID_ARG, &ctx, "NULL ambients", "NULL ambients");
    refuse(rt_set_scene_track(&ctx, nullptr, 8, P, 1, L, 2, A, 3, 0), RT_ERR_INVALID_ARG, &ctx, "bad primitive arrays", "NULL spheres");
    refuse(rt_set_scene_track(&ctx, S, 8, nullptr, 1, L, 2, A, 3, 0), RT_ERR_INVALID_ARG, &ctx, "bad primitive arrays", "NULL planes");
    refuse(rt_set_scene_track(&ctx, S, 8, P, 1, nullptr, 2, A, 3, 0), RT_ERR_INVALID_ARG, &ctx, "bad primitive arrays", "NULL lights");
    refuse(rt_set_scene_track(&ctx, S, -1, P, 1, L, 2, A, -1, 0), RT_ERR_INVALID_ARG, &ctx, "frame count", "0 frames");
    refuse(rt_set_scene_track(&ctx, S, -1, P, 1, L, 2, A, -1, RT_MAX_PATH_FRAMES + 1), RT_ERR_INVALID_ARG, &ctx, "frame count", "too many frames");
    refuse(rt_set_scene_track(&ctx, S, -1, P, 1, L, RT_MAX_LIGHTS + 1, A, 3, 6), RT_ERR_INVALID_ARG, &ctx, "bad primitive arrays", "a negative count");
    refuse(rt_set_scene_track(&ctx, S, 8, P, 1, L, RT_MAX_LIGHTS + 1, A, -1, 6), RT_ERR_INVALID_ARG, &ctx, "recursion_limit", "a negative limit");
    refuse(rt_set_scene_track(&ctx, S, 8, P, 1, L, RT_MAX_LIGHTS + 1, A, RT_MAX_RECURSION_LIMIT + 1, 6), RT_ERR_UNSUPPORTED, &ctx, "n_lights", "too many lights");
    refuse(rt_set_scene_track(&ctx, S, 8, P, 1, L, 2, A, RT_MAX_RECURSION_LIMIT + 1, RT_MAX_PATH_FRAMES), RT_ERR_UNSUPPORTED, &ctx,
           "recursion_limit", "a limit above the bound");
    // (64 spheres and 4 lights: 137 KiB of grids per frame; 65535 such frames are above 1 GiB -- refused by size alone,
    // before any frame is read: the arrays hold 6 frames)
    {
        const TrackArgs big = random_track(64, 2, 4, 5, 1);
        refuse(rt_set_scene_track(&ctx, big.sph.data(), 64, big.pl.data(), 2, big.li.data(), 4, A, 5, RT_MAX_PATH_FRAMES), RT_ERR_OOM, &ctx,
               "RT_MAX_TRACK_BYTES", "a track above the bound");
    }
    EXPECT(!ctx.has_track && !ctx.has_scene, "a refused track leaves the context without one");
    // the renders
    rt_camera cams[6];
    std::memset(cams, 0, sizeof cams);
    int32_t px[4];
    int nb = -1;
    auto bands = [&](rt_ctx* c, const rt_camera* cm, int W, int H, int first, int n) {
        return rt_render_anim_bands(c, W, H, cm, first, n, 8, 0, 1, px, 0, RT_BANDS_INT32, nullptr, &nb);
    };
    auto frames = [&](rt_ctx* c, const rt_camera* cm, int W, int H, int first, int n) { return rt_render_anim(c, W, H, cm, first, n, px); };
    for (int call = 0; call < 2; ++call) {
        auto go = [&](rt_ctx* c, const rt_camera* cm, int W, int H, int first, int n) {
            return call ? frames(c, cm, W, H, first, n) : bands(c, cm, W, H, first, n);
        };
        rt_ctx c2;
        c2.n_gpus = 2;
        rt_set_supersampling(&c2, 2);
        refuse(go(nullptr, cams, 0, 0, -1, 0), RT_ERR_INVALID_ARG, nullptr, "NULL context", "render: NULL context");
        refuse(go(&c2, nullptr, 0, 0, -1, 3), RT_ERR_INVALID_ARG, &c2, "NULL cameras", "render: NULL cameras");
        refuse(go(&c2, cams, 0, 0, -1, 0), RT_ERR_INVALID_ARG, &c2, "frame count", "render: 0 frames");
        refuse(go(&c2, cams, 0, 0, -1, RT_MAX_PATH_FRAMES + 1), RT_ERR_INVALID_ARG, &c2, "frame count", "render: too many frames");
        refuse(go(&c2, cams, 0, 0, -1, 3), RT_ERR_NO_SCENE, &c2, "rt_set_scene_track has not been called", "render: no track");
        // (rt_set_scene alone does not make a track)
        EXPECT(rt_set_scene(&c2, S, 8, P, 1, L, 2, A[0], 3) == RT_OK, "rt_set_scene");
        refuse(go(&c2, cams, 16, 8, 0, 3), RT_ERR_NO_SCENE, &c2, "rt_set_scene_track has not been called", "render: a scene but no track");
        EXPECT(rt_set_scene_track(&c2, S, 8, P, 1, L, 2, A, 3, 6) == RT_OK && c2.has_track && c2.track.n_frames == 6, "rt_set_scene_track: %s",
               c2.last_error.c_str());
        EXPECT(c2.has_scene && c2.scene_gen == 1, "the track leaves the context's scene alone");
        refuse(go(&c2, cams, 0, 8, -1, 3), RT_ERR_INVALID_ARG, &c2, "invalid frame size", "render: frame size");
        refuse(go(&c2, cams, 16, 8, -1, 3), RT_ERR_INVALID_ARG, &c2, "outside the track", "render: first_frame -1");
        refuse(go(&c2, cams, 16, 8, -5, 3), RT_ERR_INVALID_ARG, &c2, "outside the track", "render: first_frame < 0");
        refuse(go(&c2, cams, 16, 8, 4, 3), RT_ERR_INVALID_ARG, &c2, "outside the track", "render: beyond the track");
        refuse(go(&c2, cams, 16, 8, 6, 1), RT_ERR_INVALID_ARG, &c2, "outside the track", "render: first_frame at the end");
        refuse(go(&c2, cams, 16, 8, 2, 3), RT_ERR_INVALID_ARG, &c2, "single-GPU", "render: two workers");
        c2.n_gpus = 1;
        refuse(go(&c2, cams, 16, 8, 2, 3), RT_ERR_UNSUPPORTED, &c2, "does not supersample", "render: supersampling");
        // a replaced track, a cleared track
        EXPECT(rt_set_scene_track(&c2, S, 8, P, 1, L, 2, A, 3, 2) == RT_OK && c2.track.n_frames == 2, "replacing the track");
        refuse(go(&c2, cams, 16, 8, 2, 1), RT_ERR_INVALID_ARG, &c2, "outside the track", "render: beyond the replaced track");
        EXPECT(rt_clear_scene_track(&c2) == RT_OK && !c2.has_track && c2.has_scene, "rt_clear_scene_track");
        refuse(go(&c2, cams, 16, 8, 0, 1), RT_ERR_NO_SCENE, &c2, "rt_set_scene_track has not been called", "render: a cleared track");
    }
    refuse(rt_clear_scene_track(nullptr), RT_ERR_INVALID_ARG, nullptr, "NULL context", "clear: NULL context");
    // the view records of a track frame are built against that frame's spheres: frame f's record equals the record
    // of a context whose scene is frame f
    rt_ctx c3;
    EXPECT(rt_set_scene_track(&c3, S, 8, P, 1, L, 2, A, 3, 6) == RT_OK, "rt_set_scene_track");
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.position = v3(0.5f, 1.0f, -2.0f);
    DevView first;
    for (int f = 0; f < 6; ++f) {
        rt_ctx one;
        EXPECT(rt_set_scene(&one, S + (size_t)f * 8, 8, P + f, 1, L + (size_t)f * 2, 2, A[f], 3) == RT_OK, "rt_set_scene");
        LaunchParams a, b;
        std::memset(&a, 0, sizeof a), std::memset(&b, 0, sizeof b);
        EXPECT(view_fill(&one, cam, 100, 60, a) == RT_OK && view_fill(&c3, c3.track.frames[(size_t)f], cam, 100, 60, b) == RT_OK, "view_fill");
        DevView va, vb;
        view_record(a, va), view_record(b, vb);
        EXPECT(std::memcmp(&va, &vb, sizeof va) == 0, "frame %d: the view record of the track frame", f);
        if (f == 0) first = vb;
        else EXPECT(std::memcmp(&first, &vb, sizeof vb) != 0, "frame %d: the records of different scenes differ (teeth)", f);
    }
}
}  // namespace

int main() {
    check_variants();
    check_tracks();
    check_refusals();
    std::printf("anim_host: %lld variant cases with the stride 0, %lld with it set (%lld refused for a shutter, %lld without views, "
                "%lld unaligned), %zu descriptors without a stride, %zu in all (%zu ANIM), %d built\n",
                zero_cases, set_cases, refused_shutter, refused_no_views, refused_unaligned, n_zero, n_all, n_anim, n_built);
    std::printf("anim_host: %ld track slices equal scene_build, %ld pooled builds equal the serial one, %ld mixed tracks\n", slices, pooled, mixed);
    std::printf("anim_host: %ld refusals\n", refusals);
    std::printf("anim_host: %ld failures\n", failures);
    return failures == 0 && zero_cases > 0 && set_cases > 0 && slices > 0 && pooled > 0 && refusals > 0 ? 0 : 1;
}
