// anim_shutter_host.cpp -- host check of scene-track shutters (rt_render_anim_shutter[_bands]), TEST
// INFRASTRUCTURE ONLY.  rt_api.cpp is compiled into this translation unit (its helpers have internal linkage); no device
// call is reached (contexts without devices).  Built plain and under host-side ASan + UBSan (anim_shutter.mk).
//  1. Variant selection (rt_internal.h pick_trace_variant) against a restatement.  With LaunchParams::scene_shutter zero,
//     over a sweep of every field the rule reads: exactly the earlier rule, 924 distinct descriptors, none in a new mode,
//     the earlier refusals (a stride with a shutter among them).  With it set: ANIM_SHUTTER / ANIM_SHUTTER_SS exactly with
//     the value 1, views, a stride on the 256-byte grid, shutter_log2 in 1..8, no adaptive threshold and -- with view_ss
//     -- a factor in 1..3 and shutter_log2 + 2 ss_log2 <= 8; each descriptor the mirror of its SHUTTER / SHUTTER_SS twin
//     (the same launch without the stride and the mark), 60 + 60 split over the entry points as PATH's are, 1044 built,
//     the variant word reads back, and every refusal reached.  The field lies in padding inside the block.
//  2. The refusals of both calls through the C ABI, in the header's order: rt_render_anim*'s with the track bound counting
//     n_frames * shutter track frames, then the shutter's, then the band arguments and the output.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

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

using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// ---- 1. variant selection --------------------------------------------------------------------------------------------
// The rule before view_ss restated, thresholds and mode numbers as literals (view_ss, view_adapt and scene_shutter are
// not read).
bool expect_base(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    const bool tiles = p.out_fmt == 3, ordered = p.tile_order != nullptr || p.tile_cost != nullptr;
    const int sl = p.shutter_log2;
    if (sl != 0 && (p.views == nullptr || sl < 0 || sl > 8)) return false;
    if (p.scene_stride != 0 && (p.views == nullptr || sl != 0 || p.scene_stride % 256 != 0)) return false;
    if (p.prog_acc != nullptr) {
        if (p.views != nullptr || p.ss_log2 < 1 || p.ss_log2 > 3 || p.adapt_thr != 0) return false;
        if (p.prog_first < 0 || p.prog_n < 0 || p.prog_n > 2) return false;
        const int total = p.prog_first + p.prog_n;
        if (total < 1 || total > 1 << (2 * p.ss_log2)) return false;
    }
    int mode;
    if (p.views != nullptr) {
        if (p.ss_log2 > 0 || tiles || stats || ordered || p.copy_z != 0 || p.row_order_n != 0 || p.col_major != 0) return false;
        mode = sl > 0 ? 5 : p.scene_stride != 0 ? 8 : 4;
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
// ... with view_ss: views, a factor in 1..3 and sums that fit 16 bits; then the twin's launch decides, and PATH (4) /
// SHUTTER (5) / ANIM (8) become 9 / 10 / 11.
bool expect_ss(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.view_ss == 0) return expect_base(p, gpow, stats, v);
    if (p.view_ss != 1 || p.views == nullptr || p.ss_log2 < 1 || p.ss_log2 > 3) return false;
    if ((1 << p.ss_log2) * (1 << p.ss_log2) * (p.shutter_log2 > 0 ? 1ll << (p.shutter_log2 > 30 ? 30 : p.shutter_log2) : 1ll) > 256)
        return false;
    LaunchParams q = p;
    q.ss_log2 = 0, q.view_ss = 0;
    if (!expect_base(q, gpow, stats, v)) return false;
    if (v->mode != 4 && v->mode != 5 && v->mode != 8) return false;
    v->mode = v->mode == 4 ? 9 : v->mode == 5 ? 10 : 11;
    return true;
}
// Today's rule (scene_shutter is not read): with view_adapt, a value in 1..256 on a supersampled path or track launch
// without a shutter, and PATH_SS (9) / ANIM_SS (11) become 12 / 13.
bool expect_today(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.view_adapt == 0) return expect_ss(p, gpow, stats, v);
    if (p.view_adapt < 1 || p.view_adapt > 256) return false;
    if (p.views == nullptr || p.view_ss != 1 || p.ss_log2 < 1 || p.ss_log2 > 3 || p.shutter_log2 != 0) return false;
    LaunchParams q = p;
    q.view_adapt = 0;
    if (!expect_ss(q, gpow, stats, v)) return false;
    if (v->mode != 9 && v->mode != 11) return false;
    v->mode = v->mode == 9 ? 12 : 13;
    return true;
}
// With the new field set: the value 1 on a launch with a stride on the 256-byte grid, a shutter and no adaptive
// threshold; then the same launch without the stride and the mark -- a camera shutter's -- decides, and SHUTTER (5) /
// SHUTTER_SS (10) become 14 / 15.
bool expect_new(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.scene_shutter == 0) return expect_today(p, gpow, stats, v);
    if (p.scene_shutter != 1 || p.scene_stride == 0 || p.scene_stride % 256 != 0 || p.shutter_log2 < 1 || p.view_adapt != 0) return false;
    LaunchParams q = p;
    q.scene_shutter = 0, q.scene_stride = 0;
    if (!expect_today(q, gpow, stats, v)) return false;
    if (v->mode != 5 && v->mode != 10) return false;
    v->mode = v->mode == 5 ? 14 : 15;
    return true;
}

long long zero_cases = 0, set_cases = 0, zero_refused = 0, zero_refused_stride_shutter = 0;
long long ref_value = 0, ref_no_stride = 0, ref_unaligned = 0, ref_no_shutter = 0, ref_shutter_hi = 0, ref_no_views = 0, ref_adapt = 0,
          ref_view_ss = 0, ref_factor = 0, ref_sums = 0, ref_tiles = 0, ref_stats = 0, ref_ordered = 0, ref_copy = 0;
size_t n_zero = 0, n_all = 0, n_new[2] = {0, 0};
int n_built = 0;
long long mismatches = 0;
std::set<Key> seen_zero, seen;

void check_case(const LaunchParams& p, int gpow, int stats, bool set_phase) {
    TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
    const bool w = expect_new(p, gpow != 0, stats != 0, &want);
    const bool g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
    ++(set_phase ? set_cases : zero_cases);
    if (w != g || (w && key_of(want) != key_of(got))) {
        if (mismatches++ < 10)
            std::fprintf(stderr, "anim_shutter_host: MISMATCH mark %d adapt %d view_ss %d stride %llu thr %d sl %d S %d L %d a2 %d limit %d "
                         "gpow %d stats %d fmt %d ss %d views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d "
                         "{%d %d %d %d %d %d %d}\n", p.scene_shutter, p.view_adapt, p.view_ss, p.scene_stride, p.adapt_thr, p.shutter_log2, p.S,
                         p.L, p.lights_a2_ok, p.limit, gpow, stats, p.out_fmt, p.ss_log2, p.views != nullptr, p.n_frames, p.copy_z,
                         p.tile_order != nullptr, p.tile_cost != nullptr, p.row_order_n, p.col_major, (int)w, want.family, want.gpow, want.mode,
                         want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow, got.mode, got.cls, got.K, got.wpg, got.tord);
        return;
    }
    const bool views = p.views != nullptr, ordered = p.tile_order != nullptr || p.tile_cost != nullptr;
    const int ss = p.ss_log2, sl = p.shutter_log2;
    if (!set_phase && !g) {
        ++zero_refused;
        if (views && p.scene_stride != 0 && p.scene_stride % 256 == 0 && sl >= 1 && sl <= 8) ++zero_refused_stride_shutter;
    }
    if (set_phase && !g) {  // which refusal: the first thing the launch lacks
        if (p.scene_shutter != 1) ++ref_value;
        else if (p.scene_stride == 0) ++ref_no_stride;
        else if (p.scene_stride % 256 != 0) ++ref_unaligned;
        else if (sl <= 0) ++ref_no_shutter;
        else if (sl > 8) ++ref_shutter_hi;
        else if (!views) ++ref_no_views;
        else if (p.view_adapt != 0) ++ref_adapt;
        else if (p.view_ss != 0 && p.view_ss != 1) ++ref_view_ss;
        else if ((p.view_ss == 1) != (ss >= 1 && ss <= 3)) ++ref_factor;
        else if (sl + 2 * ss > 8) ++ref_sums;
        else if (p.out_fmt == OUT_TILES) ++ref_tiles;
        else if (stats) ++ref_stats;
        else if (ordered) ++ref_ordered;
        else if (p.copy_z) ++ref_copy;
    }
    if (!g) return;
    const bool is_new = got.mode >= TM_ANIM_SHUTTER;
    EXPECT(is_new == set_phase, "a new mode exactly with the field set");
    if (is_new) {
        EXPECT(p.scene_shutter == 1 && views && p.scene_stride != 0 && p.scene_stride % 256 == 0 && sl >= 1 && sl <= 8 && sl + 2 * ss <= 8,
               "a new mode only with the mark, views, a stride on the 256-byte grid, a shutter and sums that fit");
        EXPECT(got.mode == (p.view_ss != 0 ? TM_ANIM_SHUTTER_SS : TM_ANIM_SHUTTER), "ANIM_SHUTTER_SS with view_ss, otherwise ANIM_SHUTTER");
        LaunchParams q = p;  // the twin: the camera shutter's launch
        q.scene_shutter = 0, q.scene_stride = 0;
        TraceVariant twin{-3, -3, -3, -3, -3, -3, -3};
        const int twin_mode = got.mode == TM_ANIM_SHUTTER ? TM_SHUTTER : TM_SHUTTER_SS;
        EXPECT(pick_trace_variant(q, gpow != 0, stats != 0, &twin) && twin.mode == twin_mode, "the twin exists");
        twin.mode = got.mode;
        EXPECT(key_of(twin) == key_of(got), "a new descriptor mirrors its twin field for field");
    }
    if (!set_phase) seen_zero.insert(key_of(got));
    seen.insert(key_of(got));
    EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
    const unsigned word = variant_word(got);
    const unsigned old_flags = VF_STATS | VF_TILES | VF_SS | VF_PATH | VF_SHUTTER | VF_ADAPT | VF_PROG | VF_ANIM | VF_VIEW_SS | VF_VIEW_ADAPT;
    EXPECT(((word & VF_ANIM_SHUTTER) != 0) == (got.mode == TM_ANIM_SHUTTER) && ((word & VF_ANIM_SHUTTER_SS) != 0) == (got.mode == TM_ANIM_SHUTTER_SS) &&
               ((word & VF_SHUTTER) != 0) == (got.mode == TM_SHUTTER) && ((word & VF_SHUTTER_SS) != 0) == (got.mode == TM_SHUTTER_SS) &&
               ((word & VF_ANIM) != 0) == (got.mode == TM_ANIM) && ((word & VF_ANIM_SS) != 0) == (got.mode == TM_ANIM_SS) &&
               (!is_new || (word & old_flags) == 0) && vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg &&
               vf_tord_of(word) == got.tord && ((word & VF_GPOW) != 0) == (got.gpow != 0),
           "the variant word reads back");
}

void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 4, 8, 9, -1}, thrs[] = {0, 1, 256};
    // passes 0..8: the new field zero -- today's launches: plain, progressive, a stride (aligned, unaligned), view_ss without
    // and with a stride, the adaptive twins, view_ss = 2; 9..: the field set
    constexpr int PASSES = 19, SET_FROM = 9;
    static const unsigned long long strides[PASSES] = {0, 0, 256, 255, 0, 256, 256, 0, 0, 256, 256, 0, 255, 256, 256, 256, 1ull << 20, 1000, 256};
    static const int view_sss[PASSES] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 0, 1, 0, 0, 1, 0, 1, 1, 1, 2};
    static const int adapts[PASSES] = {0, 0, 0, 0, 0, 0, 16, 16, 0, 0, 0, 0, 0, 16, 0, 0, 0, 0, 0};
    static const int marks[PASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, -1, 1, 1, 1};
    static uint32_t cell[2];
    static DevView view;
    static ResolveSum acc[4];
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    for (int pass = 0; pass < PASSES; ++pass)
    for (int thr : thrs) for (int sl : sls)
    for (int S : Ss) for (int L : Ls) for (int a2 = 0; a2 < 2; ++a2) for (int limit : limits)
    for (int gpow = 0; gpow < 2; ++gpow) for (int stats = 0; stats < 2; ++stats) for (int fmt = 0; fmt < 2; ++fmt)
    for (int ss = 0; ss <= 4; ++ss) for (int views = 0; views < 2; ++views) for (int nf = 1; nf <= 2; ++nf)
    for (int cz = 0; cz < 2; ++cz) for (int to = 0; to < 2; ++to) for (int tc = 0; tc < 2; ++tc)
    for (int ro = 0; ro < 2; ++ro) for (int cm = 0; cm < 2; ++cm) {
        if (pass >= 2 && thr != 0) continue;                        // (a launch with views never reads adapt_thr)
        if (!views && sl != 0 && sl != 1) continue;                 // (without views one shutter is every shutter)
        if (sl != 0 && sl != 1 && (to || tc || ro || cm)) continue;  // (the order fields refuse whatever the shutter)
        if (pass >= 2 && limit > 1 && (to || tc || ro || cm || cz || (L != 1 && L != 5))) continue;
        if (pass >= 11 && limit > 1) continue;
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
        p.view_ss = view_sss[pass];
        p.view_adapt = adapts[pass];
        p.scene_shutter = marks[pass];
        check_case(p, gpow, stats, pass >= SET_FROM);
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_zero = seen_zero.size(), n_all = seen.size();
    EXPECT(n_zero == 924, "924 distinct descriptors with the field zero, got %zu", n_zero);
    EXPECT(n_all == 1044, "1044 distinct descriptors in all, got %zu", n_all);
    EXPECT(zero_refused_stride_shutter > 0, "with the field zero a stride with a shutter is refused");
    int per_entry[2][2][2] = {}, path_entry[2][2] = {};
    for (const Key& k : seen) {
        const int mode = std::get<2>(k);
        if (mode == TM_PATH) path_entry[std::get<0>(k)][std::get<1>(k)]++;
        if (mode < TM_ANIM_SHUTTER) continue;
        EXPECT(mode <= TM_ANIM_SHUTTER_SS, "no mode beyond ANIM_SHUTTER_SS");
        ++n_new[mode - TM_ANIM_SHUTTER];
        per_entry[mode - TM_ANIM_SHUTTER][std::get<0>(k)][std::get<1>(k)]++;
        EXPECT(std::get<5>(k) == 1 && std::get<6>(k) == 0, "a new launch has one tile per workgroup in grid order");
        EXPECT(seen_zero.count(k) == 0, "no new descriptor with the field zero");
    }
    for (int i = 0; i < 2; ++i) {
        EXPECT(n_new[i] == 60, "60 descriptors of new mode %d, got %zu", TM_ANIM_SHUTTER + i, n_new[i]);
        EXPECT(std::memcmp(per_entry[i], path_entry, sizeof path_entry) == 0, "mode %d's split over the entry points is PATH's",
               TM_ANIM_SHUTTER + i);
    }
    EXPECT(path_entry[0][0] == 12 && path_entry[0][1] == 12 && path_entry[1][0] == 18 && path_entry[1][1] == 18,
           "direct 12 + 12 GPOW, bundle 18 + 18 GPOW");
    EXPECT(ref_value > 0 && ref_no_stride > 0 && ref_unaligned > 0 && ref_no_shutter > 0 && ref_shutter_hi > 0 && ref_no_views > 0 &&
               ref_adapt > 0 && ref_view_ss > 0 && ref_factor > 0 && ref_sums > 0 && ref_tiles > 0 && ref_stats > 0 && ref_ordered > 0 &&
               ref_copy > 0,
           "every refusal of the field was reached");
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    int n_built_before = 0;
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m <= TM_ANIM_SHUTTER_SS; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        if (m < TM_ANIM_SHUTTER) ++n_built_before;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built_before == 924 && n_built == 924 + 120, "924 + 120 built descriptors, got %d + %d", n_built_before, n_built - n_built_before);
    static_assert(sizeof(LaunchParams) < 4096, "the kernarg block");
    static_assert(TM_ANIM_SHUTTER == 14 && TM_ANIM_SHUTTER_SS == 15, "the new modes follow ANIM_ADAPT");
    static_assert(VF_ANIM_SHUTTER > (1u << 23) && VF_ANIM_SHUTTER_SS > (1u << 23) && VF_ANIM_SHUTTER != VF_ANIM_SHUTTER_SS, "their flags sit above bit 23");
    static_assert(((VF_ANIM_SHUTTER | VF_ANIM_SHUTTER_SS) & (vf_cls(15) | vf_wpg(15) | vf_tord(3) | 0xffu | VF_ANIM | VF_VIEW_SS | VF_VIEW_ADAPT)) == 0,
                  "and on no earlier bit");
    static_assert(offsetof(LaunchParams, scene_shutter) == offsetof(LaunchParams, uniform_plane) + sizeof(int), "the field follows uniform_plane");
    static_assert(offsetof(LaunchParams, shgrp) == offsetof(LaunchParams, scene_shutter) + sizeof(int), "in the padding ahead of shgrp: no field moves");
    static_assert(sizeof(LaunchParams) == offsetof(LaunchParams, view_ss) + 8, "and the block keeps its size");
}

// ---- 2. refusals -----------------------------------------------------------------------------------------------------
long refusals = 0;
void refuse(int got, int want, const rt_ctx* ctx, const char* text, const char* what) {
    const char* msg = rt_last_error(ctx);
    EXPECT(got == want, "%s: status %d, expected %d (%s)", what, got, want, msg ? msg : "");
    EXPECT(msg && std::strstr(msg, text), "%s: error text \"%s\" lacks \"%s\"", what, msg ? msg : "", text);
    ++refusals;
}
rt_vec3 vec(float x, float y, float z) {
    rt_vec3 v;
    v.x = x, v.y = y, v.z = z;
    return v;
}
void check_refusals() {
    // a 16-frame track of one sphere, one plane and one light
    const int N = 16;
    std::vector<rt_sphere> S((size_t)N);
    std::vector<rt_plane> P((size_t)N);
    std::vector<rt_light> L((size_t)N);
    std::vector<rt_vec3> A((size_t)N);
    std::memset(S.data(), 0, S.size() * sizeof(rt_sphere)), std::memset(P.data(), 0, P.size() * sizeof(rt_plane));
    for (int f = 0; f < N; ++f) {
        S[(size_t)f].center = vec(0.25f * (float)f - 2.0f, 0.0f, 6.0f), S[(size_t)f].radius = 1.0f;
        S[(size_t)f].material.kd = vec(0.8f, 0.2f, 0.2f), S[(size_t)f].material.ka = vec(0.5f, 0.5f, 0.5f);
        P[(size_t)f].center = vec(0.0f, -1.0f, 0.0f), P[(size_t)f].normal = vec(0.0f, 1.0f, 0.0f);
        P[(size_t)f].material.kd = vec(1.0f, 1.0f, 1.0f);
        L[(size_t)f] = rt_light{vec(4.0f, 6.0f, -2.0f + 0.1f * (float)f), 1.0f};
        A[(size_t)f] = vec(0.1f, 0.1f, 0.1f);
    }
    rt_camera cams[16];
    std::memset(cams, 0, sizeof cams);
    int32_t px[4];
    int nb = -1;
    struct Bands {
        int rows, first, step;
        void* out;
        size_t stride;
        int fmt;
    };
    const Bands good{8, 0, 1, px, 0, RT_BANDS_INT32};
    for (int call = 0; call < 2; ++call) {
        auto go = [&](rt_ctx* c, const rt_camera* cm, int W, int H, int first, int n, int shutter, const Bands& b = Bands{8, 0, 1, nullptr, 0, 99},
                      int32_t* pixels = nullptr) {
            return call ? rt_render_anim_shutter(c, W, H, cm, first, n, shutter, pixels)
                        : rt_render_anim_shutter_bands(c, W, H, cm, first, n, shutter, b.rows, b.first, b.step, b.out, b.stride, b.fmt, nullptr, &nb);
        };
        // each refusal with everything later in the order wrong as well: a bad shutter (3), bad band arguments, no output
        rt_ctx c2;
        c2.n_gpus = 2;
        rt_set_supersampling(&c2, 2);
        EXPECT(rt_set_path_supersampling(&c2, 8) == RT_OK && rt_set_path_adaptive_sampling(&c2, 16) == RT_OK, "the path factor and threshold");
        refuse(go(nullptr, cams, 0, 0, -1, 0, 3), RT_ERR_INVALID_ARG, nullptr, "NULL context", "NULL context");
        refuse(go(&c2, nullptr, 0, 0, -1, 3, 3), RT_ERR_INVALID_ARG, &c2, "NULL cameras", "NULL cameras");
        refuse(go(&c2, cams, 0, 0, -1, 0, 3), RT_ERR_INVALID_ARG, &c2, "frame count", "0 frames");
        refuse(go(&c2, cams, 0, 0, -1, RT_MAX_PATH_FRAMES + 1, 3), RT_ERR_INVALID_ARG, &c2, "frame count", "too many frames");
        refuse(go(&c2, cams, 0, 0, -1, 2, 3), RT_ERR_NO_SCENE, &c2, "rt_set_scene_track has not been called", "no track");
        EXPECT(rt_set_scene_track(&c2, S.data(), 1, P.data(), 1, L.data(), 1, A.data(), 2, N) == RT_OK && c2.track.n_frames == N, "rt_set_scene_track: %s",
               c2.last_error.c_str());
        refuse(go(&c2, cams, 0, 8, -1, 2, 3), RT_ERR_INVALID_ARG, &c2, "invalid frame size", "frame size");
        refuse(go(&c2, cams, 16, 8, -1, 2, 3), RT_ERR_INVALID_ARG, &c2, "outside the track", "first_frame -1");
        refuse(go(&c2, cams, 16, 8, -4, 2, 3), RT_ERR_INVALID_ARG, &c2, "outside the track", "first_frame < 0");
        refuse(go(&c2, cams, 16, 8, 0, 9, 2), RT_ERR_INVALID_ARG, &c2, "outside the track", "9 frames of 2 track frames in a track of 16");
        refuse(go(&c2, cams, 16, 8, 1, 4, 4), RT_ERR_INVALID_ARG, &c2, "outside the track", "4 frames of 4 from track frame 1");
        refuse(go(&c2, cams, 16, 8, 0, 6, 3), RT_ERR_INVALID_ARG, &c2, "outside the track", "the track bound before the shutter's own rule");
        refuse(go(&c2, cams, 16, 8, 15, 1, 2), RT_ERR_INVALID_ARG, &c2, "outside the track", "the last sub-frame beyond the track");
        refuse(go(&c2, cams, 16, 8, 1, 5, 3), RT_ERR_INVALID_ARG, &c2, "single-GPU", "two workers");
        c2.n_gpus = 1;
        refuse(go(&c2, cams, 16, 8, 1, 5, 3), RT_ERR_UNSUPPORTED, &c2, "does not supersample", "rt_set_supersampling above 1");
        rt_set_supersampling(&c2, 1);
        refuse(go(&c2, cams, 8192, 8192, 1, 5, 3), RT_ERR_INVALID_ARG, &c2, "2^31", "a sample frame above 2^31 - 1");
        // the shutter's own refusals
        for (int bad : {3, 0, -2, 6, 12})
            refuse(go(&c2, cams, 16, 8, 1, 1, bad), RT_ERR_INVALID_ARG, &c2, "is not a power of two", "a shutter that is no power of two");
        refuse(go(&c2, cams, 16, 8, 0, 1, 8), RT_ERR_INVALID_ARG, &c2, "samples per pixel", "m k^2 = 8 * 64 above 256");
        EXPECT(rt_set_path_supersampling(&c2, 2) == RT_OK, "rt_set_path_supersampling");
        refuse(go(&c2, cams, 16, 8, 1, 2, 4), RT_ERR_UNSUPPORTED, &c2, "rt_set_path_adaptive_sampling", "a shutter above 1 under adaptive sampling");
        EXPECT(rt_set_path_adaptive_sampling(&c2, 0) == RT_OK, "rt_set_path_adaptive_sampling");
        // then the band arguments and the output
        if (call == 0) {
            refuse(go(&c2, cams, 16, 8, 1, 2, 4, Bands{0, 0, 1, px, 0, RT_BANDS_INT32}), RT_ERR_INVALID_ARG, &c2, "band", "band_rows 0");
            refuse(go(&c2, cams, 16, 8, 1, 2, 4, Bands{8, 0, 1, nullptr, 0, RT_BANDS_INT32}), RT_ERR_INVALID_ARG, &c2, "band", "NULL d_out");
            refuse(go(&c2, cams, 16, 8, 1, 2, 4, good), RT_ERR_INVALID_ARG, &c2, "frame stride", "a frame stride of 0 with 2 frames");
        } else {
            refuse(go(&c2, cams, 16, 8, 1, 2, 4, good, nullptr), RT_ERR_INVALID_ARG, &c2, "NULL pixels", "NULL pixels");
        }
        // a shutter above RT_MAX_SHUTTER needs a track that holds its sub-frames
        {
            const int M = 2 * RT_MAX_SHUTTER;
            std::vector<rt_sphere> s(S.begin(), S.begin() + 1);
            std::vector<rt_plane> q(P.begin(), P.begin() + 1);
            std::vector<rt_light> l(L.begin(), L.begin() + 1);
            std::vector<rt_vec3> a(A.begin(), A.begin() + 1);
            s.resize((size_t)M, S[0]), q.resize((size_t)M, P[0]), l.resize((size_t)M, L[0]), a.resize((size_t)M, A[0]);
            EXPECT(rt_set_scene_track(&c2, s.data(), 1, q.data(), 1, l.data(), 1, a.data(), 2, M) == RT_OK, "a track of %d frames", M);
            refuse(go(&c2, cams, 16, 8, 0, 1, M), RT_ERR_INVALID_ARG, &c2, "is not a power of two in 1..256", "a shutter of 512");
        }
    }
    // n_frames * shutter <= RT_MAX_PATH_FRAMES: behind the track bound no call reaches it (a track holds at most
    // RT_MAX_PATH_FRAMES frames), so the rule is asked directly
    rt_ctx c3;
    int t = -1;
    refuse(check_shutter(&c3, "rt_render_anim_shutter", RT_MAX_PATH_FRAMES / 2 + 1, 2, &t), RT_ERR_INVALID_ARG, &c3, "cameras", "n_frames * shutter above the bound");
    EXPECT(check_shutter(&c3, "rt_render_anim_shutter", RT_MAX_PATH_FRAMES / 256, 256, &t) == RT_OK && t == 8, "the largest shutter at the bound");
}
}  // namespace

int main() {
    check_variants();
    check_refusals();
    std::printf("anim_shutter_host: %lld variant cases with the field zero (%lld refused, %lld of them a stride with a shutter), %lld with it set "
                "(refused: %lld another value, %lld no stride, %lld unaligned, %lld no shutter, %lld shutter above 8, %lld without views, "
                "%lld adaptive, %lld view_ss not 0 or 1, %lld factor, %lld sums too wide, %lld tiles, %lld stats, %lld ordered, %lld copy slice), "
                "%zu descriptors with the field zero, %zu in all (%zu ANIM_SHUTTER, %zu ANIM_SHUTTER_SS), %d built\n",
                zero_cases, zero_refused, zero_refused_stride_shutter, set_cases, ref_value, ref_no_stride, ref_unaligned, ref_no_shutter,
                ref_shutter_hi, ref_no_views, ref_adapt, ref_view_ss, ref_factor, ref_sums, ref_tiles, ref_stats, ref_ordered, ref_copy, n_zero,
                n_all, n_new[0], n_new[1], n_built);
    std::printf("anim_shutter_host: %ld refusals\n", refusals);
    std::printf("anim_shutter_host: %ld failures\n", failures);
    return failures == 0 && zero_cases > 0 && set_cases > 0 && refusals > 0 ? 0 : 1;
}
