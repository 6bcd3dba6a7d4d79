// shutter_adaptive_host.cpp -- host check of adaptive shutters (rt_set_shutter_adaptive_sampling), TEST
// INFRASTRUCTURE ONLY.  rt_api.cpp is compiled into this translation unit (its helpers have internal linkage); no device
// call is reached (contexts without devices).  Built plain and under host-side ASan + UBSan (shutter_adaptive.mk).
//  1. Variant selection (rt_internal.h pick_trace_variant) against a restatement.  With LaunchParams::shutter_adapt zero,
//     over the earlier sweep of every field the rule reads: exactly the earlier rule, 1044 distinct descriptors, none in a
//     new mode, the earlier refusals (view_adapt with a shutter among them).  With it set: SHUTTER_ADAPT /
//     ANIM_SHUTTER_ADAPT exactly with a value in 1..256, views, view_ss = 1, a factor in 1..3, shutter_log2 >= 1,
//     shutter_log2 + 2 ss_log2 <= 8, no view_adapt and scene_shutter consistent with scene_stride; each descriptor the
//     mirror of its SHUTTER_SS / ANIM_SHUTTER_SS twin (the same launch without the threshold), counted per entry point,
//     the variant words distinct and the earlier words unchanged, every refusal reached.
//  2. The layout: the field lies in padding inside the block, no field moves, the block keeps its size.
//  3. The setting through the C ABI: bounds, the refusal gated on it, the band rule while it is in effect.
#include "../../uu-infogr-raytracer_amd/csrc/rt_api.cpp"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
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
// The rule before view_ss restated, thresholds and mode numbers as literals.
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
// ... with view_ss: PATH (4) / SHUTTER (5) / ANIM (8) become 9 / 10 / 11 ...
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
// ... with view_adapt (never with a shutter): PATH_SS (9) / ANIM_SS (11) become 12 / 13 ...
bool expect_adapt(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
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
// ... and with scene_shutter: SHUTTER (5) / SHUTTER_SS (10) become 14 / 15.  This is today's rule (shutter_adapt is not read).
bool expect_today(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.scene_shutter == 0) return expect_adapt(p, gpow, stats, v);
    if (p.scene_shutter != 1 || p.scene_stride == 0 || p.scene_stride % 256 != 0 || p.shutter_log2 < 1 || p.view_adapt != 0) return false;
    LaunchParams q = p;
    q.scene_shutter = 0, q.scene_stride = 0;
    if (!expect_adapt(q, gpow, stats, v)) return false;
    if (v->mode != 5 && v->mode != 10) return false;
    v->mode = v->mode == 5 ? 14 : 15;
    return true;
}
// With the new field set: a value in 1..256 on a supersampled shutter launch without view_adapt; then the same launch
// without the threshold decides, and SHUTTER_SS (10) / ANIM_SHUTTER_SS (15) become 16 / 17.
bool expect_new(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.shutter_adapt == 0) return expect_today(p, gpow, stats, v);
    if (p.shutter_adapt < 1 || p.shutter_adapt > 256) return false;
    if (p.views == nullptr || p.view_ss != 1 || p.ss_log2 < 1 || p.ss_log2 > 3 || p.shutter_log2 < 1 || p.shutter_log2 + 2 * p.ss_log2 > 8 ||
        p.view_adapt != 0)
        return false;
    LaunchParams q = p;
    q.shutter_adapt = 0;
    if (!expect_today(q, gpow, stats, v)) return false;
    if (v->mode != 10 && v->mode != 15) return false;
    v->mode = v->mode == 10 ? 16 : 17;
    return true;
}

long long zero_cases = 0, set_cases = 0, zero_refused = 0, zero_refused_adapt_shutter = 0;
long long ref_value = 0, ref_no_views = 0, ref_view_ss = 0, ref_factor = 0, ref_no_shutter = 0, ref_shutter_hi = 0, ref_sums = 0, ref_view_adapt = 0,
          ref_scene = 0, ref_tiles = 0, ref_stats = 0, ref_ordered = 0, ref_copy = 0;
size_t n_zero = 0, n_all = 0, n_new[2] = {0, 0};
int n_built = 0;
long long mismatches = 0;
std::set<Key> seen_zero, seen;
std::map<std::tuple<int, unsigned, int>, Key> words;  // (the family, the word and K name an instantiation)

void check_case(const LaunchParams& p, int gpow, int stats, bool set_phase) {
    TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
    const bool w = expect_new(p, gpow != 0, stats != 0, &want);
    const bool g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
    ++(set_phase ? set_cases : zero_cases);
    if (w != g || (w && key_of(want) != key_of(got))) {
        if (mismatches++ < 10)
            std::fprintf(stderr, "shutter_adaptive_host: MISMATCH sa %d mark %d adapt %d view_ss %d stride %llu thr %d sl %d S %d L %d a2 %d limit %d "
                         "gpow %d stats %d fmt %d ss %d views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d "
                         "{%d %d %d %d %d %d %d}\n", p.shutter_adapt, p.scene_shutter, p.view_adapt, p.view_ss, p.scene_stride, p.adapt_thr,
                         p.shutter_log2, p.S, p.L, p.lights_a2_ok, p.limit, gpow, stats, p.out_fmt, p.ss_log2, p.views != nullptr, p.n_frames, p.copy_z,
                         p.tile_order != nullptr, p.tile_cost != nullptr, p.row_order_n, p.col_major, (int)w, want.family, want.gpow, want.mode,
                         want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow, got.mode, got.cls, got.K, got.wpg, got.tord);
        return;
    }
    const bool views = p.views != nullptr, ordered = p.tile_order != nullptr || p.tile_cost != nullptr;
    const int ss = p.ss_log2, sl = p.shutter_log2;
    if (!set_phase && !g) {
        ++zero_refused;
        if (views && p.view_adapt >= 1 && p.view_adapt <= 256 && p.view_ss == 1 && ss >= 1 && ss <= 3 && sl >= 1 && sl + 2 * ss <= 8)
            ++zero_refused_adapt_shutter;
    }
    if (set_phase && !g) {  // which refusal: the first thing the launch lacks
        if (p.shutter_adapt < 1 || p.shutter_adapt > 256) ++ref_value;
        else if (!views) ++ref_no_views;
        else if (p.view_ss != 1) ++ref_view_ss;
        else if (ss < 1 || ss > 3) ++ref_factor;
        else if (sl < 1) ++ref_no_shutter;
        else if (sl > 8) ++ref_shutter_hi;
        else if (sl + 2 * ss > 8) ++ref_sums;
        else if (p.view_adapt != 0) ++ref_view_adapt;
        else if ((p.scene_shutter != 0) != (p.scene_stride != 0) || p.scene_stride % 256 != 0 || (p.scene_shutter != 0 && p.scene_shutter != 1)) ++ref_scene;
        else if (p.out_fmt == OUT_TILES) ++ref_tiles;
        else if (stats) ++ref_stats;
        else if (ordered) ++ref_ordered;
        else if (p.copy_z) ++ref_copy;
    }
    if (!g) return;
    const bool is_new = got.mode >= TM_SHUTTER_ADAPT;
    EXPECT(is_new == set_phase, "a new mode exactly with the field set");
    if (is_new) {
        EXPECT(p.shutter_adapt >= 1 && p.shutter_adapt <= 256 && views && p.view_ss == 1 && ss >= 1 && ss <= 3 && sl >= 1 && sl + 2 * ss <= 8 &&
                   p.view_adapt == 0,
               "a new mode only with a threshold, views, view_ss, a factor, a shutter, sums that fit and no view_adapt");
        EXPECT(got.mode == (p.scene_shutter != 0 ? TM_ANIM_SHUTTER_ADAPT : TM_SHUTTER_ADAPT), "ANIM_SHUTTER_ADAPT with scene_shutter, otherwise SHUTTER_ADAPT");
        EXPECT((p.scene_shutter != 0) == (p.scene_stride != 0), "scene_shutter consistent with scene_stride");
        LaunchParams q = p;  // the twin: the fully supersampled launch
        q.shutter_adapt = 0;
        TraceVariant twin{-3, -3, -3, -3, -3, -3, -3};
        const int twin_mode = got.mode == TM_SHUTTER_ADAPT ? TM_SHUTTER_SS : TM_ANIM_SHUTTER_SS;
        EXPECT(pick_trace_variant(q, gpow != 0, stats != 0, &twin) && twin.mode == twin_mode, "the twin exists");
        twin.mode = got.mode;
        EXPECT(key_of(twin) == key_of(got), "a new descriptor mirrors its twin field for field");
    }
    if (!set_phase) seen_zero.insert(key_of(got));
    seen.insert(key_of(got));
    EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
    const unsigned word = variant_word(got);
    const auto ins = words.emplace(std::make_tuple(got.family, word, got.K), key_of(got));
    EXPECT(ins.first->second == key_of(got), "two descriptors share the variant word %#x at K %d", word, got.K);
    const unsigned old_flags = VF_STATS | VF_TILES | VF_SS | VF_PATH | VF_SHUTTER | VF_ADAPT | VF_PROG | VF_ANIM | VF_VIEW_SS | VF_VIEW_ADAPT |
                               VF_ANIM_SHUTTER | VF_ANIM_SHUTTER_SS;
    EXPECT(((word & VF_SHUTTER_ADAPT) != 0) == (got.mode == TM_SHUTTER_ADAPT) && ((word & VF_ANIM_SHUTTER_ADAPT) != 0) == (got.mode == TM_ANIM_SHUTTER_ADAPT) &&
               ((word & VF_SHUTTER_SS) != 0) == (got.mode == TM_SHUTTER_SS) && ((word & VF_ANIM_SHUTTER_SS) != 0) == (got.mode == TM_ANIM_SHUTTER_SS) &&
               (!is_new || (word & old_flags) == 0) && (is_new || (word & VF_VIEW_SHUTTER_ADAPT) == 0) && vf_cls_of(word) == got.cls &&
               vf_wpg_of(word) == got.wpg && vf_tord_of(word) == got.tord && ((word & VF_GPOW) != 0) == (got.gpow != 0),
           "the variant word reads back");
    if (!is_new) {  // an earlier word is what the flags before this field made it: nothing above bit 25
        EXPECT((word >> 26) == 0, "an earlier descriptor's word has no bit above 25");
    }
}

void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 4, 8, 9, -1}, thrs[] = {0, 1, 256};
    // passes 0..11: the new field zero -- the earlier sweep: plain, progressive, a stride (aligned, unaligned), view_ss without
    // and with a stride, the adaptive twins, view_ss = 2, scene_shutter without and with view_ss, and with view_adapt;
    // 12..: the field set -- camera and track shutters, without view_ss, view_ss = 2, with view_adapt, a stride without the
    // mark, the mark without a stride, an unaligned stride, the values 256, 257, -1 and 1
    constexpr int PASSES = 25, SET_FROM = 12;
    static const unsigned long long strides[PASSES] = {0, 0, 256, 255, 0, 256, 256, 0, 0, 256, 256, 256, 0, 256, 0, 0, 0, 256, 0, 255, 0, 0, 0, 256, 1ull << 20};
    static const int view_sss[PASSES] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 0, 1, 1, 1, 1, 0, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    static const int adapts[PASSES] = {0, 0, 0, 0, 0, 0, 16, 16, 0, 0, 0, 16, 0, 0, 0, 0, 16, 0, 0, 0, 0, 0, 0, 0, 0};
    static const int marks[PASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 2};
    static const int sas[PASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 96, 96, 96, 96, 96, 96, 96, 96, 256, 257, -1, 1, 96};
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
        if (pass >= 14 && limit > 1) continue;
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
        p.shutter_adapt = sas[pass];
        check_case(p, gpow, stats, pass >= SET_FROM);
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_zero = seen_zero.size(), n_all = seen.size();
    EXPECT(n_zero == 1044, "1044 distinct descriptors with the field zero, got %zu", n_zero);
    EXPECT(zero_refused_adapt_shutter > 0, "with the field zero view_adapt with a shutter is refused");
    int per_entry[2][2][2] = {}, path_entry[2][2] = {};
    for (const Key& k : seen) {
        const int mode = std::get<2>(k);
        if (mode == TM_PATH) path_entry[std::get<0>(k)][std::get<1>(k)]++;
        if (mode < TM_SHUTTER_ADAPT) continue;
        EXPECT(mode <= TM_ANIM_SHUTTER_ADAPT, "no mode beyond ANIM_SHUTTER_ADAPT");
        ++n_new[mode - TM_SHUTTER_ADAPT];
        per_entry[mode - TM_SHUTTER_ADAPT][std::get<0>(k)][std::get<1>(k)]++;
        EXPECT(std::get<5>(k) == 1 && std::get<6>(k) == 0, "a new launch has one tile per workgroup in grid order");
        EXPECT(seen_zero.count(k) == 0, "no new descriptor with the field zero");
    }
    for (int i = 0; i < 2; ++i)
        EXPECT(std::memcmp(per_entry[i], path_entry, sizeof path_entry) == 0, "mode %d's split over the entry points is PATH's", TM_SHUTTER_ADAPT + i);
    EXPECT(n_all == n_zero + n_new[0] + n_new[1], "every descriptor beyond the earlier ones is in a new mode");
    EXPECT(words.size() == n_all, "the variant words are distinct: %zu words, %zu descriptors", words.size(), n_all);
    EXPECT(ref_value > 0 && ref_no_views > 0 && ref_view_ss > 0 && ref_factor > 0 && ref_no_shutter > 0 && ref_shutter_hi > 0 && ref_sums > 0 &&
               ref_view_adapt > 0 && ref_scene > 0 && ref_tiles > 0 && ref_stats > 0 && ref_ordered > 0 && ref_copy > 0,
           "every refusal of the field was reached");
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    int n_built_before = 0;
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m <= TM_ANIM_SHUTTER_ADAPT; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        if (m < TM_SHUTTER_ADAPT) ++n_built_before;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built_before == 1044, "1044 descriptors built before the new modes, got %d", n_built_before);
    EXPECT((size_t)n_built == n_all, "the built descriptors are those the selection returns: %d built, %zu returned", n_built, n_all);
}

// ---- 2. layout -------------------------------------------------------------------------------------------------------
void check_layout() {
    static_assert(sizeof(LaunchParams) < 4096, "the kernarg block");
    static_assert(TM_SHUTTER_ADAPT == 16 && TM_ANIM_SHUTTER_ADAPT == 17, "the new modes follow ANIM_SHUTTER_SS");
    static_assert(VF_SHUTTER_ADAPT > (1u << 25) && VF_ANIM_SHUTTER_ADAPT > (1u << 25) && VF_SHUTTER_ADAPT != VF_ANIM_SHUTTER_ADAPT, "their flags sit above bit 25");
    static_assert((VF_VIEW_SHUTTER_ADAPT & (vf_cls(15) | vf_wpg(15) | vf_tord(3) | 0xffu | VF_ANIM | VF_VIEW_SS | VF_VIEW_ADAPT | VF_ANIM_SHUTTER | VF_ANIM_SHUTTER_SS)) == 0,
                  "and on no earlier bit");
    static_assert(offsetof(LaunchParams, shutter_adapt) == offsetof(LaunchParams, enc_frame0) + sizeof(int), "the field follows enc_frame0");
    static_assert(offsetof(LaunchParams, counters) == offsetof(LaunchParams, shutter_adapt) + sizeof(int), "in the padding ahead of counters: no field moves");
    static_assert(offsetof(LaunchParams, out_fmt) == 232 && offsetof(LaunchParams, enc_frame0) == 264 && offsetof(LaunchParams, counters) == 272, "the offsets around it");
    static_assert(offsetof(LaunchParams, views) == 3352 && offsetof(LaunchParams, view_ss) == 3472 && offsetof(LaunchParams, view_adapt) == 3476, "views, view_ss and view_adapt stay");
    static_assert(sizeof(LaunchParams) == offsetof(LaunchParams, view_ss) + 8 && sizeof(LaunchParams) == 3480, "and the block keeps its size");
    LaunchParams p;
    std::memset(&p, 0xff, sizeof p);
    p.shutter_adapt = 0;
    const unsigned char* b = (const unsigned char*)&p;
    for (size_t i = 0; i < sizeof p; ++i)
        EXPECT((b[i] == 0) == (i >= offsetof(LaunchParams, shutter_adapt) && i < offsetof(LaunchParams, shutter_adapt) + sizeof(int)), "byte %zu", i);
}

// ---- 3. the setting through the C ABI --------------------------------------------------------------------------------
long refusals = 0;
void refuse(int got, int want, const rt_ctx* ctx, const char* text, const char* what) {
    const char* msg = rt_last_error(ctx);
    EXPECT(got == want, "%s: status %d, expected %d (%s)", what, got, want, msg ? msg : "");
    EXPECT(msg && std::strstr(msg, text), "%s: error text \"%s\" lacks \"%s\"", what, msg ? msg : "", text);
    ++refusals;
}
void check_api() {
    rt_ctx c;
    int t = -7;
    EXPECT(rt_get_shutter_adaptive_sampling(&c, &t) == RT_OK && t == 0, "a context that never called the setter reads 0");
    refuse(rt_set_shutter_adaptive_sampling(nullptr, 8), RT_ERR_INVALID_ARG, nullptr, "NULL context", "NULL context");
    refuse(rt_get_shutter_adaptive_sampling(nullptr, &t), RT_ERR_INVALID_ARG, nullptr, "NULL argument", "getter, NULL context");
    refuse(rt_get_shutter_adaptive_sampling(&c, nullptr), RT_ERR_INVALID_ARG, nullptr, "NULL argument", "getter, NULL out");
    for (int bad : {-1, 257, 1 << 20})
        refuse(rt_set_shutter_adaptive_sampling(&c, bad), RT_ERR_INVALID_ARG, &c, "is not in 0..256", "a threshold outside 0..256");
    for (int good : {256, 1, 0, 96}) EXPECT(rt_set_shutter_adaptive_sampling(&c, good) == RT_OK && rt_get_shutter_adaptive_sampling(&c, &t) == RT_OK && t == good, "threshold %d", good);
    EXPECT(rt_abi_version() == 10, "ABI 10");
    int pt = -1, at = -1;
    EXPECT(rt_get_path_adaptive_sampling(&c, &pt) == RT_OK && pt == 0 && rt_get_adaptive_sampling(&c, &at) == RT_OK && at == 0, "the other thresholds are their own");
    // check_shutter: the refusal is the answer while the shutter threshold is 0
    EXPECT(rt_set_path_supersampling(&c, 2) == RT_OK && rt_set_path_adaptive_sampling(&c, 16) == RT_OK, "the path factor and threshold");
    EXPECT(check_shutter(&c, "rt_render_shutter", 3, 4, &t) == RT_OK && t == 2, "both thresholds set: no refusal");
    EXPECT(check_shutter(&c, "rt_render_shutter", 3, 1, &t) == RT_OK && t == 0, "shutter 1");
    EXPECT(rt_set_shutter_adaptive_sampling(&c, 0) == RT_OK, "off");
    refuse(check_shutter(&c, "rt_render_shutter", 3, 4, &t), RT_ERR_UNSUPPORTED, &c, "rt_set_path_adaptive_sampling", "the path threshold alone: the refusal");
    EXPECT(check_shutter(&c, "rt_render_shutter", 3, 1, &t) == RT_OK, "shutter 1 under the path threshold");
    EXPECT(rt_set_path_supersampling(&c, 1) == RT_OK && check_shutter(&c, "rt_render_shutter", 3, 4, &t) == RT_OK, "k = 1: nothing is in effect");
    EXPECT(rt_set_path_supersampling(&c, 8) == RT_OK && rt_set_shutter_adaptive_sampling(&c, 96) == RT_OK, "k = 8");
    refuse(check_shutter(&c, "rt_render_shutter", 3, 8, &t), RT_ERR_INVALID_ARG, &c, "samples per pixel", "m k^2 = 8 * 64 above 256, threshold or not");
    // check_path_adaptive_bands: with a shutter the shutter threshold's rule, without one the path threshold's
    EXPECT(rt_set_path_supersampling(&c, 2) == RT_OK && rt_set_path_adaptive_sampling(&c, 0) == RT_OK, "k = 2, path threshold off");
    refuse(check_path_adaptive_bands(&c, "rt_render_shutter_bands", 12, 30, 1), RT_ERR_UNSUPPORTED, &c, "multiple of 8 rows", "12-row bands while in effect");
    EXPECT(check_path_adaptive_bands(&c, "rt_render_shutter_bands", 8, 30, 1) == RT_OK && check_path_adaptive_bands(&c, "x", 16, 30, 3) == RT_OK &&
               check_path_adaptive_bands(&c, "x", 30, 30, 1) == RT_OK && check_path_adaptive_bands(&c, "x", 37, 30, 1) == RT_OK,
           "multiples of 8 and whole frames pass");
    EXPECT(check_path_adaptive_bands(&c, "rt_render_path_bands", 12, 30, 0) == RT_OK, "shutter 1 ignores the shutter threshold");
    EXPECT(rt_set_shutter_adaptive_sampling(&c, 0) == RT_OK && check_path_adaptive_bands(&c, "x", 12, 30, 1) == RT_OK, "threshold 0: no band rule");
    EXPECT(rt_set_path_adaptive_sampling(&c, 16) == RT_OK, "path threshold");
    refuse(check_path_adaptive_bands(&c, "rt_render_path_bands", 12, 30, 0), RT_ERR_UNSUPPORTED, &c, "multiple of 8 rows", "the path threshold's rule at shutter 1");
    EXPECT(rt_set_shutter_adaptive_sampling(&c, 96) == RT_OK && rt_set_path_supersampling(&c, 1) == RT_OK && check_path_adaptive_bands(&c, "x", 12, 30, 1) == RT_OK,
           "k = 1: not in effect");
}
}  // namespace

int main() {
    check_variants();
    check_layout();
    check_api();
    std::printf("shutter_adaptive_host: %lld variant cases with the field zero (%lld refused, %lld of them view_adapt with a shutter), %lld with it set "
                "(refused: %lld value, %lld without views, %lld view_ss not 1, %lld factor, %lld no shutter, %lld shutter above 8, %lld sums too wide, "
                "%lld view_adapt, %lld scene, %lld tiles, %lld stats, %lld ordered, %lld copy slice), "
                "%zu descriptors with the field zero, %zu in all (%zu SHUTTER_ADAPT, %zu ANIM_SHUTTER_ADAPT), %d built\n",
                zero_cases, zero_refused, zero_refused_adapt_shutter, set_cases, ref_value, ref_no_views, ref_view_ss, ref_factor, ref_no_shutter,
                ref_shutter_hi, ref_sums, ref_view_adapt, ref_scene, ref_tiles, ref_stats, ref_ordered, ref_copy, n_zero, n_all, n_new[0], n_new[1], n_built);
    std::printf("shutter_adaptive_host: %ld refusals\n", refusals);
    std::printf("shutter_adaptive_host: %ld failures\n", failures);
    return failures == 0 && zero_cases > 0 && set_cases > 0 && refusals > 0 ? 0 : 1;
}
