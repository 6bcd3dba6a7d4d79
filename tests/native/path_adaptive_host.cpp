// path_adaptive_host.cpp -- host check of adaptive path and track launches (rt_set_path_adaptive_sampling; DESIGN.md 3
// and 4), TEST INFRASTRUCTURE ONLY.  Plain host C++ against the device-free header rt_internal.h; no device code is
// compiled or linked.
//  Variant selection (rt_internal.h pick_trace_variant) against a restatement.  With LaunchParams::view_adapt zero, over
//  path_ss_host's grid: exactly the earlier rule, 804 distinct descriptors, none in a new mode, the earlier refusals.  With
//  it set: PATH_ADAPT / ANIM_ADAPT exactly with a value in 1..256, views, view_ss = 1, ss_log2 in 1..3 and no shutter, each
//  descriptor the mirror of its PATH_SS / ANIM_SS twin, 60 + 60 split over the entry points as PATH's are, 924 built, the
//  variant word reads back, and every refusal reached.  The field lies in the block's tail padding.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

#include "rt_internal.h"

using namespace rtk;

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

// The rule before view_ss restated, thresholds and mode numbers as literals (neither view_ss nor view_adapt is read).
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
// Today's rule (view_adapt is not read): with view_ss set, views, a factor in 1..3 and sums that fit 16 bits; then the
// twin's launch decides, and PATH (4) / SHUTTER (5) / ANIM (8) become 9 / 10 / 11.
bool expect_zero(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
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
// With the new field set: a value in 1..256 on a supersampled path or track launch without a shutter; then that launch
// (the same block without the threshold) decides, and PATH_SS (9) / ANIM_SS (11) become 12 / 13.
bool expect_set(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.view_adapt == 0) return expect_zero(p, gpow, stats, v);
    if (p.view_adapt < 1 || p.view_adapt > 256) return false;
    if (p.views == nullptr || p.view_ss != 1 || p.ss_log2 < 1 || p.ss_log2 > 3 || p.shutter_log2 != 0) return false;
    LaunchParams q = p;
    q.view_adapt = 0;
    if (!expect_zero(q, gpow, stats, v)) return false;
    if (v->mode != 9 && v->mode != 11) return false;
    v->mode = v->mode == 9 ? 12 : 13;
    return true;
}

long long zero_cases = 0, set_cases = 0, zero_refused = 0;
long long ref_no_views = 0, ref_view_ss = 0, ref_factor0 = 0, ref_factor_hi = 0, ref_shutter = 0, ref_value = 0, ref_tiles = 0,
          ref_stats = 0, ref_ordered = 0, ref_copy = 0;
size_t n_zero = 0, n_all = 0, n_new[2] = {0, 0};
int n_built = 0;
long long mismatches = 0;
std::set<Key> seen_zero, seen;

void check_case(const LaunchParams& p, int gpow, int stats, bool set_phase) {
    TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
    const bool w = expect_set(p, gpow != 0, stats != 0, &want);
    const bool g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
    ++(set_phase ? set_cases : zero_cases);
    if (w != g || (w && key_of(want) != key_of(got))) {
        if (mismatches++ < 10)
            std::fprintf(stderr, "path_adaptive_host: MISMATCH adapt %d view_ss %d stride %llu thr %d sl %d S %d L %d a2 %d limit %d gpow %d "
                         "stats %d fmt %d ss %d views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d "
                         "%d %d %d}\n", p.view_adapt, p.view_ss, p.scene_stride, p.adapt_thr, p.shutter_log2, p.S, p.L, p.lights_a2_ok, p.limit,
                         gpow, stats, p.out_fmt, p.ss_log2, p.views != nullptr, p.n_frames, p.copy_z, p.tile_order != nullptr,
                         p.tile_cost != nullptr, p.row_order_n, p.col_major, (int)w, want.family, want.gpow, want.mode, want.cls, want.K,
                         want.wpg, want.tord, (int)g, got.family, got.gpow, got.mode, got.cls, got.K, got.wpg, got.tord);
        return;
    }
    const bool views = p.views != nullptr, ordered = p.tile_order != nullptr || p.tile_cost != nullptr;
    const int ss = p.ss_log2, sl = p.shutter_log2;
    if (!set_phase && !g) ++zero_refused;
    if (set_phase && !g) {  // which refusal: the first thing the launch lacks
        if (p.view_adapt < 1 || p.view_adapt > 256) ++ref_value;
        else if (!views) ++ref_no_views;
        else if (p.view_ss != 1) ++ref_view_ss;
        else if (ss == 0) ++ref_factor0;
        else if (ss > 3) ++ref_factor_hi;
        else if (sl != 0) ++ref_shutter;
        else if (p.out_fmt == OUT_TILES) ++ref_tiles;
        else if (stats) ++ref_stats;
        else if (ordered) ++ref_ordered;
        else if (p.copy_z) ++ref_copy;
    }
    if (!g) return;
    const bool is_new = got.mode >= TM_PATH_ADAPT;
    EXPECT(is_new == set_phase, "a new mode exactly with the field set");
    if (is_new) {
        EXPECT(p.view_adapt >= 1 && p.view_adapt <= 256 && views && p.view_ss == 1 && ss >= 1 && ss <= 3 && sl == 0,
               "a new mode only with a threshold, views, view_ss = 1, a factor in 1..3 and no shutter");
        EXPECT(got.mode == (p.scene_stride != 0 ? TM_ANIM_ADAPT : TM_PATH_ADAPT), "ANIM_ADAPT with a stride, otherwise PATH_ADAPT");
        LaunchParams q = p;  // the twin: the same launch without the threshold
        q.view_adapt = 0;
        TraceVariant twin{-3, -3, -3, -3, -3, -3, -3};
        const int twin_mode = got.mode == TM_PATH_ADAPT ? TM_PATH_SS : TM_ANIM_SS;
        EXPECT(pick_trace_variant(q, gpow != 0, stats != 0, &twin) && twin.mode == twin_mode, "the twin exists");
        twin.mode = got.mode;
        EXPECT(key_of(twin) == key_of(got), "a new descriptor mirrors its twin field for field");
    }
    if (!set_phase) seen_zero.insert(key_of(got));
    seen.insert(key_of(got));
    EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
    const unsigned word = variant_word(got);
    const unsigned mode_flags = VF_STATS | VF_TILES | VF_SS | VF_PATH | VF_SHUTTER | VF_ADAPT | VF_PROG | VF_ANIM | VF_VIEW_SS | VF_VIEW_ADAPT;
    EXPECT(((word & VF_PATH_ADAPT) != 0) == (got.mode == TM_PATH_ADAPT) && ((word & VF_ANIM_ADAPT) != 0) == (got.mode == TM_ANIM_ADAPT) &&
               ((word & VF_PATH_SS) != 0) == (got.mode == TM_PATH_SS) && ((word & VF_ANIM_SS) != 0) == (got.mode == TM_ANIM_SS) &&
               ((word & VF_SHUTTER_SS) != 0) == (got.mode == TM_SHUTTER_SS) && ((word & VF_ADAPT) != 0) == (got.mode == TM_ADAPT) &&
               ((word & VF_PATH) != 0) == (got.mode == TM_PATH) && ((word & VF_ANIM) != 0) == (got.mode == TM_ANIM) &&
               (!is_new || (word & mode_flags & ~VF_VIEW_ADAPT) == 0) && vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg &&
               vf_tord_of(word) == got.tord && ((word & VF_GPOW) != 0) == (got.gpow != 0),
           "the variant word reads back");
}

void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 8, 9}, thrs[] = {0, 1, 256};
    // passes 0..8: path_ss_host's grid with the new field zero (0..5 anim_host's, 6..8 view_ss set); 9..: the field set --
    // a threshold without and with a stride, the ends of its range, values outside it, and view_ss 0 and 2
    static const unsigned long long strides[] = {0, 0, 256, 1ull << 20, 255, 1000, 0, 256, 0, 0, 256, 0, 256, 0, 0, 0, 256};
    static const int view_sss[] = {0, 0, 0, 0, 0, 0, 1, 1, 2, 1, 1, 1, 1, 1, 1, 0, 2};
    static const int adapts[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 16, 1, 256, -1, 257, 16, 16};
    static uint32_t cell[2];
    static DevView view;
    static ResolveSum acc[4];
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    for (int pass = 0; pass < 17; ++pass)
    for (int thr : thrs) for (int sl : sls)
    for (int S : Ss) for (int L : Ls) for (int a2 = 0; a2 < 2; ++a2) for (int limit : limits)
    for (int gpow = 0; gpow < 2; ++gpow) for (int stats = 0; stats < 2; ++stats) for (int fmt = 0; fmt < 2; ++fmt)
    for (int ss = 0; ss <= 4; ++ss) for (int views = 0; views < 2; ++views) for (int nf = 1; nf <= 2; ++nf)
    for (int cz = 0; cz < 2; ++cz) for (int to = 0; to < 2; ++to) for (int tc = 0; tc < 2; ++tc)
    for (int ro = 0; ro < 2; ++ro) for (int cm = 0; cm < 2; ++cm) {
        if (pass >= 2 && pass < 6 && (thr != 0 || ss > 1)) continue;  // (anim_host's grid)
        if (pass >= 6 && thr == 1) continue;                          // (a launch with views never reads adapt_thr)
        if (pass == 8 && (sl > 1 || limit > 1)) continue;
        if (pass >= 9 && sl > 1) continue;                            // (one shutter is every shutter to the new field)
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
        check_case(p, gpow, stats, pass >= 9);
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_zero = seen_zero.size(), n_all = seen.size();
    EXPECT(n_zero == 804, "804 distinct descriptors with the field zero, got %zu", n_zero);
    EXPECT(n_all == 924, "924 distinct descriptors in all, got %zu", n_all);
    int per_entry[2][2][2] = {}, path_entry[2][2] = {};
    for (const Key& k : seen) {
        const int mode = std::get<2>(k);
        if (mode == TM_PATH) path_entry[std::get<0>(k)][std::get<1>(k)]++;
        if (mode < TM_PATH_ADAPT) continue;
        EXPECT(mode <= TM_ANIM_ADAPT, "no mode beyond ANIM_ADAPT");
        ++n_new[mode - TM_PATH_ADAPT];
        per_entry[mode - TM_PATH_ADAPT][std::get<0>(k)][std::get<1>(k)]++;
        EXPECT(std::get<5>(k) == 1 && std::get<6>(k) == 0, "a new launch has one tile per workgroup in grid order");
        EXPECT(seen_zero.count(k) == 0, "no new descriptor with the field zero");
    }
    for (int i = 0; i < 2; ++i) {
        EXPECT(n_new[i] == 60, "60 descriptors of new mode %d, got %zu", TM_PATH_ADAPT + i, n_new[i]);
        EXPECT(std::memcmp(per_entry[i], path_entry, sizeof path_entry) == 0, "mode %d's split over the entry points is PATH's",
               TM_PATH_ADAPT + i);
    }
    EXPECT(path_entry[0][0] == 12 && path_entry[0][1] == 12 && path_entry[1][0] == 18 && path_entry[1][1] == 18,
           "direct 12 + 12 GPOW, bundle 18 + 18 GPOW");
    EXPECT(ref_no_views > 0 && ref_view_ss > 0 && ref_factor0 > 0 && ref_factor_hi > 0 && ref_shutter > 0 && ref_value > 0 &&
               ref_tiles > 0 && ref_stats > 0 && ref_ordered > 0 && ref_copy > 0,
           "every refusal of the field was reached");
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m <= TM_ANIM_ADAPT; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built == 924, "924 built descriptors, got %d", n_built);
    static_assert(sizeof(LaunchParams) < 4096, "the kernarg block");
    static_assert(TM_PATH_ADAPT == 12 && TM_ANIM_ADAPT == 13, "the new modes follow ANIM_SS");
    static_assert(VF_PATH_ADAPT > (1u << 21) && VF_ANIM_ADAPT > (1u << 21) && VF_PATH_ADAPT != VF_ANIM_ADAPT, "their flags sit above bit 21");
    static_assert((VF_VIEW_ADAPT & (vf_cls(15) | vf_wpg(15) | vf_tord(3) | 0xffu | VF_ANIM | VF_VIEW_SS)) == 0, "and on no earlier bit");
    static_assert(offsetof(LaunchParams, view_adapt) == offsetof(LaunchParams, view_ss) + sizeof(int), "the field follows view_ss");
    static_assert(sizeof(LaunchParams) == offsetof(LaunchParams, view_ss) + 8, "in the tail padding: the block keeps its size");
    static_assert(offsetof(LaunchParams, view_ss) == offsetof(LaunchParams, scene_stride) + 8, "view_ss right behind scene_stride");
}
}  // namespace

int main() {
    check_variants();
    std::printf("path_adaptive_host: %lld variant cases with the field zero (%lld refused), %lld with it set (refused: %lld without views, "
                "%lld view_ss not 1, %lld factor 0, %lld factor above 3, %lld shutter, %lld value outside 1..256, %lld tiles, %lld stats, "
                "%lld ordered, %lld copy slice), %zu descriptors with the field zero, %zu in all (%zu PATH_ADAPT, %zu ANIM_ADAPT), %d built\n",
                zero_cases, zero_refused, set_cases, ref_no_views, ref_view_ss, ref_factor0, ref_factor_hi, ref_shutter, ref_value, ref_tiles,
                ref_stats, ref_ordered, ref_copy, n_zero, n_all, n_new[0], n_new[1], n_built);
    std::printf("path_adaptive_host: %ld failures\n", failures);
    return failures == 0 ? 0 : 1;
}
