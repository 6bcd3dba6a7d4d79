// path_ss_host.cpp -- host check of supersampled path, shutter and track launches (rt_set_path_supersampling; DESIGN.md
// 3 and 4), TEST INFRASTRUCTURE ONLY.  Plain host C++ against the device-free headers rt_internal.h and rt_resolve.h;
// no device code is compiled or linked.
//  1. Variant selection (rt_internal.h pick_trace_variant) against a restatement.  With LaunchParams::view_ss zero, over
//     anim_host's grid: exactly the earlier rule, 624 distinct descriptors, none in a new mode.  With it set: PATH_SS /
//     SHUTTER_SS / ANIM_SS exactly with views and ss_log2 in 1..3 (a shutter whose sums fit), each descriptor the mirror
//     of its PATH / SHUTTER / ANIM twin, 60 + 60 + 60 split over the entry points as PATH's are, 804 built, and every
//     refusal reached.
//  2. The arithmetic of the single rounding (rt_resolve.h): resolve_round_n of the field-wise sum of n = 2^(t + 2s)
//     unpacked samples is the integer mean per channel, on the extreme inputs and on random ones.
//  3. The butterfly's lane pattern restated as xor steps: every k x k block of an 8x8 tile is summed exactly once into
//     its lanes, the leader among them, for k = 2, 4, 8.
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

uint64_t rng = 0x5A4D91E55ull;
uint64_t next64() {
    uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- 1. variant selection ------------------------------------------------------------------------------------------
using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// Today's rule restated, thresholds and mode numbers as literals (view_ss is not read).
bool expect_zero(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
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
// With the field set: views, a factor in 1..3 and sums that fit 16 bits; then the twin's launch (the same block without
// the factor) decides, and PATH (4) / SHUTTER (5) / ANIM (8) become 9 / 10 / 11.
bool expect_set(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.view_ss == 0) return expect_zero(p, gpow, stats, v);
    if (p.view_ss != 1 || p.views == nullptr || p.ss_log2 < 1 || p.ss_log2 > 3) return false;
    if ((1 << p.ss_log2) * (1 << p.ss_log2) * (p.shutter_log2 > 0 ? 1ll << (p.shutter_log2 > 30 ? 30 : p.shutter_log2) : 1ll) > 256)
        return false;
    LaunchParams q = p;
    q.ss_log2 = 0, q.view_ss = 0;
    if (!expect_zero(q, gpow, stats, v)) return false;
    if (v->mode != 4 && v->mode != 5 && v->mode != 8) return false;
    v->mode = v->mode == 4 ? 9 : v->mode == 5 ? 10 : 11;
    return true;
}

long long zero_cases = 0, set_cases = 0;
long long ref_tiles = 0, ref_stats = 0, ref_ordered = 0, ref_copy = 0, ref_ss = 0, ref_no_views = 0, ref_sum = 0, ref_value = 0;
size_t n_zero = 0, n_all = 0, n_new[3] = {0, 0, 0};
int n_built = 0;
void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 8, 9}, thrs[] = {0, 1, 256};
    // passes 0..5: anim_host's grid with the field zero; 6..8: the field set, without and with a stride, and with
    // another value than 1
    static const unsigned long long strides[] = {0, 0, 256, 1ull << 20, 255, 1000, 0, 256, 0};
    static const int fields[] = {0, 0, 0, 0, 0, 0, 1, 1, 2};
    static uint32_t cell[2];
    static DevView view;
    static ResolveSum acc[4];
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    long long mismatches = 0;
    std::set<Key> seen_zero, seen;
    for (int pass = 0; pass < 9; ++pass)
    for (int thr : thrs) for (int sl : sls)
    for (int S : Ss) for (int L : Ls) for (int a2 = 0; a2 < 2; ++a2) for (int limit : limits)
    for (int gpow = 0; gpow < 2; ++gpow) for (int stats = 0; stats < 2; ++stats) for (int fmt = 0; fmt < 2; ++fmt)
    for (int ss = 0; ss <= 4; ++ss) for (int views = 0; views < 2; ++views) for (int nf = 1; nf <= 2; ++nf)
    for (int cz = 0; cz < 2; ++cz) for (int to = 0; to < 2; ++to) for (int tc = 0; tc < 2; ++tc)
    for (int ro = 0; ro < 2; ++ro) for (int cm = 0; cm < 2; ++cm) {
        if (pass >= 2 && pass < 6 && (thr != 0 || ss > 1)) continue;  // (anim_host's grid)
        if (pass >= 6 && thr == 1) continue;                          // (a launch with views never reads the threshold)
        if (pass == 8 && (sl > 1 || limit > 1)) continue;
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
        p.view_ss = fields[pass];
        TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
        const bool w = expect_set(p, gpow != 0, stats != 0, &want);
        const bool g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
        ++(pass >= 6 ? set_cases : zero_cases);
        if (w != g || (w && key_of(want) != key_of(got))) {
            if (mismatches++ < 10)
                std::fprintf(stderr, "path_ss_host: MISMATCH pass %d thr %d sl %d S %d L %d a2 %d limit %d gpow %d stats %d fmt %d ss %d "
                             "views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d %d %d %d}\n",
                             pass, thr, sl, S, L, a2, limit, gpow, stats, fmt, ss, views, nf, cz, to, tc, ro, cm, (int)w, want.family,
                             want.gpow, want.mode, want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow,
                             got.mode, got.cls, got.K, got.wpg, got.tord);
            continue;
        }
        const bool in_range = views && ss >= 1 && ss <= 3;
        if (pass >= 6 && !g) {  // which refusal: the launch that lacks only this one thing would have been taken
            if (pass == 8) ++ref_value;
            else if (!views) ++ref_no_views;
            else if (ss > 3) ++ref_ss;
            else if (in_range && sl + 2 * ss > 8 && sl <= 8) ++ref_sum;
            else if (in_range && fmt) ++ref_tiles;
            else if (in_range && stats) ++ref_stats;
            else if (in_range && (to || tc)) ++ref_ordered;
            else if (in_range && cz) ++ref_copy;
        }
        if (!g) continue;
        const bool is_new = got.mode >= TM_PATH_SS;
        EXPECT(is_new == (pass >= 6), "a new mode exactly with the field set");
        if (is_new) {
            EXPECT(pass != 8 && in_range && sl + 2 * ss <= 8, "a new mode only with views, a factor in 1..3 and sums that fit");
            const int expect_mode = sl > 0 ? TM_SHUTTER_SS : strides[pass] != 0 ? TM_ANIM_SS : TM_PATH_SS;
            EXPECT(got.mode == expect_mode, "SHUTTER_SS with a shutter, ANIM_SS with a stride, otherwise PATH_SS");
            LaunchParams q = p;  // the twin: the same launch without the factor
            q.ss_log2 = 0, q.view_ss = 0;
            TraceVariant twin{-3, -3, -3, -3, -3, -3, -3};
            const int twin_mode = got.mode == TM_PATH_SS ? TM_PATH : got.mode == TM_SHUTTER_SS ? TM_SHUTTER : TM_ANIM;
            EXPECT(pick_trace_variant(q, gpow != 0, stats != 0, &twin) && twin.mode == twin_mode, "the twin exists");
            twin.mode = got.mode;
            EXPECT(key_of(twin) == key_of(got), "a new descriptor mirrors its twin field for field");
        }
        if (pass < 6) seen_zero.insert(key_of(got));
        seen.insert(key_of(got));
        EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
        const unsigned word = variant_word(got);
        EXPECT(((word & VF_PATH_SS) != 0) == (got.mode == TM_PATH_SS) && ((word & VF_SHUTTER_SS) != 0) == (got.mode == TM_SHUTTER_SS) &&
                   ((word & VF_ANIM_SS) != 0) == (got.mode == TM_ANIM_SS) && ((word & VF_PATH) != 0) == (got.mode == TM_PATH) &&
                   ((word & VF_SHUTTER) != 0) == (got.mode == TM_SHUTTER) && ((word & VF_ANIM) != 0) == (got.mode == TM_ANIM) &&
                   ((word & VF_SS) != 0) == (got.mode == TM_SS) && vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg &&
                   vf_tord_of(word) == got.tord && ((word & VF_GPOW) != 0) == (got.gpow != 0),
               "the variant word reads back");
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    n_zero = seen_zero.size(), n_all = seen.size();
    EXPECT(n_zero == 624, "624 distinct descriptors with the field zero, got %zu", n_zero);
    EXPECT(n_all == 804, "804 distinct descriptors in all, got %zu", n_all);
    int per_entry[3][2][2] = {}, path_entry[2][2] = {};
    for (const Key& k : seen) {
        const int mode = std::get<2>(k);
        if (mode == TM_PATH) path_entry[std::get<0>(k)][std::get<1>(k)]++;
        if (mode < TM_PATH_SS) continue;
        EXPECT(mode <= TM_ANIM_SS, "no mode beyond ANIM_SS");
        ++n_new[mode - TM_PATH_SS];
        per_entry[mode - TM_PATH_SS][std::get<0>(k)][std::get<1>(k)]++;
        EXPECT(std::get<5>(k) == 1 && std::get<6>(k) == 0, "a new launch has one tile per workgroup in grid order");
        EXPECT(seen_zero.count(k) == 0, "no new descriptor with the field zero");
    }
    for (int i = 0; i < 3; ++i) {
        EXPECT(n_new[i] == 60, "60 descriptors of new mode %d, got %zu", TM_PATH_SS + i, n_new[i]);
        EXPECT(std::memcmp(per_entry[i], path_entry, sizeof path_entry) == 0, "mode %d's split over the entry points is PATH's",
               TM_PATH_SS + i);
    }
    EXPECT(path_entry[0][0] == 12 && path_entry[0][1] == 12 && path_entry[1][0] == 18 && path_entry[1][1] == 18,
           "direct 12 + 12 GPOW, bundle 18 + 18 GPOW");
    EXPECT(ref_tiles > 0 && ref_stats > 0 && ref_ordered > 0 && ref_copy > 0 && ref_ss > 0 && ref_no_views > 0 && ref_sum > 0 &&
               ref_value > 0,
           "every refusal of the field was reached");
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m <= TM_ANIM_SS; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built == 804, "804 built descriptors, got %d", n_built);
    static_assert(sizeof(LaunchParams) < 4096, "the kernarg block");
    static_assert(TM_PATH_SS == 9 && TM_SHUTTER_SS == 10 && TM_ANIM_SS == 11, "the new modes follow ANIM");
    static_assert(VF_PATH_SS > VF_ANIM && VF_SHUTTER_SS > VF_ANIM && VF_ANIM_SS > VF_ANIM, "their flags sit above ANIM's");
    static_assert(offsetof(LaunchParams, view_ss) > offsetof(LaunchParams, scene_stride), "the field is the last one");
    static_assert(offsetof(LaunchParams, view_ss) + sizeof(int) + 4 >= sizeof(LaunchParams), "nothing but padding follows it");
}

// ---- 2. the single rounding ----------------------------------------------------------------------------------------
long long rounded = 0;
void check_one(const uint32_t* px, int n, int bits) {
    ResolveSum sum{0u, 0u};
    unsigned c[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        sum = resolve_add(sum, resolve_unpack(px[i]));
        c[0] += (px[i] >> 16) & 0xffu, c[1] += (px[i] >> 8) & 0xffu, c[2] += px[i] & 0xffu;
    }
    const unsigned half = (unsigned)n >> 1;
    const uint32_t want = (((c[0] + half) >> bits) << 16) | (((c[1] + half) >> bits) << 8) | ((c[2] + half) >> bits);
    const uint32_t got = resolve_round_n(sum, bits);
    ++rounded;
    EXPECT(got == want, "n = %d: resolve_round_n %06x, the integer mean %06x", n, got, want);
}
int st_pairs = 0;
void check_arithmetic() {
    static uint32_t px[256];
    static const uint32_t fixed[] = {0x000000u, 0xffffffu, 0xff0000u, 0x00ff00u, 0x0000ffu, 0x00ffffu, 0xff00ffu, 0xffff00u};
    for (int s = 0; s <= 3; ++s)
        for (int t = 0; t + 2 * s <= 8; ++t) {
            const int bits = t + 2 * s, n = 1 << bits;
            ++st_pairs;
            // the s = 1 .. 3 form of the kernels: m = 1 is resolve_round
            if (t == 0) {
                ResolveSum one = resolve_unpack(0x123456u), sum{0u, 0u};
                for (int i = 0; i < n; ++i) sum = resolve_add(sum, one);
                EXPECT(resolve_round(sum, s) == resolve_round_n(sum, bits), "m = 1 is rt_set_supersampling's formula");
            }
            for (uint32_t f : fixed) {  // every channel at 0 / 255, one at 255 among zeros, one at 0 among 255s
                for (int i = 0; i < n; ++i) px[i] = f;
                check_one(px, n, bits);
                // (and half the samples: the rounding term decides)
                for (int i = 0; i < n; ++i) px[i] = i < n / 2 ? f : 0u;
                check_one(px, n, bits);
                for (int i = 0; i < n; ++i) px[i] = i < n / 2 - 1 || n == 1 ? f : f ^ 0xffffffu;
                check_one(px, n, bits);
            }
            for (int rep = 0; rep < 100000; ++rep) {
                // (every second set from a narrow range around a random level, so that sums sit near rounding boundaries)
                const uint64_t base = next64();
                for (int i = 0; i < n; i += 2) {
                    const uint64_t z = next64();
                    uint32_t a = (uint32_t)z & 0xffffffu, b = (uint32_t)(z >> 32) & 0xffffffu;
                    if (rep & 1) {
                        a = ((uint32_t)base & 0xfefefeu) | (a & 0x010101u);
                        b = ((uint32_t)base & 0xfefefeu) | (b & 0x010101u);
                    }
                    px[i] = a;
                    if (i + 1 < n) px[i + 1] = b;
                }
                check_one(px, n, bits);
            }
        }
}

// ---- 3. the butterfly ----------------------------------------------------------------------------------------------
int blocks_checked = 0;
void check_butterfly() {
    for (int s = 1; s <= 3; ++s) {
        // resolve_block_sum's steps as lane xors: 1 and 8 (k >= 2), 2 and 16 (k >= 4), 4 and 32 (k = 8)
        static const int steps[3][2] = {{1, 8}, {2, 16}, {4, 32}};
        uint64_t v[64], w[64];
        for (int l = 0; l < 64; ++l) v[l] = 1ull << l;  // (a lane's value: its own bit -- a sum of distinct lanes is their mask)
        for (int level = 0; level < s; ++level)
            for (int x : steps[level]) {
                for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ x];
                std::memcpy(v, w, sizeof v);
            }
        const int k = 1 << s;
        for (int l = 0; l < 64; ++l) {
            const int rx = l & 7, ry = l >> 3, bx = rx & ~(k - 1), by = ry & ~(k - 1);
            uint64_t block = 0;
            for (int j = 0; j < k; ++j)
                for (int i = 0; i < k; ++i) block |= 1ull << ((by + j) * 8 + bx + i);
            EXPECT(v[l] == block, "k = %d lane %d holds %016llx, its block is %016llx", k, l, (unsigned long long)v[l],
                   (unsigned long long)block);
            if (rx == bx && ry == by) ++blocks_checked;  // the leader: (x | r) & (k - 1) == 0
        }
    }
}
}  // namespace

int main() {
    check_variants();
    check_arithmetic();
    check_butterfly();
    std::printf("path_ss_host: %lld variant cases with the field zero, %lld with it set (refused: %lld tiles, %lld stats, %lld ordered, "
                "%lld copy slice, %lld factor above 3, %lld without views, %lld sums too wide, %lld another value), %zu descriptors "
                "with the field zero, %zu in all (%zu PATH_SS, %zu SHUTTER_SS, %zu ANIM_SS), %d built\n",
                zero_cases, set_cases, ref_tiles, ref_stats, ref_ordered, ref_copy, ref_ss, ref_no_views, ref_sum, ref_value, n_zero,
                n_all, n_new[0], n_new[1], n_new[2], n_built);
    std::printf("path_ss_host: %lld sample sets over %d (s, t) pairs round to the integer mean\n", rounded, st_pairs);
    std::printf("path_ss_host: %d block leaders hold exactly their block's sum\n", blocks_checked);
    std::printf("path_ss_host: %ld failures\n", failures);
    return failures == 0 ? 0 : 1;
}
