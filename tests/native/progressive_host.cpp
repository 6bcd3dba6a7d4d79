// progressive_host.cpp -- host checks of progressive accumulation (rt_set_progressive), TEST INFRASTRUCTURE ONLY.
// Plain host C++ against the device-free headers of csrc (rt_resolve.h, rt_progressive.h, rt_internal.h), built by
// progressive.mk beside it with ASan + UBSan and run as a plain executable (tests/test_progressive_host.py).
//
//  1. resolve_round_div (rt_resolve.h, the function the PROG kernels round with) against plain per-channel integer
//     division: every c in 1..64, every field sum 0..255 c, the three fields filled at once with different sums; and
//     against resolve_round_n at c = 1, 2, 4, .., 64.
//  2. The sample order (rt_progressive.h prog_sample / prog_pass) against a table for k = 4 and as a permutation whose
//     first 4^t samples are the stride-k/2^t sub-grid, k = 1, 2, 4, 8.
//  3. The per-Tick plan (prog_plan) over scripted sequences: a resting run to convergence and beyond, key changes of
//     every field, a reset, a change of k, a change of the worker layout, k = 1.
//  4. The variant selection (rt_internal.h pick_trace_variant): adaptive_host's enumeration with the new fields at
//     zero against the rules as they were, restated below; then with the fields set, where a launch that selected SS
//     selects PROG and mirrors the ADAPT descriptor field for field; 564 descriptors, 60 of them new, 564 built.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "rt_internal.h"
#include "rt_progressive.h"
#include "rt_resolve.h"

using namespace rtk;

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

// ---- 1. the rounding ----------------------------------------------------------------------------------------------
long round_cases = 0, round_n_cases = 0;
void check_round_div() {
    for (int c = 1; c <= 64; ++c) {
        const uint32_t top = 255u * (uint32_t)c;
        for (uint32_t n = 0; n <= top; ++n) {
            // three different sums at once: nothing of one field reaches another
            const uint32_t r = n, g = (n * 7u + 3u) % (top + 1u), b = top - n;
            const ResolveSum sum{r << 16 | b, g};
            const uint32_t want = ((r + (uint32_t)c / 2u) / (uint32_t)c) << 16 | ((g + (uint32_t)c / 2u) / (uint32_t)c) << 8 |
                                  ((b + (uint32_t)c / 2u) / (uint32_t)c);
            const uint32_t got = resolve_round_div(sum, c);
            EXPECT(got == want, "resolve_round_div c %d sums %u %u %u: %06x, want %06x", c, r, g, b, got, want);
            ++round_cases;
            if ((c & (c - 1)) == 0) {
                int t = 0;
                while ((1 << t) < c) ++t;
                EXPECT(got == resolve_round_n(sum, t), "resolve_round_div c %d against resolve_round_n t %d, sums %u %u %u", c, t, r, g, b);
                ++round_n_cases;
            }
        }
    }
    // sums of real samples: c pixels through resolve_unpack / resolve_add
    const uint32_t px[3] = {0x00ff00u, 0xff00ffu, 0x010203u};
    ResolveSum s{0u, 0u};
    for (uint32_t p : px) s = resolve_add(s, resolve_unpack(p));
    EXPECT(resolve_round_div(s, 3) == (((0xffu + 0x01u + 1u) / 3u) << 16 | ((0xffu + 0x02u + 1u) / 3u) << 8 | ((0xffu + 0x03u + 1u) / 3u)),
           "three unpacked pixels");
    EXPECT(resolve_round_div(resolve_unpack(0x00abcdefu), 1) == 0x00abcdefu, "c = 1 is the pixel itself");
}

// ---- 2. the order -------------------------------------------------------------------------------------------------
long order_cases = 0;
void check_order() {
    static const int k4[16][2] = {{0, 0}, {2, 0}, {0, 2}, {2, 2}, {1, 0}, {3, 0}, {1, 2}, {3, 2},
                                  {0, 1}, {2, 1}, {0, 3}, {2, 3}, {1, 1}, {3, 1}, {1, 3}, {3, 3}};
    for (int n = 0; n < 16; ++n) {
        int i = -1, j = -1;
        prog_sample(2, n, &i, &j);
        EXPECT(i == k4[n][0] && j == k4[n][1], "k = 4 sample %d: (%d, %d), want (%d, %d)", n, i, j, k4[n][0], k4[n][1]);
        EXPECT(prog_pass(2, n) == k4[n][1] * 4 + k4[n][0], "k = 4 pass code of sample %d", n);
        ++order_cases;
    }
    static const int k2[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
    for (int n = 0; n < 4; ++n) {
        int i = -1, j = -1;
        prog_sample(1, n, &i, &j);
        EXPECT(i == k2[n][0] && j == k2[n][1], "k = 2 sample %d", n);
        ++order_cases;
    }
    for (int s = 0; s <= 3; ++s) {
        const int k = 1 << s;
        std::set<int> seen;
        for (int n = 0; n < k * k; ++n) {
            int i = -1, j = -1;
            prog_sample(s, n, &i, &j);
            EXPECT(i >= 0 && i < k && j >= 0 && j < k, "k = %d sample %d inside the block", k, n);
            EXPECT(prog_pass(s, n) == j * k + i, "k = %d pass code of sample %d", k, n);
            seen.insert(j * k + i);
            // the first 4^t samples are the sub-grid of stride k >> t
            for (int t = 0; t <= s; ++t)
                if (n < 1 << (2 * t)) EXPECT(i % (k >> t) == 0 && j % (k >> t) == 0, "k = %d sample %d on the stride-%d grid", k, n, k >> t);
            ++order_cases;
        }
        EXPECT((int)seen.size() == k * k, "k = %d: a permutation of the block", k);
        EXPECT(prog_log2(k) == s, "prog_log2(%d)", k);
    }
    for (int bad : {0, 3, 5, 6, 7, 9, 16, -1, -2, INT_MIN, INT_MAX}) EXPECT(prog_log2(bad) == -1, "prog_log2(%d) is refused", bad);
}

// ---- 3. the plan --------------------------------------------------------------------------------------------------
long plan_ticks = 0;
rt_camera cam(float x, float y, float z, float yaw, float pitch) {
    rt_camera c;
    c.position = rt_vec3{x, y, z}, c.yaw = yaw, c.pitch = pitch;
    return c;
}
void tick(ProgRun* run, const ProgKey& key, int kind, int first, int samples, int divisor, const char* what) {
    const ProgPlan p = prog_plan(run, key);
    EXPECT(p.kind == kind && p.first == first && p.samples == samples && p.divisor == divisor,
           "%s: plan {%d, %d, %d, %d}, want {%d, %d, %d, %d}", what, p.kind, p.first, p.samples, p.divisor, kind, first, samples, divisor);
    EXPECT(run->count == divisor && prog_key_equal(run->key, key), "%s: the run after the Tick", what);
    ++plan_ticks;
}
// A resting run at factor k from its second Tick to two Ticks past convergence.
void rest(ProgRun* run, const ProgKey& key, const char* what) {
    const int kk = key.k * key.k;
    tick(run, key, PROG_TRACE, 0, 2, 2, what);
    for (int c = 3; c <= kk; ++c) tick(run, key, PROG_TRACE, c - 1, 1, c, what);
    tick(run, key, PROG_EMIT, kk, 0, kk, what);
    tick(run, key, PROG_EMIT, kk, 0, kk, what);
}
void check_plan() {
    const rt_camera c0 = cam(0.0f, 1.0f, -2.0f, 0.25f, -0.5f);
    for (int k : {2, 4, 8}) {
        ProgRun run;
        const ProgKey key = prog_key(3, c0, 50, 30, 0, k, 1);
        tick(&run, key, PROG_PLAIN, 0, 1, 1, "the first Tick");
        rest(&run, key, "a resting run");
        // every field of the key restarts, from any point of a run: converged, and after the second and third Ticks
        const ProgKey others[] = {
            prog_key(4, c0, 50, 30, 0, k, 1),                                   // rt_set_scene
            prog_key(3, cam(0.0f, 1.0f, -2.0f, 0.25f, -0.25f), 50, 30, 0, k, 1),  // pitch
            prog_key(3, cam(0.0f, 1.0f, -2.0f, 0.5f, -0.5f), 50, 30, 0, k, 1),    // yaw
            prog_key(3, cam(0.0f, 1.0f, -1.0f, 0.25f, -0.5f), 50, 30, 0, k, 1),   // position z
            prog_key(3, cam(0.0f, 2.0f, -2.0f, 0.25f, -0.5f), 50, 30, 0, k, 1),   // y
            prog_key(3, cam(-0.0f, 1.0f, -2.0f, 0.25f, -0.5f), 50, 30, 0, k, 1),  // x: -0 against +0, compared as bits
            prog_key(3, c0, 51, 30, 0, k, 1),                                   // width
            prog_key(3, c0, 50, 31, 0, k, 1),                                   // height
            prog_key(3, c0, 50, 30, 40, k, 1),                                  // rt_set_view_height
            prog_key(3, c0, 50, 30, 0, k == 2 ? 4 : 2, 1),                      // rt_set_progressive to another k
            prog_key(3, c0, 50, 30, 0, k, 2),                                   // another worker layout
        };
        ProgKey prev = key;
        int depth = 0;
        for (const ProgKey& o : others) {
            EXPECT(!prog_key_equal(prev, o) && !prog_key_equal(key, o), "a different key");
            tick(&run, o, PROG_PLAIN, 0, 1, 1, "a changed key");
            tick(&run, o, PROG_TRACE, 0, 2, 2, "the Tick after a changed key");
            if (depth++ % 2 && o.k > 2) tick(&run, o, PROG_TRACE, 2, 1, 3, "the third Tick");
            prev = o;
        }
        // back to the first key: a new run, not the old one's count
        tick(&run, key, PROG_PLAIN, 0, 1, 1, "back to an earlier key");
        // the same camera values set again (rt_set_camera with unchanged values): the key is equal, the run goes on
        const ProgKey same = prog_key(3, cam(0.0f, 1.0f, -2.0f, 0.25f, -0.5f), 50, 30, 0, k, 1);
        EXPECT(prog_key_equal(key, same), "equal values make equal keys");
        tick(&run, same, PROG_TRACE, 0, 2, 2, "unchanged camera values");
        // rt_reset_progressive, and a failed Tick: count 0
        run.count = 0;
        tick(&run, key, PROG_PLAIN, 0, 1, 1, "after a reset");
        rest(&run, key, "a resting run after a reset");
        run.count = 0;
        tick(&run, key, PROG_PLAIN, 0, 1, 1, "a reset of a converged run");
    }
    // k = 1: every Tick is the plain launch, whatever the run holds
    ProgRun run;
    const ProgKey off = prog_key(1, c0, 50, 30, 0, 1, 1);
    for (int i = 0; i < 4; ++i) tick(&run, off, PROG_PLAIN, 0, 1, 1, "k = 1");
    // from k = 1 to k = 2 and back
    const ProgKey on = prog_key(1, c0, 50, 30, 0, 2, 1);
    tick(&run, on, PROG_PLAIN, 0, 1, 1, "k = 1 -> 2");
    tick(&run, on, PROG_TRACE, 0, 2, 2, "k = 2, second Tick");
    tick(&run, off, PROG_PLAIN, 0, 1, 1, "k = 2 -> 1");
    tick(&run, on, PROG_PLAIN, 0, 1, 1, "k = 1 -> 2 again");
}

// ---- 4. variant selection -------------------------------------------------------------------------------------------
using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// The selection as it is without the progressive fields (adaptive_host's restatement, thresholds as literals).
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
        mode = p.adapt_thr > 0 ? 6 : 3;  // ADAPT : SS
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
// With an accumulator: one view, supersampling on, no threshold, 1 .. k^2 samples in all and 0 .. 2 traced; then the
// launch that selected SS selects PROG (7).
bool expect_prog(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    if (p.views != nullptr || p.ss_log2 < 1 || p.ss_log2 > 3 || p.adapt_thr != 0) return false;
    if (p.prog_first < 0 || p.prog_n < 0 || p.prog_n > 2) return false;
    const int total = p.prog_first + p.prog_n, kk = p.ss_log2 == 1 ? 4 : p.ss_log2 == 2 ? 16 : 64;
    if (total < 1 || total > kk) return false;
    if (!expect_before(p, gpow, stats, v)) return false;
    v->mode = 7;
    return true;
}

long long zero_cases = 0, set_cases = 0, set_refused = 0;
size_t n_descriptors = 0, n_prog = 0;
int n_built = 0;
void check_variants() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static const int sls[] = {0, 1, 8, 9}, thrs[] = {0, 1, 256};
    static uint32_t cell[2];
    static DevView view;
    static ResolveSum acc[4];
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    long long mismatches = 0;
    std::set<Key> seen;
    // pass 0: the grid adaptive_host.cpp walks, the new fields at zero; pass 1: the same grid with an accumulator, 2
    // samples from 0 (the Tick for P_2)
    for (int pass = 0; pass < 2; ++pass)
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
        p.prog_acc = pass ? acc : nullptr;
        p.prog_first = 0, p.prog_n = pass ? 2 : 0;
        p.prog_pass[0] = 0, p.prog_pass[1] = pass ? 1 : 0;
        TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
        const bool w = pass ? expect_prog(p, gpow != 0, stats != 0, &want) : expect_before(p, gpow != 0, stats != 0, &want);
        const bool g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
        ++(pass ? set_cases : zero_cases);
        if (pass && !w) ++set_refused;
        if (w != g || (w && key_of(want) != key_of(got))) {
            if (mismatches++ < 10)
                std::fprintf(stderr, "progressive_host: MISMATCH pass %d thr %d sl %d S %d L %d a2 %d limit %d gpow %d stats %d fmt %d ss %d "
                             "views %d nf %d cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d %d %d %d}\n",
                             pass, thr, sl, S, L, a2, limit, gpow, stats, fmt, ss, views, nf, cz, to, tc, ro, cm, (int)w, want.family,
                             want.gpow, want.mode, want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow,
                             got.mode, got.cls, got.K, got.wpg, got.tord);
            continue;
        }
        if (!g) continue;
        EXPECT((got.mode == TM_PROG) == (pass == 1), "the PROG mode exactly with an accumulator");
        seen.insert(key_of(got));
        EXPECT(trace_variant_built(got), "a descriptor returned is one that is built");
        const unsigned word = variant_word(got);
        EXPECT(((word & VF_PROG) != 0) == (got.mode == TM_PROG) && ((word & VF_ADAPT) != 0) == (got.mode == TM_ADAPT) &&
                   ((word & VF_SS) != 0) == (got.mode == TM_SS) && vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg &&
                   vf_tord_of(word) == got.tord && ((word & VF_GPOW) != 0) == (got.gpow != 0),
               "the variant word reads back");
        if (pass) {  // the ADAPT twin: the same launch with a threshold in place of the accumulator
            LaunchParams q = p;
            q.prog_acc = nullptr, q.prog_first = q.prog_n = 0, q.prog_pass[1] = 0, q.adapt_thr = 16;
            TraceVariant twin{-3, -3, -3, -3, -3, -3, -3};
            EXPECT(pick_trace_variant(q, gpow != 0, stats != 0, &twin) && twin.mode == TM_ADAPT, "the ADAPT twin exists");
            twin.mode = TM_PROG;
            EXPECT(key_of(twin) == key_of(got), "a PROG descriptor mirrors its ADAPT twin field for field");
        }
    }
    failures += (long)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);
    // the sample fields of a PROG launch: every (first, n) at every factor
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12, p.S = 3, p.L = 1, p.limit = 2, p.prog_acc = acc;
    for (int ss = -1; ss <= 4; ++ss)
        for (int first = -1; first <= 66; ++first)
            for (int n = -1; n <= 3; ++n) {
                p.ss_log2 = ss, p.prog_first = first, p.prog_n = n;
                TraceVariant want, got;
                const bool w = expect_prog(p, false, false, &want), g = pick_trace_variant(p, false, false, &got);
                EXPECT(w == g && (!w || (key_of(want) == key_of(got) && got.mode == TM_PROG)), "ss_log2 %d first %d n %d", ss, first, n);
                ++set_cases;
                if (!w) ++set_refused;
            }
    n_descriptors = seen.size();
    EXPECT(seen.size() == 564, "564 distinct descriptors, got %zu", seen.size());
    int per_entry[2][2] = {};
    for (const Key& k : seen)
        if (std::get<2>(k) == TM_PROG) {
            ++n_prog;
            per_entry[std::get<0>(k)][std::get<1>(k)]++;
            EXPECT(std::get<5>(k) == 1 && std::get<6>(k) == 0, "a PROG launch has one tile per workgroup in grid order");
        }
    EXPECT(n_prog == 60, "60 PROG descriptors, got %zu", n_prog);
    EXPECT(per_entry[0][0] == 12 && per_entry[0][1] == 12 && per_entry[1][0] == 18 && per_entry[1][1] == 18,
           "direct 12 + 12 GPOW, bundle 18 + 18 GPOW");
    // trace_variant_built admits exactly these, over every value a field takes
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m < 8; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++n_built;
        EXPECT(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    EXPECT(n_built == 564, "564 built descriptors, got %d", n_built);
    static_assert(sizeof(LaunchParams) < 4096, "the kernarg block");
    static_assert(TM_PROG == 7 && VF_PROG == 128u, "the new mode follows the earlier ones");
}
}  // namespace

int main() {
    check_round_div();
    check_order();
    check_plan();
    check_variants();
    std::printf("progressive_host: %ld rounding cases, %ld against resolve_round_n\n", round_cases, round_n_cases);
    std::printf("progressive_host: %ld order cases, %ld plan ticks\n", order_cases, plan_ticks);
    std::printf("progressive_host: %lld variant cases with the fields at zero, %lld with them set (%lld refused), %zu descriptors "
                "(%zu PROG), %d built\n", zero_cases, set_cases, set_refused, n_descriptors, n_prog, n_built);
    std::printf("progressive_host: %ld failures\n", failures);
    return failures == 0 && round_cases > 0 && order_cases > 0 && plan_ticks > 0 && zero_cases > 0 ? 0 : 1;
}
