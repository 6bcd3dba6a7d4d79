// variant_host.cpp -- host check of the trace kernels' variant selection (rt_internal.h pick_trace_variant), TEST
// INFRASTRUCTURE ONLY.  Built by the Makefile beside it under ASan + UBSan and run as a plain executable on the CPU
// (tests/test_variant_host.py); needs rt_internal.h alone, no device call exists here.
//
// Every combination of the launch parameters the selection reads is enumerated, and each result compared with
// `expect` below: the selection rules written out as one if-chain over the inputs, with the thresholds as
// literals, sharing nothing with the code under test.  Then the set of descriptors returned is counted: 384, split
// over the entry points as the kernels of the code object are, and equal to the set trace_variant_built admits.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <tuple>

#include "rt_internal.h"

using namespace rtk;

namespace {
using Key = std::tuple<int, int, int, int, int, int, int>;
Key key_of(const TraceVariant& v) { return Key{v.family, v.gpow, v.mode, v.cls, v.K, v.wpg, v.tord}; }

// The rules, restated: false = refused.
bool expect(const LaunchParams& p, bool gpow, bool stats, TraceVariant* v) {
    const bool tiles = p.out_fmt == 3;
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
        mode = 4;  // PATH
    } else if (p.ss_log2 > 0) {
        if (p.ss_log2 > 3) return false;
        if (tiles) return false;
        if (stats) return false;
        if (p.tile_order != nullptr) return false;
        if (p.tile_cost != nullptr) return false;
        mode = 3;  // SS
    } else if (tiles) {
        mode = 2;  // TILES (whatever `stats`)
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

int failures = 0;
void check(bool ok, const char* what) {
    if (!ok && failures++ < 20) std::printf("variant_host: FAILED %s\n", what);
}
}  // namespace

int main() {
    static const int Ss[] = {0, 8, 9, 11, 12, 64, 65}, Ls[] = {0, 1, 4, 5}, limits[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 40};
    static uint32_t cell[2];
    static DevView view;
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.W = 20, p.H = 12, p.local_rows = 12, p.band_rows = 12;
    long long cases = 0, refused = 0, mismatches = 0;
    std::set<Key> seen;
    std::map<unsigned, Key> word_of;  // (family, word) -> the descriptor's fields but K
    for (int S : Ss) for (int L : Ls) for (int a2 = 0; a2 < 2; ++a2) for (int limit : limits)
    for (int gpow = 0; gpow < 2; ++gpow) for (int stats = 0; stats < 2; ++stats) for (int fmt = 0; fmt < 2; ++fmt)
    for (int ss = 0; ss <= 4; ++ss) for (int views = 0; views < 2; ++views) for (int nf = 1; nf <= 2; ++nf)
    for (int cz = 0; cz < 2; ++cz) for (int to = 0; to < 2; ++to) for (int tc = 0; tc < 2; ++tc)
    for (int ro = 0; ro < 2; ++ro) for (int cm = 0; cm < 2; ++cm) {
        p.S = S, p.L = L, p.lights_a2_ok = a2, p.limit = limit;
        p.out_fmt = fmt ? OUT_TILES : 0;
        p.ss_log2 = ss;
        p.views = views ? &view : nullptr;
        p.n_frames = nf, p.copy_z = cz;
        p.tile_order = to ? &cell[0] : nullptr, p.tile_cost = tc ? &cell[1] : nullptr;
        p.row_order_n = ro ? 2 : 0, p.col_major = cm;
        TraceVariant want{-1, -1, -1, -1, -1, -1, -1}, got{-2, -2, -2, -2, -2, -2, -2};
        const bool w = expect(p, gpow != 0, stats != 0, &want), g = pick_trace_variant(p, gpow != 0, stats != 0, &got);
        ++cases;
        if (!w) ++refused;
        if (w != g || (w && key_of(want) != key_of(got))) {
            if (mismatches++ < 10)
                std::printf("variant_host: MISMATCH S %d L %d a2 %d limit %d gpow %d stats %d fmt %d ss %d views %d nf %d "
                            "cz %d to %d tc %d ro %d cm %d: want %d {%d %d %d %d %d %d %d} got %d {%d %d %d %d %d %d %d}\n",
                            S, L, a2, limit, gpow, stats, fmt, ss, views, nf, cz, to, tc, ro, cm, (int)w, want.family,
                            want.gpow, want.mode, want.cls, want.K, want.wpg, want.tord, (int)g, got.family, got.gpow,
                            got.mode, got.cls, got.K, got.wpg, got.tord);
            continue;
        }
        if (!g) continue;
        seen.insert(key_of(got));
        check(trace_variant_built(got), "a descriptor returned is one that is built");
        // the variant word names the descriptor (but K and the family) uniquely, and reads back by name
        const unsigned word = variant_word(got);
        const Key nok{got.family, got.gpow, got.mode, got.cls, 0, got.wpg, got.tord};
        const auto it = word_of.emplace((unsigned)got.family << 31 | word, nok).first;
        check(it->second == nok, "one variant word per descriptor");
        check(vf_cls_of(word) == got.cls && vf_wpg_of(word) == got.wpg && vf_tord_of(word) == got.tord &&
                  ((word & VF_GPOW) != 0) == (got.gpow != 0) && ((word & VF_STATS) != 0) == (got.mode == TM_STATS) &&
                  ((word & VF_TILES) != 0) == (got.mode == TM_TILES) && ((word & VF_SS) != 0) == (got.mode == TM_SS) &&
                  ((word & VF_PATH) != 0) == (got.mode == TM_PATH),
              "the variant word reads back");
    }
    failures += (int)(mismatches > 0x7fffffff ? 0x7fffffff : mismatches);

    // the descriptors by the kernels they name: per family {no GPOW, GPOW} x {PLAIN / STATS / TILES, SS, PATH}
    int count[2][2][3] = {};
    for (const Key& k : seen) count[std::get<0>(k)][std::get<1>(k)][std::get<2>(k) == TM_SS ? 1 : std::get<2>(k) == TM_PATH ? 2 : 0]++;
    static const int want_count[2][2][3] = {{{72, 12, 12}, {72, 12, 12}}, {{66, 18, 18}, {54, 18, 18}}};
    check(std::memcmp(count, want_count, sizeof count) == 0, "per-kernel-name counts 72/72/12/12/12/12 and 66/54/18/18/18/18");
    check(seen.size() == 384, "384 distinct descriptors");

    // trace_variant_built admits exactly these, over every value a field takes
    static const int Ks[] = {1, 2, 4, 6, 8, 64}, clss[] = {0, 1, 2, DIRECT_SMAX}, wpgs[] = {1, SINGLE_WPG};
    int built = 0;
    for (int f = 0; f < 2; ++f) for (int gp = 0; gp < 2; ++gp) for (int m = 0; m < 5; ++m) for (int c : clss)
    for (int K : Ks) for (int w : wpgs) for (int t = 0; t < 3; ++t) {
        const TraceVariant v{f, gp, m, c, K, w, t};
        if (!trace_variant_built(v)) continue;
        ++built;
        check(seen.count(key_of(v)) == 1, "a built descriptor is one the selection returns");
    }
    check(built == 384, "384 built descriptors");

    // the merged-class helper on its own (the host's shadow grids and its lone bundle frames use it)
    check(merged_class(11, 2, true) == 0 && merged_class(12, 0, true) == 0 && merged_class(12, 5, true) == 0 &&
              merged_class(65, 1, true) == 0 && merged_class(12, 1, false) == 1 && merged_class(64, 4, false) == 1 &&
              merged_class(12, 1, true) == 2 && merged_class(64, 4, true) == 2,
          "merged_class");

    std::printf("variant_host: %lld cases, %lld refused, %zu descriptors, %d built\n", cases, refused, seen.size(), built);
    std::printf("variant_host: direct %d %d %d / %d %d %d, bundle %d %d %d / %d %d %d\n", count[0][0][0], count[0][0][1],
                count[0][0][2], count[0][1][0], count[0][1][1], count[0][1][2], count[1][0][0], count[1][0][1],
                count[1][0][2], count[1][1][0], count[1][1][1], count[1][1][2]);
    std::printf("variant_host: %d failures\n", failures);
    return failures == 0 ? 0 : 1;
}
