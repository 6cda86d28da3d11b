// lookback_rule_host.cpp -- the window rule of deltarice_amd/csrc/drx_lookback.h (lookback_window, lookback_counts) on the host,
// against a scalar model that walks the 128 entries of a window from the nearest one: state 0 is a hole, state 2 (a prefix) ends
// the walk, state 1 (an aggregate) counts.  For every window: fp, hole and the set of lanes that count.
// (tests/test_lookback_rule_host.py compiles this host-side, plainly and with sanitizers, and asserts the last line.)
#include <stdint.h>
#include <stdio.h>

#include "drx_lookback.h"

using namespace drx;

static long windows = 0, mismatches = 0;

static void check(const uint8_t (&s)[kLookbackWin]) {
    // the model
    int fp = kLookbackWin;
    bool hole = false;
    bool counts[kLookbackWin];
    for (int d = 0; d < kLookbackWin; ++d) counts[d] = false;
    for (int d = 0; d < kLookbackWin; ++d) {
        counts[d] = true;
        if (s[d] == 2) { fp = d; break; }
        if (s[d] == 0) hole = true;
    }
    // the rule, from the ballots a wavefront takes
    uint64_t p[2] = {0, 0}, z[2] = {0, 0};
    for (int j = 0; j < 2; ++j)
        for (int lane = 0; lane < 64; ++lane) {
            if (s[64 * j + lane] == 2) p[j] |= 1ull << lane;
            if (s[64 * j + lane] == 0) z[j] |= 1ull << lane;
        }
    const LookbackWindow w = lookback_window(p[0], z[0], p[1], z[1]);
    bool ok = w.fp == fp && w.hole == hole;
    for (int j = 0; j < 2; ++j)
        for (int lane = 0; lane < 64; ++lane) ok = ok && lookback_counts(w.fp, j, lane) == counts[64 * j + lane];
    ++windows;
    if (!ok) {
        if (mismatches < 10) printf("mismatch: model fp %d hole %d, rule fp %d hole %d\n", fp, (int)hole, w.fp, (int)w.hole);
        ++mismatches;
    }
}

int main() {
    static_assert(kLookbackWin == 128, "two groups of 64");
    uint8_t s[kLookbackWin];
    // a prefix at f and a single hole at h, aggregates everywhere else; 128 = none (f = 128: the windows without a prefix,
    // with a hole and without one; h == f: the hole takes the prefix's place)
    for (int f = 0; f <= kLookbackWin; ++f)
        for (int h = 0; h <= kLookbackWin; ++h) {
            for (int d = 0; d < kLookbackWin; ++d) s[d] = 1;
            if (f < kLookbackWin) s[f] = 2;
            if (h < kLookbackWin) s[h] = 0;
            check(s);
        }
    // windows drawn by a fixed LCG over {0, 1, 2}; every fourth round mostly aggregates, so that far prefixes occur too
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto next = [&x]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); };
    for (int n = 0; n < 200000; ++n) {
        const uint32_t rare = (n & 3) == 3 ? 64u : 1u;
        for (int d = 0; d < kLookbackWin; ++d) {
            const uint32_t r = next();
            s[d] = rare == 1u ? (uint8_t)(r % 3u) : (uint8_t)((r % (3u * rare)) == 0u ? 0u : ((r % (3u * rare)) == 1u ? 2u : 1u));
        }
        check(s);
    }
    printf("%ld windows, %ld mismatches\n", windows, mismatches);
    return mismatches ? 1 : 0;
}
