// sel_survey_host.cpp -- deltarice_amd/csrc/drx_sel_survey.h on the host, against a plain loop (tests/test_sel_survey_host.py
// compiles this with the host compiler and -fsanitize=address,undefined and runs it).
//
// sel_survey(): every entry's chunk and length against a linear search of the chunk table, the touched chunks against a
// std::set, the walk's three lists against a stable partition of that set.  GatherChunks: the output chunks' sample counts and
// the refusals against a loop over each output chunk's entries.  Small uniform and ragged plans whose lists are written out,
// larger ones for the two ways the touched chunks are collected (n_sel above n_chunks / 8: a flag per chunk; else sort + unique),
// a uniform plan of more than 2^32 waveforms (arithmetic only), and some thousands of random lists.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "drx_sel_survey.h"

using namespace drx;

static std::mt19937_64 rng(20240917u);
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1u); }  // inclusive

static int failures = 0, cases = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (failures < 20) {                            \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                        \
                printf("\n");                               \
            }                                               \
            ++failures;                                     \
        }                                                   \
    } while (0)

struct Chunk { uint64_t wave_base; uint32_t n_samples, wave_len, n_waves; };  // what the survey reads of a chunk table's entry

struct Plan {
    const char *name;
    SelGeom G;
    std::vector<Chunk> chunks;  // ragged plans
    Chunk at(uint64_t c) const { return G.uniform ? Chunk{c * G.u_n_waves, G.u_n_samples, G.u_wave_len, G.u_n_waves} : chunks[c]; }
};
static Plan uniform_plan(const char *name, uint64_t n_chunks, uint32_t N, uint32_t L) {
    const uint32_t W = (N + L - 1) / L;
    return Plan{name, SelGeom{true, n_chunks, n_chunks * W, N, L, W}, {}};
}
static Plan ragged_plan(const char *name, const std::vector<std::pair<uint32_t, uint32_t>> &NL) {
    Plan P{name, SelGeom{false, NL.size(), 0, NL[0].first, NL[0].second, 0}, {}};
    for (const auto &nl : NL) {
        const uint32_t W = (uint32_t)(((uint64_t)nl.first + nl.second - 1) / nl.second);
        P.chunks.push_back(Chunk{P.G.total_waves, nl.first, nl.second, W});
        P.G.total_waves += W;
    }
    return P;
}

// a walk class of the test's own: three classes that the small plans' chunks all occur in
static int walk_class(uint32_t n_waves, uint32_t wave_len) { return wave_len <= 3 ? 0 : (n_waves >= 3 ? 1 : 2); }

struct Seen { uint64_t i, c; uint32_t len; };

// ---- the plain loop: entry -> (chunk, length) by a linear search
static bool plain_entry(const Plan &P, uint64_t g, uint64_t *c_out, uint32_t *len) {
    if (g >= P.G.total_waves) return false;
    uint64_t c = 0;
    if (P.G.uniform) c = g / P.G.u_n_waves;  // (a linear search of 2^31 equal chunks is this division)
    else while (c + 1 < P.G.n_chunks && P.chunks[c + 1].wave_base <= g) ++c;
    const Chunk d = P.at(c);
    const uint64_t idx = g - d.wave_base;
    *len = idx + 1 == d.n_waves ? d.n_samples - (uint32_t)(idx * d.wave_len) : d.wave_len;
    *c_out = c;
    return true;
}

static void survey_case(const Plan &P, const std::vector<uint64_t> &sel, bool sideband) {
    ++cases;
    std::vector<uint32_t> lists{7u, 7u};  // (what it held before must not show)
    uint32_t n_class[3] = {9, 9, 9};
    uint64_t at = ~0ull;
    std::vector<Seen> seen;
    const int r = sel_survey(P.G, P.chunks.data(), sel.data(), sel.size(), sideband, walk_class, lists, n_class, &at,
                             [&](uint64_t i, uint64_t c, uint32_t len) { seen.push_back(Seen{i, c, len}); return 0; });
    std::set<uint32_t> touched;
    for (uint64_t i = 0; i < sel.size(); ++i) {
        uint64_t c;
        uint32_t len;
        if (!plain_entry(P, sel[i], &c, &len)) {
            CHECK(r == kSelBadIndex && at == i, "%s: entry %llu is no waveform: survey said %d at %llu", P.name, (unsigned long long)i, r, (unsigned long long)at);
            CHECK(seen.size() == i, "%s: %zu entries handed on in front of the refused entry %llu", P.name, seen.size(), (unsigned long long)i);
            return;
        }
        touched.insert((uint32_t)c);
        CHECK(i < seen.size() && seen[i].i == i && seen[i].c == c && seen[i].len == len, "%s: entry %llu = waveform %llu: chunk %llu length %u expected",
              P.name, (unsigned long long)i, (unsigned long long)sel[i], (unsigned long long)c, len);
    }
    CHECK(r == 0 && seen.size() == sel.size(), "%s: survey said %d, %zu of %zu entries handed on", P.name, r, seen.size(), sel.size());
    std::vector<uint32_t> want(touched.begin(), touched.end());
    uint32_t want_class[3] = {0, 0, 0};
    if (!sideband) {
        auto cls = [&](uint32_t c) { const Chunk d = P.at(c); return walk_class(d.n_waves, d.wave_len); };
        for (uint32_t c : want) ++want_class[cls(c)];
        auto mid = std::stable_partition(want.begin(), want.end(), [&](uint32_t c) { return cls(c) == 0; });
        std::stable_partition(mid, want.end(), [&](uint32_t c) { return cls(c) == 1; });
    }
    CHECK(lists == want, "%s: %zu entries, side-band %d: the chunk lists differ (%zu chunks, %zu expected)", P.name, sel.size(), (int)sideband, lists.size(),
          want.size());
    CHECK(n_class[0] == want_class[0] && n_class[1] == want_class[1] && n_class[2] == want_class[2], "%s: classes %u %u %u, expected %u %u %u", P.name,
          n_class[0], n_class[1], n_class[2], want_class[0], want_class[1], want_class[2]);
}

// ---- the gather's output chunks: a loop over each chunk's entries
static void gather_case(const Plan &P, const std::vector<uint64_t> &sel, uint64_t cw, int expect = -1, uint64_t expect_entry = 0) {
    ++cases;
    const uint64_t n_sel = sel.size(), n_out = (n_sel + cw - 1) / cw;
    std::vector<uint32_t> len(n_sel), want_n(n_out, 0);
    for (uint64_t i = 0; i < n_sel; ++i) {
        uint64_t c;
        if (!plain_entry(P, sel[i], &c, &len[i])) { printf("FAIL: gather_case wants lists of waveforms of the batch\n"); ++failures; return; }
    }
    int want = GatherChunks::kOk;
    uint64_t want_entry = 0, want_oc = 0;
    for (uint64_t oc = 0; oc < n_out && !want; ++oc) {
        const uint64_t b = oc * cw, e = std::min(n_sel, b + cw);
        uint64_t sum = 0;
        for (uint64_t j = b; j < e && !want; ++j) {
            want_entry = j; want_oc = oc;
            if (j > b && len[j - 1] < len[b]) { want = GatherChunks::kShorterNotLast; want_entry = j - 1; }
            else if (len[j] > len[b]) want = GatherChunks::kLonger;
            else if ((sum += len[j]) >= (1ull << 31)) want = GatherChunks::kTooLong;
            else want_n[oc] = (uint32_t)sum;
        }
    }
    std::vector<uint32_t> chunk_n(n_out, 0), lists;
    GatherChunks rule{cw, chunk_n.data()};
    uint32_t n_class[3];
    uint64_t at = 0;
    const int r = sel_survey(P.G, P.chunks.data(), sel.data(), n_sel, false, walk_class, lists, n_class, &at,
                             [&](uint64_t i, uint64_t, uint32_t l) { return (int)rule.add(i, l); });
    CHECK(r == want, "%s: gather of %llu entries by %llu: %d, expected %d", P.name, (unsigned long long)n_sel, (unsigned long long)cw, r, want);
    if (expect >= 0) CHECK(r == expect && (!r || rule.entry == expect_entry), "%s: gather by %llu: %d at entry %llu, the case expects %d at %llu", P.name,
                           (unsigned long long)cw, r, (unsigned long long)rule.entry, expect, (unsigned long long)expect_entry);
    if (want) {
        CHECK(rule.entry == want_entry && rule.oc == want_oc && rule.first == len[want_oc * cw], "%s: refusal %d names entry %llu of chunk %llu (first %u), expected %llu of %llu (%u)",
              P.name, r, (unsigned long long)rule.entry, (unsigned long long)rule.oc, rule.first, (unsigned long long)want_entry, (unsigned long long)want_oc, len[want_oc * cw]);
        return;
    }
    CHECK(chunk_n == want_n, "%s: gather of %llu entries by %llu: the output chunks' sample counts differ", P.name, (unsigned long long)n_sel, (unsigned long long)cw);
}

static std::vector<uint64_t> random_list(const Plan &P, uint64_t n) {
    std::vector<uint64_t> s(n);
    const uint64_t span = rnd(0, 3) ? P.G.total_waves : std::min<uint64_t>(P.G.total_waves, rnd(1, 12));  // (a narrow span: duplicates, few chunks)
    for (uint64_t &g : s) g = rnd(0, span - 1);
    if (rnd(0, 3) == 0) std::sort(s.begin(), s.end());
    return s;
}

int main() {
    // 3 chunks of 10 samples at WaveformLength 4: waveforms of 4, 4 and 2 samples
    const Plan U = uniform_plan("uniform 3x10/4", 3, 10, 4);
    // mixed WaveformLengths; chunk 1 is one waveform (the whole chunk), chunk 3 one waveform shorter than its WaveformLength
    const Plan R = ragged_plan("ragged 5", {{10, 4}, {7, 7}, {12, 3}, {3, 8}, {9, 2}});
    // enough chunks for n_chunks / 8 to be a size: 8 entries are sorted, 9 flagged
    const Plan U64 = uniform_plan("uniform 64x9/2", 64, 9, 2);
    std::vector<std::pair<uint32_t, uint32_t>> nl;
    for (uint32_t c = 0; c < 64; ++c) nl.push_back({(uint32_t)rnd(1, 40), (uint32_t)rnd(1, 12)});
    const Plan R64 = ragged_plan("ragged 64", nl);
    for (const Plan *P : {&U, &R, &U64, &R64}) {
        const uint64_t W = P->G.total_waves, edge = P->G.n_chunks / 8u;
        for (int sideband = 0; sideband < 2; ++sideband) {
            survey_case(*P, {0}, sideband);
            survey_case(*P, {W - 1}, sideband);                // the batch's last waveform
            survey_case(*P, {2, 2, 2, W - 1, 2}, sideband);    // duplicates
            std::vector<uint64_t> down;
            for (uint64_t g = W; g-- > 0;) down.push_back(g);  // descending, every waveform
            survey_case(*P, down, sideband);
            survey_case(*P, {1, W, 0}, sideband);              // entry 1 is refused
            survey_case(*P, {W + 5}, sideband);
            for (uint64_t n : {edge - 1, edge, edge + 1, edge + 2})  // around the switch from sorting to flags (0 entries where edge is 0)
                if (n <= W && n + 1 != 0) {
                    survey_case(*P, random_list(*P, n), sideband);
                    std::vector<uint64_t> spread(n);
                    for (uint64_t i = 0; i < n; ++i) spread[i] = P->at((n - 1 - i) * (P->G.n_chunks / (n ? n : 1))).wave_base;  // n chunks, descending
                    survey_case(*P, spread, sideband);
                }
            for (int t = 0; t < 1000; ++t) survey_case(*P, random_list(*P, rnd(1, 3 * P->G.n_chunks)), sideband);
        }
        for (int t = 0; t < 500; ++t) {
            std::vector<uint64_t> s = random_list(*P, rnd(1, 24));
            gather_case(*P, s, rnd(1, s.size() + 1));
        }
    }
    // ---- the gather's rule on lists written out (U: waveforms 0 1 2 | 3 4 5 | 6 7 8 of 4 4 2 samples)
    for (uint64_t cw : {1ull, 2ull, 4ull}) gather_case(U, {0, 1, 3, 4}, cw, GatherChunks::kOk);  // chunk_waves 1, 2 and n_sel
    gather_case(U, {0, 1, 2, 3, 4, 5}, 3, GatherChunks::kOk);                      // a shorter entry that is its chunk's last
    gather_case(U, {0, 2}, 5, GatherChunks::kOk);                                  // ... and the list's
    gather_case(U, {0, 2, 1, 3}, 3, GatherChunks::kShorterNotLast, 1);             // not its chunk's last: entry 1, named at entry 2
    gather_case(U, {0, 2, 2}, 3, GatherChunks::kShorterNotLast, 1);
    gather_case(U, {2, 5, 0}, 3, GatherChunks::kLonger, 2);                        // a longer entry
    gather_case(U, {0, 1, 2, 0}, 2, GatherChunks::kLonger, 3);                     // ... in the second output chunk
    gather_case(R, {3, 4, 8, 9, 10, 11, 12, 13}, 2, GatherChunks::kOk);            // chunks 1 (7) 2 (3 3) 3 (3) 4 (2 2 2 ...)
    gather_case(R, {8, 3}, 2, GatherChunks::kLonger, 1);
    // an output chunk of two entries of 2^30 samples: a chunk table of such lengths with no data behind it
    const Plan big = ragged_plan("ragged 2^30", {{1u << 30, 1u << 30}, {1u << 30, 1u << 30}, {(1u << 30) - 1u, 1u << 30}});
    gather_case(big, {0, 1}, 2, GatherChunks::kTooLong, 1);
    gather_case(big, {0, 1}, 1, GatherChunks::kOk);
    gather_case(big, {0, 2}, 2, GatherChunks::kOk);  // 2^31 - 1 samples
    gather_case(big, {2, 2, 0, 1}, 2, GatherChunks::kTooLong, 3);
    // ---- more than 2^32 waveforms: the 64-bit side of the division (2^31 chunks of 3 waveforms; sorted, no flag per chunk)
    const Plan huge = uniform_plan("uniform 2^31 x 10/4", 1ull << 31, 10, 4);
    const uint64_t HW = huge.G.total_waves;
    for (int sideband = 0; sideband < 2; ++sideband) {
        survey_case(huge, {(1ull << 32) + 5, 4, (1ull << 32) + 5, HW - 1, (1ull << 32) - 1, 1ull << 32}, sideband);
        survey_case(huge, {HW - 1, HW}, sideband);
        for (int t = 0; t < 200; ++t) {
            std::vector<uint64_t> s(rnd(1, 40));
            for (uint64_t &g : s) g = rnd(0, 1) ? rnd((1ull << 32) - 8, (1ull << 32) + 8) : rnd(0, HW - 1);
            survey_case(huge, s, sideband);
        }
    }
    printf("%d cases; %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
