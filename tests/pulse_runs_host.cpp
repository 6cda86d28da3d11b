// pulse_runs_host.cpp -- deltarice_amd/csrc/drx_pulse_runs.h on the host, against a plain loop (tests/test_pulse_runs_host.py
// compiles this with the host compiler and -fsanitize=address,undefined and runs it).
//
// Random int16 sequences of 1-300 samples are cut into 1-40 stretches ("blocks"), every block into "lanes" (some of them empty),
// as drx_pulses_blocks.hip does: a summary per lane from its samples, the summaries in front of every lane by folding
// pulse_combine() in a random association order, the second pass that stages the block's own pulses under block-relative
// numbers (the first `cap` of them), the block's summary, and pulse_stitch() over the blocks.  Counts and records must equal the
// loop's; a summary put together from parts must equal the summary of the same samples taken in one go, however it is folded.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "drx_pulse_runs.h"

using namespace drx;

static std::mt19937_64 rng(20240611u);
static uint32_t rnd(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (uint64_t)(hi - lo + 1u)); }  // inclusive

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures < 20) {                          \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
            ++failures;                                   \
        }                                                 \
    } while (0)

static bool same(const PulseSeg &a, const PulseSeg &b) {
    return a.n == b.n && a.inner == b.inner && a.lead_w == b.lead_w && a.trail_w == b.trail_w && a.trail_s == b.trail_s &&
           a.lead_key == b.lead_key && a.lead_sum == b.lead_sum && a.trail_key == b.trail_key && a.trail_sum == b.trail_sum;
}

struct Case {
    std::vector<int16_t> y;
    int64_t t;  // the threshold as the reference defines it: the saturated sum, not clamped
    int32_t tv;
    bool neg;
    uint32_t min_width, max_pulses, cap;
};

// the stretch [lo, hi) in one go
static PulseSeg summarise(const Case &c, uint32_t lo, uint32_t hi) {
    PulseSeg S = pulse_seg_empty();
    for (uint32_t i = lo; i < hi; ++i) pulse_seg_step(S, (int32_t)(c.y[i] ^ (c.neg ? -1 : 0)), c.tv, i, c.min_width);
    pulse_seg_finish(S);
    return S;
}

// parts[lo, hi) folded in a random association order
static PulseSeg fold(const std::vector<PulseSeg> &parts, size_t lo, size_t hi, uint32_t mw) {
    if (lo == hi) return pulse_seg_empty();
    if (hi - lo == 1) return parts[lo];
    const size_t mid = lo + 1 + (size_t)(rng() % (uint64_t)(hi - lo - 1));
    return pulse_combine(fold(parts, lo, mid, mw), fold(parts, mid, hi, mw), mw);
}

static std::vector<uint32_t> cuts(uint32_t lo, uint32_t hi, uint32_t pieces, bool allow_empty) {
    std::vector<uint32_t> c{lo};
    for (uint32_t i = 1; i < pieces; ++i) c.push_back(rnd(lo, hi));
    c.push_back(hi);
    std::sort(c.begin() + 1, c.end() - 1);
    if (!allow_empty) c.erase(std::unique(c.begin(), c.end()), c.end());
    if (c.size() < 2) c.push_back(hi);
    return c;
}

static void run_case(const Case &c, int id) {
    const uint32_t L = (uint32_t)c.y.size();
    // ---- the plain loop
    std::vector<int64_t> want((size_t)c.max_pulses * 5, 0);
    uint32_t want_count = 0;
    for (uint32_t i = 0; i < L;) {
        auto over = [&](uint32_t j) { return c.neg ? (int64_t)c.y[j] < c.t : (int64_t)c.y[j] > c.t; };
        if (!over(i)) { ++i; continue; }
        const uint32_t s = i;
        int64_t pk = c.y[i], sum = 0;
        uint32_t apk = i;
        for (; i < L && over(i); ++i) {
            if (c.neg ? c.y[i] < pk : c.y[i] > pk) { pk = c.y[i]; apk = i; }
            sum += c.y[i];
        }
        if (i - s >= c.min_width) {
            if (want_count < c.max_pulses) {
                int64_t *r = &want[(size_t)want_count * 5];
                r[0] = s; r[1] = i - s; r[2] = pk; r[3] = apk; r[4] = sum;
            }
            ++want_count;
        }
    }
    // ---- blocks of lanes
    const std::vector<uint32_t> bc = cuts(0, L, rnd(1, 40), false);
    const uint32_t nb = (uint32_t)bc.size() - 1;
    std::vector<PulseSeg> table(nb);
    std::vector<int64_t> staging((size_t)nb * (c.cap ? c.cap : 1) * 5, -7);  // (what is not staged is never read: -7 would show)
    std::vector<uint32_t> staged(nb, 0);
    std::vector<std::vector<int64_t>> full(nb);  // every pulse a block emits, staged or not: what the block writes when it is run again
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t b0 = bc[b], b1 = bc[b + 1];
        const std::vector<uint32_t> lc = cuts(b0, b1, rnd(1, 12), true);
        const size_t nl = lc.size() - 1;
        std::vector<PulseSeg> lanes(nl);
        for (size_t l = 0; l < nl; ++l) lanes[l] = summarise(c, lc[l], lc[l + 1]);
        for (size_t l = 0; l < nl; ++l) {
            const PulseSeg P = fold(lanes, 0, l, c.min_width);
            CHECK(same(P, summarise(c, b0, lc[l])), "case %d block %u lane %zu: the folded prefix differs from the summary in one go", id, b, l);
            PulseEmit E = pulse_emit_seed(P);
            for (uint32_t i = lc[l]; i < lc[l + 1]; ++i)
                pulse_emit_step(E, (int32_t)(c.y[i] ^ (c.neg ? -1 : 0)), c.tv, i, b0, c.min_width,
                                [&](uint32_t r, uint32_t s, uint32_t w, int64_t key, int64_t sum) {
                                    CHECK(r == staged[b], "case %d block %u: pulse number %u, expected %u", id, b, r, staged[b]);
                                    ++staged[b];
                                    if (r < c.cap) pulse_record(&staging[((size_t)b * c.cap + r) * 5], s, w, key, sum, c.neg);
                                    full[b].resize(full[b].size() + 5);
                                    pulse_record(&full[b][(size_t)r * 5], s, w, key, sum, c.neg);
                                });
        }
        table[b] = fold(lanes, 0, nl, c.min_width);
        CHECK(same(table[b], summarise(c, b0, b1)), "case %d block %u: the folded summary differs from the summary in one go", id, b);
        CHECK(staged[b] == table[b].inner, "case %d block %u: %u pulses emitted, summary counts %u", id, b, staged[b], table[b].inner);
    }
    CHECK(same(fold(table, 0, nb, c.min_width), summarise(c, 0, L)), "case %d: the blocks folded differ from the waveform in one go", id);
    // ---- the stitch
    std::vector<int64_t> got((size_t)c.max_pulses * 5, 0);
    std::vector<char> written(c.max_pulses, 0);
    uint32_t got_count = 0xffffffffu;
    bool expect_complete = true;
    {
        uint32_t before = 0;  // pulses in front of block b: those wholly inside earlier blocks and those stitched across borders
        uint32_t cw = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const PulseSeg &S = table[b];
            if (S.lead_w == S.n) { cw += S.lead_w; continue; }
            if (cw + S.lead_w >= c.min_width) ++before;
            const uint32_t room = c.max_pulses > before ? c.max_pulses - before : 0u;
            if ((S.inner < room ? S.inner : room) > c.cap) expect_complete = false;
            before += S.inner;
            cw = S.trail_w;
        }
    }
    std::vector<uint32_t> base(nb, 0xffffffffu);
    const bool complete = pulse_stitch(
        nb, c.min_width, c.max_pulses, c.cap, [&](uint32_t b) { return table[b]; },
        [&](uint32_t p, uint32_t s, uint32_t w, int64_t key, int64_t sum) {
            CHECK(p < c.max_pulses && !written[p], "case %d: slot %u emitted twice or out of range", id, p);
            if (p < c.max_pulses) { written[p] = 1; pulse_record(&got[(size_t)p * 5], s, w, key, sum, c.neg); }
        },
        [&](uint32_t b, uint32_t r, uint32_t p) {
            CHECK(p < c.max_pulses && !written[p] && r < c.cap && r < staged[b], "case %d: copy of block %u record %u to slot %u", id, b, r, p);
            if (p < c.max_pulses && r < c.cap) { written[p] = 1; memcpy(&got[(size_t)p * 5], &staging[((size_t)b * c.cap + r) * 5], 5 * sizeof(int64_t)); }
        },
        [&](uint32_t b, uint32_t first) { base[b] = first; }, &got_count);
    // the second launch: an incomplete waveform's blocks run again, each knowing the number of its first pulse, and write the
    // slots themselves (those the stitch filled already receive the same record)
    if (!complete) {
        for (uint32_t b = 0; b < nb; ++b)
            for (uint32_t r = 0; r < staged[b]; ++r) {
                CHECK(base[b] != 0xffffffffu, "case %d block %u holds pulses and was told no number", id, b);
                const uint32_t p = base[b] + r;
                if (p >= c.max_pulses) break;
                if (written[p]) CHECK(memcmp(&got[(size_t)p * 5], &full[b][(size_t)r * 5], 5 * sizeof(int64_t)) == 0, "case %d: slot %u written twice, differently", id, p);
                written[p] = 1;
                memcpy(&got[(size_t)p * 5], &full[b][(size_t)r * 5], 5 * sizeof(int64_t));
            }
        for (uint32_t p = 0; p < c.max_pulses && p < want_count; ++p) CHECK(written[p], "case %d: slot %u of %u pulses still missing behind the second launch", id, p, want_count);
    }
    CHECK(got_count == want_count, "case %d: count %u, the loop's %u", id, got_count, want_count);
    CHECK(complete == expect_complete, "case %d: complete %d, expected %d", id, (int)complete, (int)expect_complete);
    for (uint32_t p = 0; p < c.max_pulses; ++p) {
        if (!written[p]) {
            CHECK(!complete || p >= want_count, "case %d: slot %u of %u pulses not written by a complete stitch", id, p, want_count);
            continue;
        }
        CHECK(memcmp(&got[(size_t)p * 5], &want[(size_t)p * 5], 5 * sizeof(int64_t)) == 0,
              "case %d: slot %u = {%lld %lld %lld %lld %lld}, the loop's {%lld %lld %lld %lld %lld}", id, p, (long long)got[p * 5], (long long)got[p * 5 + 1],
              (long long)got[p * 5 + 2], (long long)got[p * 5 + 3], (long long)got[p * 5 + 4], (long long)want[p * 5], (long long)want[p * 5 + 1],
              (long long)want[p * 5 + 2], (long long)want[p * 5 + 3], (long long)want[p * 5 + 4]);
    }
}

int main() {
    const int n_cases = 6000;
    int all_over = 0, none_over = 0, clamp_lo = 0, clamp_hi = 0, negs = 0;
    for (int id = 0; id < n_cases; ++id) {
        Case c;
        const uint32_t L = rnd(1, 300);
        c.y.resize(L);
        const uint32_t kind = rnd(0, 9);
        const int32_t centre = (int32_t)rnd(0, 60000) - 30000, spread = (int32_t)rnd(1, 6);
        const bool extremes = rnd(0, 7) == 0;  // samples at the ends of the int16 range
        for (uint32_t i = 0; i < L; ++i) {
            int32_t v;
            switch (kind) {
                case 0: v = centre + spread; break;                                      // every sample over (positive polarity)
                case 1: v = centre - spread; break;                                      // none
                case 2: v = centre + ((i & 1u) ? spread : -spread); break;               // alternating
                case 3: v = centre + (((i / rnd(1, 9)) & 1u) ? spread : -spread); break;  // ragged square wave
                default: v = centre + (int32_t)rnd(0, 2u * (uint32_t)spread) - spread; break;
            }
            if (extremes) v = rnd(0, 1) ? (rnd(0, 3) ? 32767 : 32766) : (rnd(0, 3) ? -32768 : -32767);
            c.y[i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
        }
        c.neg = rnd(0, 1) != 0;
        negs += c.neg;
        c.min_width = rnd(1, 8);
        c.max_pulses = rnd(0, 6);
        c.cap = rnd(0, 1) ? rnd(0, 6) : (c.max_pulses < 2u ? c.max_pulses : 2u);
        // the threshold: a table entry and an offset, the sum saturating; beyond both clamps now and then
        int64_t tab = centre, off = 0;
        const uint32_t tk = rnd(0, 11);
        if (tk == 0) { tab = INT64_MAX - 5; off = 100; }          // saturates at the top: nothing over / everything below
        else if (tk == 1) { tab = INT64_MIN + 5; off = -100; }    // saturates at the bottom
        else if (tk == 2) { tab = 32767; off = rnd(0, 2); }       // the clamps themselves and one beyond
        else if (tk == 3) { tab = -32768; off = -(int64_t)rnd(0, 2); }
        else if (tk == 4) { tab = 40000; off = 0; }
        else if (tk == 5) { tab = -40000; off = 0; }
        else off = (int64_t)rnd(0, 4) - 2;
        if (extremes && tk > 5) tab = rnd(0, 1) ? 32766 : -32767;
        const bool has_tab = rnd(0, 3) != 0;
        __int128 sum = (has_tab ? (__int128)tab : 0) + off;
        c.t = sum > INT64_MAX ? INT64_MAX : (sum < INT64_MIN ? INT64_MIN : (int64_t)sum);
        c.tv = pulse_threshold(has_tab, tab, off, c.neg);
        clamp_hi += c.t > 32767;
        clamp_lo += c.t < -32768;
        uint32_t n_over = 0;
        for (uint32_t i = 0; i < L; ++i) n_over += c.neg ? (int64_t)c.y[i] < c.t : (int64_t)c.y[i] > c.t;
        all_over += n_over == L;
        none_over += n_over == 0;
        run_case(c, id);
    }
    printf("%d cases: %d all over, %d none over, %d above the upper clamp, %d below the lower, %d negative polarity; %d failures\n", n_cases, all_over,
           none_over, clamp_hi, clamp_lo, negs, failures);
    if (all_over < 50 || none_over < 50 || clamp_hi < 50 || clamp_lo < 50 || negs < 1000 || n_cases - negs < 1000) {
        printf("FAIL: the cases do not cover what they should\n");
        return 1;
    }
    return failures ? 1 : 0;
}
