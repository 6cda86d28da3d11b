// The bin cursor of drx_wave_bins (deltarice_amd/csrc/drx_bin_cursor.h) on the host, against a scalar model in 128-bit
// arithmetic: sample i of a waveform whose bins start at a lies in bin floor((i - a) / bin) if i >= a and that is below n_bins,
// and in no bin otherwise.  A cursor begun at any sample i0 and moved on at every border must say the same of every sample it
// passes, bins_begin() must return the first bin that receives a sample at or behind i0, and a cursor walked from i0 to the
// waveform's end must leave the same empty rows behind the last bin as one walked from sample 0 (whose empty rows in front are
// the model's).  tests/test_bins_rule_host.py builds and runs this, plainly and under the sanitizers.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>

#include "drx_bin_cursor.h"

using namespace drx;

typedef __int128 i128;

// the model: the bin of sample i, n_bins for none
static uint32_t model_bin(int64_t a, uint32_t bin, uint32_t n_bins, uint32_t i) {
    const i128 d = (i128)i - (i128)a;
    if (d < 0) return n_bins;
    const i128 b = d / (i128)bin;
    return b < (i128)n_bins ? (uint32_t)b : n_bins;
}
// the first bin that receives a sample with index in [i0, len), n_bins for none
static uint32_t model_first(int64_t a, uint32_t bin, uint32_t n_bins, uint32_t len, uint32_t i0) {
    if (i0 >= len) return n_bins;
    if ((i128)a > (i128)i0) return (i128)a < (i128)len ? 0u : n_bins;
    return model_bin(a, bin, n_bins, i0);
}

static long mismatches = 0;
static void fail(const char *what, int64_t a, uint32_t bin, uint32_t n_bins, uint32_t len, uint32_t i0, uint32_t i, uint32_t got, uint32_t want) {
    if (++mismatches <= 20)
        std::printf("%s: a %" PRId64 " bin %u n_bins %u len %u i0 %u sample %u: %u, model %u\n", what, a, bin, n_bins, len, i0, i, got, want);
}

// walks [i0, i0 + count) and holds every sample to the model; returns the cursor behind the last sample
static BinCursor walk(int64_t a, uint32_t bin, uint32_t n_bins, uint32_t len, uint32_t i0, uint32_t count, uint32_t *first) {
    BinCursor c;
    *first = bins_begin(c, a, bin, n_bins, len, i0);
    for (uint32_t i = i0; i < i0 + count; ++i) {
        if (i == c.nb) bins_border(c, bin, n_bins, len);
        const uint32_t got = c.live ? c.cur : n_bins, want = model_bin(a, bin, n_bins, i);
        if (got != want || (c.live && c.cur >= n_bins)) fail("bin of a sample", a, bin, n_bins, len, i0, i, got, want);
    }
    return c;
}

int main() {
    std::mt19937_64 rng(20240607u);
    auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    const int64_t special[] = {INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, -((int64_t)1 << 31), ((int64_t)1 << 31), -((int64_t)1 << 31) - 1,
                               ((int64_t)1 << 31) - 1, ((int64_t)1 << 32), -((int64_t)1 << 32), 0, -1, 1};
    const uint32_t special_bin[] = {1u, 2u, 15u, 16u, 17u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    long tuples = 0;
    for (int t = 0; t < 240000; ++t) {
        const bool small = t % 4 != 3;  // three in four: a waveform short enough to be walked whole, from 0 and from i0
        const uint32_t len = small ? (uint32_t)below(513) : (uint32_t)(1u + below(0x7fffffffu));
        int64_t a;
        switch (below(4)) {
            case 0: a = special[below(sizeof special / sizeof *special)]; break;
            case 1: a = (int64_t)below(2u * (uint64_t)len + 600u) - 300 - (int64_t)len / 2; break;
            case 2: a = (int64_t)rng(); break;
            default: a = (int64_t)below(1u << 16) - (1 << 15); break;
        }
        uint32_t bin;
        switch (below(4)) {
            case 0: bin = special_bin[below(sizeof special_bin / sizeof *special_bin)]; break;
            case 1: bin = 1u + (uint32_t)below(40); break;
            case 2: bin = 1u + (uint32_t)below((uint64_t)len + 2u); break;
            default: bin = 1u + (uint32_t)below(0xffffffffull); break;
        }
        const uint32_t n_bins = below(3) == 0 ? 1u + (uint32_t)below(0xffffffffull) : 1u + (uint32_t)below(2u * (uint64_t)len / bin + 4u);
        const uint32_t i0 = len ? (uint32_t)below(len) : 0u;
        ++tuples;
        uint32_t first = 0;
        if (small) {
            uint32_t first0 = 0;
            const BinCursor c0 = walk(a, bin, n_bins, len, 0u, len, &first0);
            // (a waveform of no samples: the lane kernels store the row the cursor names with the identity's values, as they store
            // an empty row, so what bins_begin() returns there is not held to the model)
            if (len && first0 != model_first(a, bin, n_bins, len, 0u)) fail("empty rows in front", a, bin, n_bins, len, 0u, 0u, first0, model_first(a, bin, n_bins, len, 0u));
            const BinCursor c1 = walk(a, bin, n_bins, len, i0, len - i0, &first);
            const uint32_t trail0 = c0.cur + (c0.live ? 1u : 0u), trail1 = c1.cur + (c1.live ? 1u : 0u);
            if (len && trail0 != trail1) fail("empty rows behind", a, bin, n_bins, len, i0, len, trail1, trail0);
        } else {
            const uint32_t want = (uint32_t)below(200);
            const uint32_t count = want < len - i0 ? want : len - i0;
            (void)walk(a, bin, n_bins, len, i0, count, &first);
        }
        if (len && first != model_first(a, bin, n_bins, len, i0)) fail("first bin", a, bin, n_bins, len, i0, i0, first, model_first(a, bin, n_bins, len, i0));
    }
    std::printf("%ld tuples, %ld mismatches\n", tuples, mismatches);
    return mismatches ? 1 : 0;
}
