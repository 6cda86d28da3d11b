/* h5_direct_plan_host.c -- deltarice_amd/csrc/h5_direct_plan.h on the host, against a plain restatement
 * (tests/test_h5_direct_plan_host.py compiles this with the host compiler and -fsanitize=address,undefined and runs it).
 *
 * make_slabs: the slabs partition [0, n_chunks) in order, number at most kMaxSlabs, and each but the last reaches
 * max(8 MB, total / 64 + 1).  touched_chunks / rows_to_waves: against a linear search over a sorted set.  row_geometry: each
 * refusal at its edge, and the precedence where two apply.  The cd_values of a new dataset: the cases written out in
 * include/deltarice_h5io.h.  Fixed cases, then some thousands of random ones. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "h5_direct_plan.h"

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

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64(void) {  /* xorshift64* */
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rnd64() % (hi - lo + 1u); }  /* inclusive */

/* ---- slabs ---- */
static void slab_case(const char *what, const uint64_t *bytes, uint64_t n_chunks) {  /* bytes: a multiple of 4 each */
    ++cases;
    uint64_t *off = (uint64_t *)malloc((n_chunks + 1) * sizeof *off);
    off[0] = 0;
    for (uint64_t c = 0; c < n_chunks; ++c) off[c + 1] = off[c] + bytes[c] / 4;
    slab_t slabs[kMaxSlabs + 1];
    memset(slabs, 0xff, sizeof slabs);
    const int n = make_slabs(off, n_chunks, slabs);
    const uint64_t total = off[n_chunks] * 4;
    uint64_t want = total / 64 + 1;
    if (want < 8u * 1024 * 1024) want = 8u * 1024 * 1024;
    CHECK(n >= 1 && n <= kMaxSlabs && n <= 64, "%s: %d slabs", what, n);
    uint64_t at = 0;
    for (int s = 0; s < n && s < kMaxSlabs; ++s) {
        CHECK(slabs[s].c0 == at && slabs[s].c1 > slabs[s].c0 && slabs[s].c1 <= n_chunks, "%s: slab %d = [%llu, %llu) at %llu", what, s,
              (unsigned long long)slabs[s].c0, (unsigned long long)slabs[s].c1, (unsigned long long)at);
        at = slabs[s].c1;
        if (s + 1 < n) CHECK((off[slabs[s].c1] - off[slabs[s].c0]) * 4 >= want, "%s: slab %d is short of %llu bytes", what, s, (unsigned long long)want);
    }
    CHECK(at == n_chunks, "%s: the slabs end at %llu of %llu", what, (unsigned long long)at, (unsigned long long)n_chunks);
    CHECK(slabs[kMaxSlabs].c0 == ~0ull, "%s: a slab behind the last", what);
    free(off);
}
static void slab_cases(void) {
    const uint64_t MB = 1024 * 1024;
    uint64_t *b = (uint64_t *)malloc(100000 * sizeof *b);
    b[0] = 4; slab_case("one tiny chunk", b, 1);
    b[0] = 3000 * MB; slab_case("one huge chunk", b, 1);
    for (int i = 0; i < 65; ++i) b[i] = 8 * MB;
    slab_case("64 chunks of 8 MB", b, 64);
    slab_case("65 chunks of 8 MB", b, 65);
    for (int i = 0; i < 100000; ++i) b[i] = 40;
    slab_case("100 000 tiny chunks", b, 100000);
    for (int i = 0; i < 100000; ++i) b[i] = 4 * rnd(1, 3 * MB);
    slab_case("100 000 chunks of up to 12 MB", b, 100000);
    b[0] = 8 * MB - 4; b[1] = 4; b[2] = 4;
    slab_case("8 MB less a word, a word, a word", b, 3);
    for (int r = 0; r < 1500; ++r) {
        const uint64_t n = rnd(1, r % 3 ? 300 : 3000), top = (uint64_t[]){64, 64 * 1024, 2 * MB, 40 * MB}[r % 4];
        for (uint64_t i = 0; i < n; ++i) b[i] = 4 * rnd(1, top / 4);
        slab_case("random", b, n);
    }
    free(b);
}

/* ---- rows -> touched chunks -> waveform indices ---- */
static void rows_case(const char *what, const uint64_t *rows, uint64_t n_rows, uint64_t chunk_rows, uint64_t wpr) {
    ++cases;
    /* the plain restatement: a sorted set by insertion, the place of a chunk in it by a linear search */
    uint64_t *set = (uint64_t *)malloc(n_rows * sizeof *set), n_set = 0;
    for (uint64_t i = 0; i < n_rows; ++i) {
        const uint64_t c = rows[i] / chunk_rows;
        uint64_t at = 0;
        while (at < n_set && set[at] < c) ++at;
        if (at < n_set && set[at] == c) continue;
        memmove(set + at + 1, set + at, (n_set - at) * sizeof *set);
        set[at] = c;
        ++n_set;
    }
    uint64_t *touched = (uint64_t *)malloc(n_rows * sizeof *touched), *idx = (uint64_t *)malloc(n_rows * wpr * sizeof *idx);
    const uint64_t n = touched_chunks(rows, n_rows, chunk_rows, touched);
    CHECK(n == n_set && !memcmp(touched, set, n_set * sizeof *set), "%s: %llu touched chunks, %llu in the set", what, (unsigned long long)n, (unsigned long long)n_set);
    if (n == n_set) {
        rows_to_waves(rows, n_rows, chunk_rows, wpr, touched, n, idx);
        for (uint64_t i = 0; i < n_rows; ++i) {
            uint64_t place = 0;
            while (set[place] != rows[i] / chunk_rows) ++place;
            for (uint64_t j = 0; j < wpr; ++j)
                CHECK(idx[i * wpr + j] == (place * chunk_rows + rows[i] % chunk_rows) * wpr + j, "%s: row %llu (entry %llu), waveform %llu: index %llu",
                      what, (unsigned long long)rows[i], (unsigned long long)i, (unsigned long long)j, (unsigned long long)idx[i * wpr + j]);
        }
    }
    free(set); free(touched); free(idx);
}
static void rows_cases(void) {
    const uint64_t dup[] = {5, 1, 5, 5, 9, 1}, down[] = {15, 12, 9, 8, 4, 3, 0}, one[] = {6, 4, 7, 4}, padded[] = {0, 13, 12}, single[] = {3};
    for (int w = 0; w < 2; ++w) {
        const uint64_t wpr = w ? 7 : 1;
        rows_case("duplicates", dup, 6, 4, wpr);
        rows_case("descending rows", down, 7, 4, wpr);
        rows_case("all rows in one chunk", one, 4, 4, wpr);
        rows_case("a row in the padded last chunk (14 rows in chunks of 4)", padded, 3, 4, wpr);
        rows_case("one row", single, 1, 4, wpr);
        rows_case("chunks of one row", down, 7, 1, wpr);
    }
    uint64_t rows[600];
    for (int r = 0; r < 3000; ++r) {
        const uint64_t n = rnd(1, r % 5 ? 40 : 600), chunk_rows = rnd(1, r % 2 ? 9 : 500), n_data = r % 7 ? rnd(1, 5000) : rnd(1, 1ull << 40);
        for (uint64_t i = 0; i < n; ++i) rows[i] = rnd(0, n_data - 1);
        rows_case("random", rows, n, chunk_rows, (uint64_t[]){1, 7, 2, 3}[r % 4]);
    }
}

/* ---- the geometry drx_h5_read_rows and drx_h5_copy_rows accept ---- */
/* the plain restatement: the refusals in the order of include/deltarice_h5io.h's calls */
static int plain_geometry(uint64_t n_data, uint64_t cols, uint64_t chunk_rows, int64_t wave_len, uint64_t dst_chunk_rows, const uint64_t *rows, uint64_t n_rows,
                          uint64_t *L, uint64_t *wpr) {
    if (chunk_rows * cols >= (1ull << 31)) return 1;
    if (dst_chunk_rows && dst_chunk_rows * cols >= (1ull << 31)) return 1;
    *L = wave_len == -1 ? chunk_rows * cols : (uint64_t)wave_len;
    if (cols % *L) return 5;
    if (wave_len == -1 && dst_chunk_rows && dst_chunk_rows != 1) return 5;
    *wpr = cols / *L;
    for (uint64_t i = 0; i < n_rows; ++i) if (rows[i] >= n_data) return 1;
    if (n_rows * *wpr > 0xffffffffull) return 1;
    return 0;
}
static void geometry_case(const char *what, uint64_t n_data, uint64_t cols, uint64_t chunk_rows, int64_t wave_len, uint64_t dst_chunk_rows,
                          const uint64_t *rows, uint64_t n_rows, int want) {
    ++cases;
    uint64_t L = 0, wpr = 0, L2 = 0, wpr2 = 0;
    const int got = row_geometry(n_data, cols, chunk_rows, wave_len, dst_chunk_rows, rows, n_rows, &L, &wpr);
    const int plain = plain_geometry(n_data, cols, chunk_rows, wave_len, dst_chunk_rows, rows, n_rows, &L2, &wpr2);
    CHECK(got == plain && (want < 0 || got == want), "%s: status %d, the restatement's %d, expected %d", what, got, plain, want);
    if (got == 0 && plain == 0) CHECK(L == L2 && wpr == wpr2, "%s: L %llu wpr %llu", what, (unsigned long long)L, (unsigned long long)wpr);
}
static void geometry_cases(void) {
    const uint64_t r01[] = {0, 1}, r16[] = {0, 16}, r15[] = {15, 0};
    geometry_case("whole waveforms", 16, 1000, 4, 500, 0, r15, 2, 0);
    geometry_case("cols % L != 0", 16, 1000, 4, 300, 0, r01, 2, 5);
    geometry_case("L above cols", 16, 1000, 4, 4000, 0, r01, 2, 5);
    geometry_case("whole chunk, chunks of four rows", 16, 1000, 4, -1, 0, r01, 2, 5);
    geometry_case("whole chunk, chunks of one row", 16, 1000, 1, -1, 0, r01, 2, 0);
    geometry_case("whole chunk, chunks of one row, new chunks of one", 16, 1000, 1, -1, 1, r01, 2, 0);
    geometry_case("whole chunk, chunks of one row, new chunks of two", 16, 1000, 1, -1, 2, r01, 2, 5);
    geometry_case("a row equal to the dataset's row count", 16, 1000, 4, 500, 0, r16, 2, 1);
    geometry_case("... which cols % L precedes", 16, 1000, 4, 300, 0, r16, 2, 5);
    geometry_case("no rows", 16, 1000, 4, 500, 0, NULL, 0, 0);
    geometry_case("no rows, cols % L != 0", 16, 1000, 4, 300, 0, NULL, 0, 5);
    /* chunk_rows * cols at 2^31 - 1 and 2^31, on either side */
    geometry_case("a chunk of 2^31 - 1 samples", 16, 0x7fffffffull, 1, 0x7fffffff, 0, r01, 2, 0);
    geometry_case("a chunk of 2^31 samples", 16, 1ull << 30, 2, 1 << 30, 0, r01, 2, 1);
    geometry_case("... which precedes cols % L", 16, 1ull << 30, 2, 300, 0, r01, 2, 1);
    geometry_case("a new chunk of 2^31 - 1 samples", 16, 0x7fffffffull, 1, 0x7fffffff, 1, r01, 2, 0);
    geometry_case("a new chunk of 2^31 samples", 16, 1ull << 30, 1, 1 << 30, 2, r01, 2, 1);
    /* n_rows * wpr at 2^32 - 1 and 2^32: 65537 * 65535 = 2^32 - 1, 65536 * 65536 = 2^32 */
    uint64_t *many = (uint64_t *)calloc(65537, sizeof *many);
    geometry_case("2^32 - 1 waveforms", 16, 65535, 4, 1, 0, many, 65537, 0);
    geometry_case("2^32 waveforms", 16, 65536, 4, 1, 0, many, 65536, 1);
    free(many);
    uint64_t rows[8];
    for (int r = 0; r < 4000; ++r) {
        const uint64_t L = rnd(1, 64), cols = r % 3 ? L * rnd(1, 8) : rnd(1, 512), chunk_rows = r % 11 ? rnd(1, 8) : rnd(1, 1ull << 32), n_data = rnd(1, 64), n = rnd(0, 8);
        for (uint64_t i = 0; i < n; ++i) rows[i] = rnd(0, r % 4 ? n_data - 1 : n_data);
        geometry_case("random", n_data, cols, chunk_rows, r % 5 ? (int64_t)L : -1, (uint64_t[]){0, 1, 2, 1ull << 31}[rnd(0, 3)], rows, n, -1);
    }
}

/* ---- cd_values ---- */
static void cd_case(const char *what, size_t got_n, const unsigned *got, size_t want_n, const unsigned *want) {
    ++cases;
    CHECK(got_n == want_n && !memcmp(got, want, want_n * sizeof *want), "%s: %zu values, expected %zu", what, got_n, want_n);
}
#define CD(...) (sizeof((unsigned[]){__VA_ARGS__}) / sizeof(unsigned)), (const unsigned[]){__VA_ARGS__}
static void cd_cases(void) {
    const int32_t fir4[] = {1, -1, 1, -1}, delta[] = {1, -1}, one[] = {-3};
    unsigned cd[3 + 64 + 1];
    /* drx_h5_write[_filtered]: (RiceParameter, WaveformLength), then n_taps, taps... for a general filter; wave_len 0 is -1 */
    cd[2] = 0x5a5a5a5au;
    cd_case("write, delta", write_cd_values(8, 7000, 0, NULL, cd), cd, CD(8, 7000));
    CHECK(cd[2] == 0x5a5a5a5au, "write, delta: a third value written");
    cd_case("write, whole chunk", write_cd_values(16, 0, 0, NULL, cd), cd, CD(16, 0xffffffffu));
    cd_case("write, four taps", write_cd_values(8, 1500, 4, fir4, cd), cd, CD(8, 1500, 4, 1, 0xffffffffu, 1, 0xffffffffu));
    cd_case("write, {1, -1} given as taps", write_cd_values(8, 1500, 2, delta, cd), cd, CD(8, 1500, 2, 1, 0xffffffffu));
    /* drx_h5_recompress: the source's verbatim except cd_values[0] */
    memcpy(cd, (unsigned[]){8, 7000}, 8);
    cd_case("recompress (8, 7000)", recompress_cd_values(2, cd, 32, 7000, 0, NULL), cd, CD(32, 7000));
    memcpy(cd, (unsigned[]){8, 1500, 4, 1, 0xffffffffu, 1, 0xffffffffu, 77}, 32);
    cd_case("recompress, a general filter and a value behind it", recompress_cd_values(8, cd, 1, 1500, 0, NULL), cd, CD(1, 1500, 4, 1, 0xffffffffu, 1, 0xffffffffu, 77));
    memcpy(cd, (unsigned[]){8}, 4);
    cd_case("recompress (8)", recompress_cd_values(1, cd, 32768, -1, 0, NULL), cd, CD(32768));
    cd_case("recompress, no cd_values: ncd == 0 becomes 1", recompress_cd_values(0, cd, 4, -1, 0, NULL), cd, CD(4));
    /* drx_h5_recompress_filtered: (m, WaveformLength, n_taps, taps...), a delta target the two-value form */
    memcpy(cd, (unsigned[]){8, 7000}, 8);
    cd_case("refilter delta -> four taps", recompress_cd_values(2, cd, 16, 7000, 4, fir4), cd, CD(16, 7000, 4, 1, 0xffffffffu, 1, 0xffffffffu));
    cd_case("refilter four taps -> delta", recompress_cd_values(7, cd, 8, 7000, 2, delta), cd, CD(8, 7000));
    cd_case("refilter no cd_values -> one tap", recompress_cd_values(0, cd, 8, -1, 1, one), cd, CD(8, 0xffffffffu, 1, 0xfffffffdu));
    memcpy(cd, (unsigned[]){8}, 4);
    cd_case("refilter (8) -> delta: WaveformLength -1 is 0xffffffff", recompress_cd_values(1, cd, 2, -1, 2, delta), cd, CD(2, 0xffffffffu));
    int32_t taps[64];
    unsigned want[3 + 64];
    for (int r = 0; r < 2000; ++r) {
        const unsigned n_taps = (unsigned)rnd(1, 64), m = 1u << rnd(0, 15), src_n = (unsigned)rnd(0, 8);
        const int64_t wave_len = r % 4 ? (int64_t)rnd(1, 0x7fffffff) : -1;
        for (unsigned j = 0; j < n_taps; ++j) taps[j] = (int32_t)(uint32_t)rnd64();
        if (!taps[0]) taps[0] = 1;
        const int is_delta = n_taps == 2 && taps[0] == 1 && taps[1] == -1;
        want[0] = m; want[1] = wave_len < 0 ? 0xffffffffu : (unsigned)wave_len; want[2] = n_taps;
        for (unsigned j = 0; j < n_taps; ++j) want[3 + j] = (unsigned)taps[j];
        for (unsigned j = 0; j < 3 + 64 + 1; ++j) cd[j] = (unsigned)rnd64();
        cd_case("random refilter", recompress_cd_values(src_n, cd, m, wave_len, n_taps, taps), cd, is_delta ? 2 : 3 + n_taps, want);
        for (unsigned j = 0; j < 3 + 64; ++j) cd[j] = want[j] = (unsigned)rnd64();
        want[0] = m;
        cd_case("random recompress", recompress_cd_values(src_n, cd, m, wave_len, 0, NULL), cd, src_n ? src_n : 1, want);
    }
}

int main(void) {
    slab_cases();
    rows_cases();
    geometry_cases();
    cd_cases();
    printf("%d cases; %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
