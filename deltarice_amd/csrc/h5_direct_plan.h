/*
 * h5_direct_plan.h -- what the direct-chunk HDF5 path (h5_direct.c) computes from numbers alone: slabs of chunks, rows to
 * fetched chunks and waveform indices, the row geometry drx_h5_read_rows / drx_h5_copy_rows accept, the cd_values of a new
 * dataset.  No HDF5, no device runtime and no project header: tests/h5_direct_plan_host.c holds it to a plain restatement on
 * the CPU.  The statuses are the numbers of drx_status (include/deltarice_hip.h).
 */
#ifndef H5_DIRECT_PLAN_H
#define H5_DIRECT_PLAN_H

#include <stdint.h>
#include <stdlib.h>

enum { GEOM_OK = 0, GEOM_ERR_ARG = 1, GEOM_ERR_UNSUPPORTED = 5 };

/* The chunks of a dataset in SLABS of consecutive chunks, at least 8 MB each and at most kMaxSlabs of them: the unit in which
 * data moves between the file and the device while the other side works on the slab before / behind it.
 * off_words[n_chunks + 1]: the chunks' word offsets; returns the number of slabs. */
enum { kMaxSlabs = 64 };
typedef struct { uint64_t c0, c1; } slab_t;
static inline int make_slabs(const uint64_t *off_words, uint64_t n_chunks, slab_t *slabs) {
    const uint64_t total = off_words[n_chunks] * 4;
    uint64_t target = total / kMaxSlabs + 1;
    if (target < (8u << 20)) target = 8u << 20;
    int n = 0;
    uint64_t c = 0;
    while (c < n_chunks) {
        uint64_t e = c + 1;
        while (e < n_chunks && (off_words[e] - off_words[c]) * 4 < target) ++e;
        if (n == kMaxSlabs - 1) e = n_chunks;
        slabs[n].c0 = c; slabs[n].c1 = e;
        ++n;
        c = e;
    }
    return n;
}

/* Rows as drx_h5_read_rows and drx_h5_copy_rows take them, of a dataset of n_data_rows x cols in chunks of chunk_rows x cols
 * stored with WaveformLength wave_len (-1: the whole chunk one waveform); dst_chunk_rows: the chunk rows of copy_rows' new
 * dataset, 0 where there is none.  GEOM_OK with *L the waveform length in samples and *wpr the waveforms per row, or the status
 * the call returns: a chunk above 2^31 - 1 samples on either side is ERR_ARG; a row that is no whole number of waveforms
 * (their samples are rows of drx_decode_select's output), or WaveformLength -1 with a new chunk of more than one row (the
 * cd_values travel verbatim), ERR_UNSUPPORTED; a row past the dataset's or 2^32 and more waveforms ERR_ARG. */
static inline int row_geometry(uint64_t n_data_rows, uint64_t cols, uint64_t chunk_rows, int64_t wave_len, uint64_t dst_chunk_rows,
                               const uint64_t *rows, uint64_t n_rows, uint64_t *L, uint64_t *wpr) {
    if (chunk_rows * cols > 0x7fffffffull || dst_chunk_rows * cols > 0x7fffffffull) return GEOM_ERR_ARG;
    *L = wave_len < 0 ? chunk_rows * cols : (uint64_t)wave_len;
    if (cols % *L != 0 || (wave_len < 0 && dst_chunk_rows > 1)) return GEOM_ERR_UNSUPPORTED;
    *wpr = cols / *L;
    for (uint64_t i = 0; i < n_rows; ++i) if (rows[i] >= n_data_rows) return GEOM_ERR_ARG;
    if (n_rows * *wpr >= (1ull << 32)) return GEOM_ERR_ARG;
    return GEOM_OK;
}

static inline int cmp_u64(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* The sorted set of chunks the rows lie in, into touched[n_rows]; returns their number.  (HDF5 stores a padded last chunk
 * full size: the same geometry as the others.) */
static inline uint64_t touched_chunks(const uint64_t *rows, uint64_t n_rows, uint64_t chunk_rows, uint64_t *touched) {
    for (uint64_t i = 0; i < n_rows; ++i) touched[i] = rows[i] / chunk_rows;
    qsort(touched, n_rows, sizeof(uint64_t), cmp_u64);
    uint64_t n = 0;
    for (uint64_t i = 0; i < n_rows; ++i) if (!n || touched[n - 1] != touched[i]) touched[n++] = touched[i];
    return n;
}

/* The rows as waveform indices of a uniform plan over the touched chunks, wave_idx[n_rows * wpr]: row r is waveforms
 * ((place of its chunk among the touched) * chunk_rows + its row within the chunk) * wpr + 0 .. wpr - 1. */
static inline void rows_to_waves(const uint64_t *rows, uint64_t n_rows, uint64_t chunk_rows, uint64_t wpr,
                                 const uint64_t *touched, uint64_t n_touched, uint64_t *wave_idx) {
    for (uint64_t i = 0; i < n_rows; ++i) {
        const uint64_t c = rows[i] / chunk_rows, lr = rows[i] % chunk_rows;
        uint64_t lo = 0, hi = n_touched;  /* invariant: touched[lo] <= c < touched[hi] */
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (touched[mid] <= c) lo = mid; else hi = mid;
        }
        for (uint64_t j = 0; j < wpr; ++j) wave_idx[i * wpr + j] = (lo * chunk_rows + lr) * wpr + j;
    }
}

/* cd_values as drx_h5_write_filtered stores them into cd[3 + n_taps]; returns their number: (m, WaveformLength) for the delta
 * filter (n_taps == 0), (m, WaveformLength, n_taps, taps...) for a general one; wave_len 0 is WaveformLength -1. */
static inline size_t write_cd_values(unsigned rice_m, unsigned wave_len, unsigned n_taps, const int32_t *taps, unsigned *cd) {
    cd[0] = rice_m;
    cd[1] = wave_len ? wave_len : 0xffffffffu;
    if (!n_taps) return 2;
    cd[2] = n_taps;
    for (unsigned j = 0; j < n_taps; ++j) cd[3 + j] = (unsigned)taps[j];
    return 3 + (size_t)n_taps;
}

/* The cd_values of drx_h5_recompress[_filtered]'s new dataset, in place over the source's cd[ncd] (room for 3 + n_taps);
 * returns their number.  Without target taps: the source's verbatim with cd[0] = m (a dataset stored under the default
 * RiceParameter names none: then that one value).  With them: what write_cd_values stores for (m, the source's
 * WaveformLength wave_len, the taps), a delta target {1, -1} the two-value form. */
static inline size_t recompress_cd_values(size_t ncd, unsigned *cd, unsigned m, int64_t wave_len, unsigned n_taps, const int32_t *taps) {
    if (!n_taps) {
        cd[0] = m;
        return ncd ? ncd : 1;
    }
    const int delta = n_taps == 2 && taps[0] == 1 && taps[1] == -1;
    return write_cd_values(m, wave_len < 0 ? 0u : (unsigned)wave_len, delta ? 0 : n_taps, taps, cd);
}

#endif
