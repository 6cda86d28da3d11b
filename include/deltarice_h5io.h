/*
 * deltarice_h5io.h -- direct-chunk HDF5 file <-> VRAM path.
 *
 * The H5Z callback (deltarice_h5filter.h) is handed one chunk at a time in host memory, so
 * every chunk crosses PCIe twice and costs a kernel launch of its own; the reference's authors
 * measured the same ceiling for their GPU prototype ("File -> VRAM", docs/Performance.md:74,87,89).
 * This interface moves whole datasets instead: the stored (filtered) bytes of all chunks go
 * between the file and ONE pinned staging buffer with H5Dread_chunk / H5Dwrite_chunk (HDF5 >=
 * 1.10.3, no filter pipeline involved), one PCIe copy, and ONE drx_decode / drx_encode over the
 * whole batch.  Files are bit-compatible both ways with the filter path and with the reference.
 *
 * Datasets: 2-D, 16-bit little-endian integers (signed or unsigned: the bytes are what is coded), chunked as
 * (chunk_rows x all columns), filter 32025 alone in the pipeline with any cd_values the filter accepts.  A chunk
 * that was never written (fill value only) is DRX_ERR_UNSUPPORTED, another element type or byte order likewise.
 * This library links libhdf5 (the application's); the codec itself stays in libdeltarice_hip.so.
 */
#ifndef DELTARICE_H5IO_H
#define DELTARICE_H5IO_H

#include <stdint.h>

#include "deltarice_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t rows, cols, chunk_rows, n_chunks;
    uint64_t raw_bytes, stored_bytes;  /* int16 payload / bytes in the file's chunks */
    double t_file, t_pcie, t_gpu;      /* seconds: HDF5 chunk I/O, host<->device copies, codec kernels */
} drx_h5_stats;

/* File -> VRAM: decodes dataset `name` of `file` into d_out (device int16[out_cap_samples]). */
drx_status drx_h5_read(drx_ctx *ctx, const char *file, const char *name, int16_t *d_out,
                       uint64_t out_cap_samples, drx_h5_stats *stats);

/* File -> VRAM, selected rows: row i of d_out (device int16[out_cap_samples], rows of `cols` samples back to back) receives
 * dataset row rows[i] (host array; any order, duplicates allowed).  Same datasets as drx_h5_read, with the further condition
 * that a row is a whole number of waveforms (cols % WaveformLength == 0; otherwise DRX_ERR_UNSUPPORTED).  Only the stored
 * bytes of the chunks the rows lie in are fetched (H5Dread_chunk into the context's staging buffer), copied to the device
 * once and decoded by one drx_decode_select over a plan of those chunks: stats->n_chunks and stats->stored_bytes count
 * what was fetched, stats->raw_bytes what was delivered; the other chunks are neither read nor validated.
 * A row >= the dataset's rows: DRX_ERR_ARG. */
drx_status drx_h5_read_rows(drx_ctx *ctx, const char *file, const char *name, const uint64_t *rows, uint64_t n_rows,
                            int16_t *d_out, uint64_t out_cap_samples, drx_h5_stats *stats);

/* File -> file, selected rows: dataset `dst_name` of `dst_file` (created / truncated as drx_h5_write does; dst_file equal to
 * src_file: DRX_ERR_ARG) receives the n_rows x cols rows `rows` names (host array; any order, duplicates allowed; n_rows >= 1),
 * in chunks of dst_chunk_rows x cols (1 <= dst_chunk_rows <= n_rows; 0: the source's chunk rows, or n_rows where that is less), with the SOURCE's element type and cd_values verbatim
 * (general prediction filters included).  Source datasets as drx_h5_read_rows takes them.  The stored bytes of the chunks the
 * rows lie in are fetched, and ONE drx_gather_encoded with dst_chunk_rows * (cols / WaveformLength) waveforms per output chunk
 * makes the new chunks out of them without decoding a sample: they are the bytes the filter would write for those rows.
 * Where n_rows does not divide by dst_chunk_rows HDF5 stores the last chunk full size: that one chunk is decoded
 * (drx_decode_select), padded with the fill value 0 and encoded, as drx_h5_write pads its last chunk.  WaveformLength -1 (the
 * whole chunk is one waveform) needs chunks of one row on both sides, else DRX_ERR_UNSUPPORTED.
 * stats: n_chunks / stored_bytes count what was FETCHED, raw_bytes the int16 bytes the new dataset represents, rows /
 * chunk_rows describe the new dataset. */
drx_status drx_h5_copy_rows(drx_ctx *ctx, const char *src_file, const char *src_name, const uint64_t *rows, uint64_t n_rows,
                            const char *dst_file, const char *dst_name, uint64_t dst_chunk_rows, drx_h5_stats *stats);

/* File -> file, another RiceParameter: dataset `dst_name` of `dst_file` (created / truncated as drx_h5_write does; dst_file equal
 * to src_file: DRX_ERR_ARG) receives dataset `src_name` of `src_file` with every stored chunk re-coded at RiceParameter rice_m
 * (a power of two up to 32768; 0: the one that makes the dataset smallest, on a tie the smaller) and never decoded.  Source
 * datasets as drx_h5_read takes them.  The stored chunks go to the context's staging buffer and to the device as
 * drx_h5_copy_rows fetches them; then one drx_estimate_words_encoded (if rice_m is 0), one drx_transcode and H5Dwrite_chunk.
 * The new dataset has the source's shape, element type and chunking; its cd_values are the source's verbatim except
 * cd_values[0] (general prediction filters included: the chunks are the bytes the filter would write for the source's data
 * under the new cd_values).  stats: n_chunks / stored_bytes count what was FETCHED, raw_bytes the int16 bytes the dataset
 * represents. */
drx_status drx_h5_recompress(drx_ctx *ctx, const char *src_file, const char *src_name, const char *dst_file, const char *dst_name,
                             unsigned rice_m, drx_h5_stats *stats);
/* ... and another prediction filter: taps[n_taps] (1 <= n_taps <= DRX_MAX_TAPS, taps[0] != 0; {1, -1}: the delta filter) replaces
 * the source's; n_taps == 0 is drx_h5_recompress.  One drx_estimate_words_encoded_filter (if rice_m is 0) and one
 * drx_transcode_filter take the place of the estimate and the transcode: no decoded sample is held in memory.  The new dataset's
 * cd_values carry the new RiceParameter and the new taps as drx_h5_write_filtered stores them -- (m, WaveformLength, n_taps,
 * taps...), a delta target the two-value form (m, WaveformLength) -- and every stored chunk is the bytes the filter would write
 * for the source's DECODED data under them. */
drx_status drx_h5_recompress_filtered(drx_ctx *ctx, const char *src_file, const char *src_name, const char *dst_file, const char *dst_name,
                                      unsigned rice_m, unsigned n_taps, const int32_t *taps, drx_h5_stats *stats);

/* VRAM -> file: encodes d_in (device int16[rows*cols]) and writes it as dataset `name` (file is
 * created/truncated).  rice_m, wave_len: compression_opts (RiceParameter, WaveformLength). */
drx_status drx_h5_write(drx_ctx *ctx, const char *file, const char *name, const int16_t *d_in,
                        uint64_t rows, uint64_t cols, uint64_t chunk_rows, unsigned rice_m,
                        unsigned wave_len, drx_h5_stats *stats);

/* The same with a general prediction filter (cd_values[2..] = n_taps, taps..., src/deltaRice.c:277-289); n_taps = 0:
 * the delta filter, cd_values = (RiceParameter, WaveformLength) as drx_h5_write stores them. */
drx_status drx_h5_write_filtered(drx_ctx *ctx, const char *file, const char *name, const int16_t *d_in,
                                 uint64_t rows, uint64_t cols, uint64_t chunk_rows, unsigned rice_m,
                                 unsigned wave_len, unsigned n_taps, const int32_t *taps, drx_h5_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
