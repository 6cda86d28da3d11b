/*
 * deltarice_hip.h -- C ABI of the MI355X (gfx950) Delta-Rice codec.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * It replaces the arithmetic of the reference's per-chunk filter
 * (/root/reference/src/deltaRice.c) with HIP kernels; the HDF5-facing surface
 * (H5Z_filter_deltarice, H5Z_DELTARICE, registration, plugin entry points) is
 * declared in deltarice_h5filter.h and is a thin host wrapper over this file.
 *
 * Reference interface replaced by each entry point:
 *   drx_parse_cd_values      parseCD_VALUES + determinePowerOf2  src/deltaRice.c:248-291,114-136
 *   drx_encode               writeWholeCompressedByteString      src/deltaRice.c:383-441
 *                            (perWaveCompression :365-381, encodeWaveform :49-63,
 *                             compressWithRiceCoding :191-244), for a batch of chunks
 *   drx_decode               readWholeCompressedByteString       src/deltaRice.c:301-341
 *                            (perWaveDecompression :293-297, decompressWithRiceCoding
 *                             :138-189, decodeWaveform :78-90), for a batch of chunks
 *   drx_filter_chunk_host    the body of H5Z_filter_deltarice    src/deltaRice.c:468-490
 *                            (host buffer in, malloc'ed host buffer out, one chunk)
 *
 * Data model.  A *batch* is a list of HDF5 chunks.  Chunk c holds n_samples[c]
 * int16 samples cut into waveforms of wave_len[c] samples (the last one may be
 * shorter, src/deltaRice.c:399-403).  Raw chunks lie back to back in one int16
 * device buffer.  The encoded batch is one uint32 device buffer holding each
 * chunk's filtered bytes exactly as the reference's filter would emit them
 *   u32 n_samples | { u32 n_i | u32 payload_i[n_i] } per waveform
 * plus a table chunk_word_off[n_chunks+1] of where each chunk starts (the role
 * HDF5's chunk index plays in a file).
 *
 * All device pointers are on the context's device; every call is ordered on the
 * context's stream and returns without waiting.  Errors found on the device
 * (capacity, corrupt stream) are collected by drx_plan_finish().
 * There is no CPU fallback anywhere behind this ABI.
 *
 * Buffers.  A device pointer may have any alignment of its element type (int16 samples: 2 bytes, uint32 words: 4,
 * uint64 offsets: 8), such as a view at any element of a larger tensor or a stream that starts at any word of a larger
 * encoded buffer.  A call writes nothing outside [ptr, ptr + n) of the buffers it writes: out_cap_words words of an
 * encode's output, also when it fails with DRX_ERR_CAPACITY; n_chunks + 1 offsets; total_samples decoded samples.  Its
 * results depend neither on what those buffers held before the call nor on the words outside [0, in_words) of a decoder's
 * input.  tests/test_gpu_placement.py holds every encoder and decoder route to this.
 */
#ifndef DELTARICE_HIP_H
#define DELTARICE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRX_FILTER_ID 32025 /* H5Z_FILTER_DELTARICE, src/deltaRice.h:7 */
#define DRX_MAX_TAPS 64

typedef struct drx_ctx drx_ctx;   /* one device + one stream + scratch */
typedef struct drx_plan drx_plan; /* geometry of one batch, device resident */

typedef enum {
    DRX_OK = 0,
    DRX_ERR_ARG = 1,         /* bad argument / compression_opts (reference: stderr + -1, :116-135,394-397) */
    DRX_ERR_DEVICE = 2,      /* HIP runtime failure, or no usable GPU */
    DRX_ERR_CAPACITY = 3,    /* encoded batch does not fit out_cap_words */
    DRX_ERR_CORRUPT = 4,     /* encoded input fails validation (header chain, sizes) */
    DRX_ERR_UNSUPPORTED = 5, /* valid for the reference, not (yet) on the device */
    DRX_ERR_NOMEM = 6
} drx_status;

/* Parsed compression_opts = cd_values (src/deltaRice.c:248-291). */
typedef struct {
    uint32_t rice_k;   /* log2(RiceParameter), 0..15 */
    int64_t wave_len;  /* WaveformLength; -1 = the whole chunk is one waveform */
    uint32_t n_taps;   /* prediction filter; default 2 taps [1,-1] = delta */
    int32_t taps[DRX_MAX_TAPS];
} drx_opts;

const char *drx_version(void);
const char *drx_status_str(drx_status s);
int drx_device_count(void);

/* cd_values -> options.  Defaults: M=8, wave_len=-1, taps [1,-1]. */
drx_status drx_parse_cd_values(size_t cd_nelmts, const unsigned *cd_values, drx_opts *out);

/* hip_stream: a hipStream_t to borrow (e.g. the caller's), or NULL to create one. */
drx_status drx_ctx_create(int device, void *hip_stream, drx_ctx **out);
void drx_ctx_destroy(drx_ctx *ctx);
drx_status drx_ctx_synchronize(drx_ctx *ctx);
const char *drx_ctx_last_error(const drx_ctx *ctx);
void *drx_ctx_stream(const drx_ctx *ctx);
int drx_ctx_device(const drx_ctx *ctx); /* the HIP device the context was created on (-1 for NULL) */
/* A pinned host buffer of at least `bytes` that belongs to the context and is kept across calls (grown when a call asks for
 * more; freed with the context): staging for callers that move batches between host memory and the device, such as the
 * direct-chunk HDF5 path -- a fresh hipHostMalloc per call costs more than the copy it serves (7 ms for 113 MB).
 * One user at a time, like the context itself. */
drx_status drx_ctx_host_staging(drx_ctx *ctx, size_t bytes, void **host_out);

/* Plans.  chunk_wave_len[c] == 0 means "whole chunk" (WaveformLength = -1).
 * Allocates the per-waveform tables and the scratch of every path the batch's geometry takes by default on the device;
 * drx_decode allocates nothing, drx_encode only for a route that DRX_DBG_FORCE_STREAM_SEGS or DRX_DBG_FORCE_SEGMENTS forces.
 *
 * Threading: a context and its plans are for one thread at a time (calls are ordered on the context's stream);
 * drx_filter_chunk_host alone takes the context's lock and may be called from any thread (HDF5 does).
 * Every call runs on the context's device and restores the calling thread's current device before returning. */
drx_status drx_plan_create(drx_ctx *ctx, uint64_t n_chunks, const uint32_t *chunk_samples,
                           const uint32_t *chunk_wave_len, uint32_t rice_k, drx_plan **out);
drx_status drx_plan_create_uniform(drx_ctx *ctx, uint64_t n_chunks, uint32_t chunk_samples,
                                   uint32_t wave_len, uint32_t rice_k, drx_plan **out);
/* Prediction filter of the plan (cd_values[2..], src/deltaRice.c:277-289).  Default: the delta filter [1,-1].  Any other
 * taps (1 <= n_taps <= DRX_MAX_TAPS, taps[0] != 0) run on the GPU as well:
 *   up to four taps            the single-pass encoders' own kernels (forward filter in packed 16-bit math);
 *   ... and taps[0] = +-1      the fast decoders: a lane per waveform with the recurrence in the lane, or -- few long waveforms --
 *                              the block decoder with the inverse filter inside it (DRX_PATH_IIR_FUSED) or as a parallel pass of
 *                              its own behind it (DRX_PATH_IIR);
 *   anything else              the two-pass encoder and the simple decode kernel (DRX_PATH_SIMPLE): a lane per waveform, serial.
 * The arithmetic is the reference's modulo 2^16, the division by the whole int32 taps[0] towards zero; tests/test_gpu_filter_domain.py
 * holds every route to it over this domain (1 to 64 taps, coefficients up to the int32 extremes, any lead but 0).
 *   May be called on a plan that has been used, any number of times: it WAITS for the context's stream (calls in flight still
 * read the old filter's device tables, which it frees or replaces), forgets the code length the plan's last encode measured
 * (the next encode chooses its kernel as a new plan's would) and ends a pending drx_gather_encoded sizing call's resume.
 * The plan's geometry, scratch, RiceParameter and status word stay as they are. */
drx_status drx_plan_set_filter(drx_plan *plan, uint32_t n_taps, const int32_t *taps);
void drx_plan_destroy(drx_plan *plan);
uint64_t drx_plan_n_chunks(const drx_plan *plan);
uint64_t drx_plan_total_samples(const drx_plan *plan);
uint64_t drx_plan_total_waves(const drx_plan *plan);
/* Worst-case size of the encoded batch in uint32 words (25 bits per sample + headers). */
uint64_t drx_plan_max_encoded_words(const drx_plan *plan);

/* Encode.  d_in: int16[total_samples]; d_out: uint32[out_cap_words];
 * d_chunk_word_off: uint64[n_chunks+1], written (word index of each chunk's first
 * word in d_out; last entry = total words). */
drx_status drx_encode(drx_plan *plan, const int16_t *d_in, uint32_t *d_out, uint64_t out_cap_words,
                      uint64_t *d_chunk_word_off);

/* Decode.  d_in: uint32[in_words]; d_chunk_word_off: uint64[n_chunks+1], read;
 * d_out: int16[total_samples].  in_words is also what the decoder of few long waveforms sizes its blocks by
 * (32 in_words / total_samples bits per sample): stating the encoded size rather than a buffer's capacity
 * costs nothing and is worth up to 1.5x there; it never affects the result. */
drx_status drx_decode(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                      const uint64_t *d_chunk_word_off, int16_t *d_out);

/* Decode with a side-band: d_wave_words = the n_i of every waveform (uint32[total_waves], e.g. a copy of what
 * drx_plan_wave_words() shows after the drx_encode that produced d_in).  The reference's format has no index, so drx_decode
 * must find every waveform's header by walking or searching the stream (src/deltaRice.c:320-325); a device-resident pipeline
 * that still has the encoder's table can hand it back and skip that.  NOT part of the HDF5 drop-in surface (a file holds no
 * such table) and never used by bench.py.  The table is checked against the stream (every header word must equal its n_i,
 * the chain must end at the chunk's end): a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_decode_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                      const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words, int16_t *d_out);

/* Decode SELECTED waveforms.  wave_idx: HOST array of n_sel global waveform indices (0 ... total_waves - 1, any order,
 * duplicates allowed), consumed before the call returns; row i of d_out -- int16 at d_out + i * out_stride_samples -- receives
 * the len_i samples of waveform wave_idx[i] (WaveformLength, or less for the last waveform of a chunk) and nothing else is
 * written: the samples between rows keep what they held.  Otherwise asynchronous on the context's stream like drx_decode;
 * errors found on the device arrive at drx_plan_finish.
 *   Only the chunks that hold a selected waveform are walked (whole, with drx_decode's validation of the header chain: a
 * corrupt touched chunk is reported as drx_decode reports it, and then no waveform is decoded: d_out keeps what it held; a
 * payload found damaged while it is parsed is reported too, and which other rows were written by then is undefined).  The other
 * chunks are NEITHER READ NOR VALIDATED, and drx_plan_wave_words / drx_plan_wave_word_off after the call are valid for the
 * touched chunks only.
 *   DRX_ERR_ARG, with nothing launched: an index >= total_waves, out_stride_samples below the longest selected waveform,
 * n_sel >= 2^32, a NULL pointer with n_sel > 0.  n_sel == 0: DRX_OK, nothing launched.
 *   Every prediction filter the plan accepts: the delta filter a wavefront per selected waveform (parallel inside the
 * waveform), any other a lane per selected waveform.  The selection's scratch belongs to the plan: allocated by the first
 * such call, grown when a later one needs more. */
drx_status drx_decode_select(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint64_t *wave_idx, uint64_t n_sel, int16_t *d_out, uint64_t out_stride_samples);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device): no
 * walk; the table is checked against the stream for the touched chunks, its entries for the others are not looked at. */
drx_status drx_decode_select_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                             const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words,
                                             const uint64_t *wave_idx, uint64_t n_sel, int16_t *d_out,
                                             uint64_t out_stride_samples);

/* Gather SELECTED waveforms into a new ENCODED batch, without decoding them.  wave_idx: HOST array of n_sel global waveform
 * indices as drx_decode_select takes it (any order, duplicates allowed), consumed before the call returns.  Output chunk c holds
 * entries [c * out_chunk_waves, min(n_sel, (c + 1) * out_chunk_waves)) of the list, in list order; n_out_chunks =
 * ceil(n_sel / out_chunk_waves).  Its words are N_c | { n_i | payload_i } per entry, N_c the sum of the entries' sample counts;
 * the chunks lie back to back from d_out[0], and d_out_chunk_word_off (uint64[n_out_chunks + 1]) is written as drx_encode
 * writes it (last entry = total words).  A waveform is coded on its own and is a whole number of words (src/deltaRice.c:365-381,
 * 427-432), so these are the bytes drx_encode -- hence the reference's filter -- gives for the gathered samples under the source
 * plan's RiceParameter and prediction filter, whichever filter that is.  d_out_wave_words (uint32[n_sel], or NULL) receives the
 * n_i of every entry: the side-band of the result.
 *   One WaveformLength per output chunk: all its entries have the length of its first, except the last, which may be shorter.
 * That admits ragged source plans (group by length) and the short last waveform of a source chunk (at the end of an output
 * chunk only).
 *   DRX_ERR_ARG, with nothing launched: a list that breaks that rule (the message names the entry), an index >= total_waves,
 * out_chunk_waves == 0, n_sel >= 2^32, an output chunk of 2^31 samples or more (src/deltaRice.c:389), a NULL pointer among d_in,
 * d_chunk_word_off, wave_idx, d_out_chunk_word_off with n_sel > 0.  n_sel == 0: DRX_OK, nothing launched.
 *   Sizing.  The size of the result is known on the device before a word is copied.  d_out == NULL (with out_cap_words == 0)
 * runs exactly that far: the offset table and d_out_wave_words are written, drx_plan_finish reports the total, nothing else is
 * touched.  With d_out != NULL and a total above out_cap_words: DRX_ERR_CAPACITY at drx_plan_finish, which still reports the
 * total NEEDED, and not one word of d_out is written.
 *   The call behind a sizing call costs no second walk: the drx_gather_encoded call that follows a SIZING call on the same plan
 * with the same pointers, sizes and list (compared entry by entry), no other call on the plan in between, resumes from the
 * sizing call's tables -- once.  Every other call, also one that repeats the arguments of a call that copied, walks and
 * validates the stream anew.
 *   Asynchronous on the context's stream like drx_decode_select; errors found on the device arrive at drx_plan_finish.  Only
 * the chunks that hold a selected waveform are walked -- whole, with drx_decode's validation of the header chain: a corrupt
 * touched chunk is DRX_ERR_CORRUPT and nothing is copied.  The other chunks are NEITHER READ NOR VALIDATED.  Payload words are
 * COPIED, NOT PARSED: damage inside a payload that leaves the header chain intact travels to the output unnoticed (the
 * reference's own level of trust in a stored chunk).  drx_plan_wave_words / drx_plan_wave_word_off after the call are valid for
 * the touched chunks only.
 *   The buffers rule at the top of this file holds: any element alignment for d_in, d_out and both tables; nothing is written
 * outside [d_out, d_out + total), the n_out_chunks + 1 offsets and the n_sel table entries; the result depends neither on what
 * those held before nor on words outside [0, in_words).  d_out must not overlap d_in (not checked).  The gather's scratch
 * belongs to the plan beside the selection's: allocated by the first such call, grown when a later one needs more. */
drx_status drx_gather_encoded(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const uint64_t *wave_idx, uint64_t n_sel, uint64_t out_chunk_waves, uint32_t *d_out,
                              uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words);
/* ... with the encoder's side-band (d_wave_words: uint32[total_waves] on the device, neither the plan's own table nor
 * d_out_wave_words): no walk; the table is checked against the stream for the touched chunks as
 * drx_decode_select_with_wave_words checks it (a table that does not belong to the stream: DRX_ERR_CORRUPT). */
drx_status drx_gather_encoded_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                              const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words,
                                              const uint64_t *wave_idx, uint64_t n_sel, uint64_t out_chunk_waves, uint32_t *d_out,
                                              uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words);

/* Per-waveform STATISTICS straight from the encoded stream: what a cut needs of a waveform -- a baseline, an extreme and where
 * it sits, an integral, a noise figure -- without decoding the batch to memory.  d_out: int64[total_waves][DRX_STAT_COLS] on the
 * device; row g holds the eight values of global waveform g (the order of drx_plan_wave_words), computed over the int16 samples
 * y[0 .. len) that drx_decode would write for it (len = WaveformLength, or less for the last waveform of a chunk, which is a row
 * like any other; the samples of an unsigned dataset are read as int16, as they are coded).  Everything is exact: a waveform has
 * fewer than 2^31 samples, so every sum fits an int64.  head_len: the window of the two HEAD columns, e.g. a baseline in front
 * of the pulse; 0 gives 0 in both, a value beyond len the whole waveform.
 *   Asynchronous on the context's stream like drx_decode; the call clears the plan's status word first, errors found on the
 * device arrive at drx_plan_finish.  Validation is drx_decode's: the header chain of every chunk is walked and judged, and a
 * payload that ends before its samples do, or whose codes do not end in its last payload word, is DRX_ERR_CORRUPT; the rows
 * are then undefined and the plan stays usable.  DRX_ERR_ARG, with nothing launched and the status word as it was: a NULL pointer.
 *   The buffers rule at the top of this file holds: any 4-byte alignment of d_in and any 8-byte alignment of d_out; exactly
 * 8 * total_waves int64 are written; the result depends neither on what they held before nor on words outside [0, in_words),
 * and no load leaves [0, in_words).
 *   Every prediction filter the plan accepts: the delta filter a lane per waveform that parses as the lane decoder does and
 * reduces in registers; any other filter a lane per waveform in a serial kernel, correct but not fast.  Few long waveforms
 * under the delta filter -- the batches drx_decode gives to its block decoder (DRX_PATH_BLOCKS), on a plan created with that
 * geometry -- take a WORKGROUP per block of a waveform's stream instead: the block decoder's parse, the samples reduced where
 * the decoder would put them in order and write them out, a block's result folded into its waveform's by integer atomics.  A
 * waveform whose block had to correct its start after publishing its end, or whose count or last code does not fit its
 * payload, is computed again and judged by the serial lane kernel: correct and slow, a flagged waveform of 14 M samples costs
 * there what the whole call cost before (50-60 ns per sample); noise and quiet data are never flagged.  Under a general filter
 * few long waveforms stay a lane per waveform.  DRX_DBG_STATS_LANES: never the block form; DRX_DBG_STATS_ALL_FALLBACK: the
 * block form lists every waveform for the lane kernel behind it (tests).  drx_plan_last_decode_path reports DRX_PATH_STATS
 * alone whichever form ran; drx_plan_last_stats_form says which. */
#define DRX_STAT_MIN 0        /* smallest sample                                   */
#define DRX_STAT_ARGMIN 1     /* smallest i with y[i] == MIN                        */
#define DRX_STAT_MAX 2
#define DRX_STAT_ARGMAX 3     /* smallest i with y[i] == MAX                        */
#define DRX_STAT_SUM 4        /* sum of y[i], all i                                 */
#define DRX_STAT_SUMSQ 5      /* sum of y[i]^2                                      */
#define DRX_STAT_HEAD_SUM 6   /* sum of y[i], i < min(head_len, len)                */
#define DRX_STAT_HEAD_SUMSQ 7 /* sum of y[i]^2 over the same window                 */
#define DRX_STAT_COLS 8
drx_status drx_wave_stats(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                          uint32_t head_len, int64_t *d_out);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, not
 * the plan's own table): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_wave_stats_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                          const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words, uint32_t head_len,
                                          int64_t *d_out);

/* Which form the plan's last drx_wave_stats took (0 before its first statistics call) */
#define DRX_STATS_FORM_LANES 1u        /* a lane per waveform */
#define DRX_STATS_FORM_BLOCKS 2u       /* a workgroup per block of a waveform's stream, the lane kernel behind it for listed waveforms */
#define DRX_STATS_FORM_FALLBACK_ALL 4u /* or-ed: DRX_DBG_STATS_ALL_FALLBACK was in force */
uint32_t drx_plan_last_stats_form(const drx_plan *plan);

/* BINNED statistics of every waveform straight from the encoded stream: the sum, the sum of squares, the minimum and the maximum
 * of every stretch of `bin` samples from a per-waveform origin -- the overview of a long trace (min, max and mean per 1/1000 of
 * it; the RMS per time bin of a decaying signal), the charge in gates around a pulse, a baseline that drifts -- without decoding
 * the batch to memory.  drx_wave_stats' two HEAD columns generalised to any number of equal windows.
 *   Bins.  Waveform g (a global waveform index in the order of drx_plan_wave_words) has samples y[0 .. len_g), the int16
 * drx_decode would write.  Its origin is a_g = (d_start ? d_start[g * start_stride] : 0) + offset; the sum saturates at the int64
 * ends, as in drx_decode_window.  d_start: int64 on the device, any 8-byte alignment; start_stride counts int64 elements, so a
 * column of drx_wave_stats' output or of drx_find_pulses' records goes in as it is.  Bin b, 0 <= b < n_bins, holds the samples
 * with index in [a_g + b * bin, a_g + (b + 1) * bin) and in [0, len_g).
 *   Rows.  Row (g, b) is d_out + g * out_wave_stride + b * DRX_BIN_COLS: four int64, the DRX_BIN_* columns.  An empty bin -- one
 * outside the waveform, one beyond the short last waveform of a chunk -- is (0, 0, 32767, -32768), the identities of the four
 * reductions: neighbouring bins merge by add, add, min, max with no special case, and the bins that cover a waveform merge to
 * drx_wave_stats' SUM, SUMSQ, MIN, MAX.  Everything is exact (a waveform has fewer than 2^31 samples).
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: a NULL pointer among d_in, d_chunk_word_off, d_out; bin == 0;
 * start_stride == 0 with d_start != NULL; out_wave_stride < n_bins * DRX_BIN_COLS; in the second form a NULL side-band, or the
 * plan's own table passed as the side-band.  n_bins == 0 returns DRX_OK with nothing launched.
 *   Validation is drx_wave_stats': the header chain of every chunk is walked and judged (the second form checks the table
 * against the stream instead), and EVERY waveform is parsed to its end whatever its bins cover: a payload that ends before its
 * samples do, or whose codes do not end in its last payload word, is DRX_ERR_CORRUPT at drx_plan_finish; the rows are then
 * undefined and the plan stays usable.
 *   The buffers rule at the top of this file holds: any 4-byte alignment of d_in, any 8-byte alignment of d_start and d_out; no
 * load leaves [0, in_words); exactly total_waves x n_bins rows of four int64 are written, nothing between the rows of different
 * waveforms is touched, and the result does not depend on what the rows held before; row addressing is 64-bit.
 *   Asynchronous on the context's stream like drx_wave_stats; the call clears the plan's status word first and ends a pending
 * drx_gather_encoded sizing call's resume; errors found on the device arrive at drx_plan_finish.  drx_plan_last_decode_path
 * reports DRX_PATH_BINS alone whichever form ran (drx_plan_last_bins_form says which), drx_plan_last_timings
 * { header-chain walk, everything behind the walk, 0, whole call }.
 *   Every prediction filter the plan accepts, a lane per waveform: the delta filter parses as drx_wave_stats' lane kernel does
 * and splits a group of 16 samples that holds a bin's end in registers (bins shorter than 16 samples take a sample-at-a-time
 * path: correct, several times slower); any other filter runs a serial kernel, correct but not fast.
 *   Few long waveforms -- the batches drx_wave_stats gives to its block form -- stay a lane per waveform BY DEFAULT, 50-60 ns per
 * sample and lane.  The context option "bins_impl" = 1 (drx_ctx_set_option) gives them a workgroup per block of the waveform's
 * stream instead, under the delta filter: the rows are first set to the identity, the blocks merge their partial rows into them
 * with 64-bit integer atomics (the same answer in any order: the result is exact and reproducible), and the waveforms the blocks
 * flag are written again, every row, and judged by a lane each (drx_plan_last_bins_listed counts them).  The same rows, the same
 * verdicts, the same buffers rule; drx_plan_last_bins_form says which form ran.  Bins of a few samples are correct there and not
 * tuned.  With "bins_impl" 0 drx_plan_last_bins_form says DRX_BINS_FORM_LANES for every batch and DRX_DBG_BINS_LANES and
 * DRX_DBG_BINS_ALL_FALLBACK change nothing; with 1 they mean what the other calls' flags mean.  (The block form is an option and
 * not the default because the form word of a default call is part of what the tests pin; making it the default is a follow-up.) */
#define DRX_BIN_SUM 0     /* sum of y[i] over the bin                     */
#define DRX_BIN_SUMSQ 1   /* sum of y[i]^2                                */
#define DRX_BIN_MIN 2     /* smallest sample;  32767 for an empty bin     */
#define DRX_BIN_MAX 3     /* largest sample;  -32768 for an empty bin     */
#define DRX_BIN_COLS 4
drx_status drx_wave_bins(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                         const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t bin, uint32_t n_bins,
                         int64_t *d_out, uint64_t out_wave_stride);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, not
 * the plan's own table): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_wave_bins_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                         const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_stride,
                                         int64_t offset, uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride);
/* which form the plan's last drx_wave_bins took (0: none yet) */
#define DRX_BINS_FORM_LANES 1u        /* a lane per waveform */
#define DRX_BINS_FORM_BLOCKS 2u       /* a workgroup per block of a waveform's stream ("bins_impl" 1) */
#define DRX_BINS_FORM_FALLBACK_ALL 4u /* or-ed: DRX_DBG_BINS_ALL_FALLBACK was in force */
uint32_t drx_plan_last_bins_form(const drx_plan *plan);
/* ... and, behind drx_plan_finish while drx_plan_last_decode_path is DRX_PATH_BINS, how many waveforms a block form handed to
 * the lane kernel behind the blocks, as drx_plan_last_windows_listed; 0 for the lane form */
uint32_t drx_plan_last_bins_listed(const drx_plan *plan);

/* The STACK of selected, aligned waveforms straight from the encoded stream: per position, how many waveforms have a sample
 * there, the sum of those samples and the sum of their squares -- the average pulse (the template of pulse-shape fits, optimal
 * filters and pile-up models) and its per-sample variance, over the waveforms that passed the cuts, aligned on the trigger or on
 * the maximum -- without decoding the batch to memory and with no temporary larger than the result.  The first stream call that
 * reduces ACROSS waveforms.
 *   Contributions.  Waveform g (a global waveform index in the order of drx_plan_wave_words) has samples y[0 .. len_g), the int16
 * drx_decode would write.  Its origin is a_g = (d_start ? d_start[g * start_stride] : 0) + offset; the sum saturates at the int64
 * ends, as in drx_decode_window.  d_start is drx_wave_bins': int64 on the device, any 8-byte alignment, start_stride in int64
 * elements, so a column of drx_wave_stats' output or of drx_find_pulses' records goes in as it is.  Waveform g is selected when
 * d_select == NULL or d_select[g] != 0; d_select: uint8[total_waves] on the device, any alignment.  Position j, 0 <= j < width,
 * receives y[a_g + j] from every selected g with 0 <= a_g + j < len_g.
 *   Rows.  Row j is d_out + j * out_stride, out_stride >= DRX_STACK_COLS in int64 elements, any 8-byte alignment of d_out: the
 * three DRX_STACK_* columns over those contributions, exact.  A position nobody reaches is (0, 0, 0).  Exactly `width` rows are
 * written and nothing between them is touched; the result does not depend on what the rows held before (the call sets them
 * itself), and it is the same in any execution order, because the adds are integer adds.  Outputs of several batches or several
 * GPUs add.  Row addressing is 64-bit.
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: a NULL pointer among d_in, d_chunk_word_off, d_out;
 * start_stride == 0 with d_start != NULL; out_stride < DRX_STACK_COLS; in the second form a NULL side-band, or the plan's own
 * table passed as the side-band.  width == 0 returns DRX_OK with nothing launched.
 *   Validation and trust are drx_decode_window's.  The header chain of every chunk is walked and judged (the second form checks
 * the table against the stream instead).  A selected waveform is parsed no further than the last code of its window, a waveform
 * that is not selected is not parsed at all, and neither the result nor the verdict depends on bits that were not parsed.  A
 * window that reaches the waveform's last sample makes the end-of-payload check; a payload that runs out before the window does
 * is DRX_ERR_CORRUPT at drx_plan_finish, the rows are then undefined and the plan stays usable.  No store's address depends on
 * the stream.
 *   Asynchronous on the context's stream like drx_wave_stats; the call clears the plan's status word first and ends a pending
 * drx_gather_encoded sizing call's resume; errors found on the device arrive at drx_plan_finish.  drx_plan_last_decode_path
 * reports DRX_PATH_STACK alone, drx_plan_last_timings { header-chain walk, everything behind the walk, 0, whole call }.
 *   Every prediction filter the plan accepts, uniform and ragged plans.  Under the delta filter a lane per waveform parses, in
 * persistent workgroups that keep the sums of a tile of positions (512, or 7168) in LDS across many waveforms and add them to
 * the rows once, with 64-bit integer atomics; COUNT comes from the geometry alone; under a selection the lanes take a list of
 * the selected waveforms (8 bytes per waveform of plan scratch, allocated by the first such call).  What is slow: any other filter runs a serial
 * kernel that adds every sample to its row by atomics, correct and not tuned; and few long waveforms (the reference's default of
 * one waveform per chunk) stay a lane per waveform, 50-60 ns per sample and lane, parsed once per tile of 7168 positions, until
 * a block form exists.  A width far beyond the reach of every window costs what its rows cost -- every tile of positions is
 * launched and COUNT's scan is one workgroup over all `width` cells: seconds at the 2^32 - 1 the type allows. */
#define DRX_STACK_COUNT 0   /* selected waveforms that have a sample at this position */
#define DRX_STACK_SUM   1   /* sum of those samples                                   */
#define DRX_STACK_SUMSQ 2   /* sum of their squares                                   */
#define DRX_STACK_COLS  3
drx_status drx_wave_stack(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                          const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width,
                          const uint8_t *d_select, int64_t *d_out, uint64_t out_stride);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, not
 * the plan's own table): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_wave_stack_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                          const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_stride,
                                          int64_t offset, uint32_t width, const uint8_t *d_select, int64_t *d_out,
                                          uint64_t out_stride);

/* A WINDOW of every waveform, at per-waveform offsets, straight from the encoded stream: the samples around a pulse that
 * drx_wave_stats found, or the first few hundred samples of each waveform, without decoding the batch to memory and -- unlike
 * every other stream call -- without reading a payload beyond its window.
 *   The window.  Waveform g (a global waveform index in the order of drx_plan_wave_words) has a window that starts at sample
 * a_g = (d_start ? d_start[g * start_stride] : 0) + offset; the sum saturates.  d_start: int64 on the device, any 8-byte
 * alignment; start_stride counts int64 elements, so a column of drx_wave_stats' [total_waves][8] output is passed as it is,
 * with stride 8: no host round trip lies between the statistics and the windows.
 *   The output row.  Row g is d_out + g * out_stride_samples and receives exactly `width` samples: y[a_g + j] where
 * 0 <= a_g + j < len_g (the int16 drx_decode would write there), and `pad` elsewhere.  A window entirely outside the waveform is
 * a row of pad; the short last waveform of a chunk is a row like any other; the samples between rows keep what they held.
 *   Asynchronous on the context's stream like drx_decode; the call clears the plan's status word first and ends a pending
 * drx_gather_encoded sizing call's resume; errors found on the device arrive at drx_plan_finish.  drx_plan_last_decode_path
 * reports DRX_PATH_WINDOW alone, drx_plan_last_timings { header-chain walk, window kernel, 0, whole call }.
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: a NULL pointer among d_in, d_chunk_word_off, d_out; a NULL
 * side-band in the second form, or the plan's own table passed as the side-band; out_stride_samples < width; start_stride == 0
 * with d_start != NULL.  width == 0 returns DRX_OK with nothing launched.
 *   Validation and trust.  The header chain of every chunk is walked and judged as drx_decode does (the second form checks the
 * table against the stream instead).  A lane parses no further than the last code of its window: neither the result nor the
 * verdict depends on payload bits behind it.  A lane whose window reaches its waveform's last sample makes drx_wave_stats'
 * end-of-payload check; a payload that runs out of words before the window's codes do is DRX_ERR_CORRUPT.  After a corrupt
 * verdict the rows are undefined and the plan stays usable.
 *   The buffers rule at the top of this file holds: any 4-byte alignment of d_in, any 2-byte alignment of d_out and any stride
 * >= width; no load leaves [0, in_words); nothing is written outside the total_waves rows of width samples; row addressing is
 * 64-bit (g * out_stride_samples may exceed 2^32 bytes).
 *   Every prediction filter the plan accepts: the delta filter a lane per waveform that parses as the lane decoder does and
 * writes its own row; any other filter a lane per waveform in a serial kernel that stops at the window's end, correct but not
 * fast.  Few long waveforms go through the same lane-per-waveform kernels, 50-60 ns per sample and lane (correct, slow): for
 * such batches drx_decode_windows with n_win = 1 is the fast form, a workgroup per block of a waveform's stream. */
drx_status drx_decode_window(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width, int16_t pad,
                             int16_t *d_out, uint64_t out_stride_samples);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, not
 * the plan's own table): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_decode_window_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                             const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words, const int64_t *d_start,
                                             uint64_t start_stride, int64_t offset, uint32_t width, int16_t pad, int16_t *d_out,
                                             uint64_t out_stride_samples);

/* SEVERAL WINDOWS of every waveform, at per-window starts, straight from the encoded stream: the samples around EVERY pulse
 * that drx_find_pulses found, its records taken as it writes them -- no host round trip, no reshaping, and the batch is not
 * decoded to memory.
 *   The windows.  Waveform g (a global waveform index in the order of drx_plan_wave_words) has window slots p = 0 .. n_win - 1.
 * Slot p is LIVE when p < min(d_count[g], n_win); d_count == NULL: every slot is live.  d_count: uint32[total_waves] on the device,
 * any 4-byte alignment -- drx_find_pulses' count as written, which may exceed max_pulses: the min handles that.  A live window
 * starts at a = d_start[g * start_wave_stride + p * start_win_stride] + offset; the sum saturates at the int64 ends, as in
 * drx_decode_window.  d_start: int64 on the device, any 8-byte alignment; both strides count int64 elements.  The DRX_PULSE_START
 * or DRX_PULSE_ARGPEAK column of drx_find_pulses' [total_waves][max_pulses][DRX_PULSE_COLS] output goes in as it is: the pointer is
 * d_pulses + column, the strides are DRX_PULSE_COLS * max_pulses and DRX_PULSE_COLS.
 *   The rows.  Row (g, p) is d_out + g * out_wave_stride + p * out_win_stride and receives exactly `width` samples.  A live row
 * holds y[a + j] where 0 <= a + j < len_g (the int16 drx_decode would write there) and `pad` elsewhere; a row that is not live is
 * all pad; the samples between rows keep what they held.  Row addressing is 64-bit.
 *   Order and overlap.  The live windows of a waveform may come in any order and may overlap, nest or coincide: every row is what
 * it would be alone.  Non-decreasing starts, as drx_find_pulses numbers its pulses, are the fast case: the lane kernel then keeps
 * a cursor, and a group of 16 samples that touches no window costs one compare.  An unsorted list costs a scan of all live
 * windows of the waveform per group of 16 samples.
 *   Extent and verdict.  Let e_g be the largest min(a + width, len_g) over the live windows of g, or 0 when no window holds a
 * sample.  Neither the rows nor the verdict depend on payload bits behind sample e_g.  A waveform with e_g == len_g gets
 * drx_wave_stats' end-of-payload check; a payload that runs out of words before the windows' codes do is DRX_ERR_CORRUPT.  The
 * header chain of every chunk is walked and judged as drx_decode does (the second form checks the table against the stream
 * instead).  After a corrupt verdict the rows are undefined and the plan stays usable.  All of this holds in every form.
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: a NULL pointer among d_in, d_chunk_word_off, d_start, d_out;
 * start_wave_stride == 0 or start_win_stride == 0; out_win_stride < width; out_wave_stride < (n_win - 1) * out_win_stride + width
 * (rows would overlap); in the second form a NULL side-band, or the plan's own table passed as the side-band.  width == 0 or
 * n_win == 0 returns DRX_OK with nothing launched.
 *   Asynchronous on the context's stream like drx_decode_window; the call clears the plan's status word first and ends a pending
 * drx_gather_encoded sizing call's resume; errors found on the device arrive at drx_plan_finish.  drx_plan_last_decode_path
 * reports DRX_PATH_WINDOWS alone whichever form ran (drx_plan_last_windows_form says which), drx_plan_last_timings
 * { header-chain walk, everything between the walk and the call's end, 0, whole call }.
 *   The buffers rule at the top of this file holds: any 4-byte alignment of d_in, any 2-byte alignment of d_out; no load leaves
 * [0, in_words); nothing is written outside the total_waves x n_win rows of width samples, and the result does not depend on what
 * the rows held before.
 *   Every prediction filter the plan accepts, a lane per waveform: the delta filter in drx_decode_window's lane kernel with a
 * window list (a lane ends behind e_g), any other filter in a serial kernel that loops over the live windows per sample, correct
 * but not fast.  Few long waveforms under the delta filter -- the batches drx_wave_stats gives to its block form -- take a block
 * form: a workgroup per block of a waveform's stream parses as the block decoder does, and puts its samples in order and stores
 * them only where a live window meets the block, so sparse windows cost the parse alone and a window deep in a long trace does
 * not cost a lane the whole trace in front of it.  A waveform that the block parse flags, or whose payload fails the blocks'
 * end-of-payload check (they parse every waveform to its end), has all its rows written again and is judged, to e_g, by the lane
 * kernel over a list: a waveform damaged only behind its last window ends with the lane form's verdict.  The list's scratch
 * belongs to the plan and is allocated by the first call of this form.  The results of all forms are the same bit for bit.
 * DRX_DBG_WINDOWS_LANES: never the block form; DRX_DBG_WINDOWS_ALL_FALLBACK: the block form lists every waveform for the lane
 * kernel behind it; DRX_DBG_NO_LONG_PATHS and DRX_DBG_LONG_NOT_BLOCKS keep the call on lanes as they do for statistics and pulses.
 *   One window of short waveforms: drx_decode_window's kernel stores whole dwords at either row parity and is the one to prefer
 * there (DESIGN.md section 4.2j has the measured rows). */
drx_status drx_decode_windows(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const int64_t *d_start, uint64_t start_wave_stride, uint64_t start_win_stride, const uint32_t *d_count,
                              uint32_t n_win, int64_t offset, uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_wave_stride,
                              uint64_t out_win_stride);
/* which form the plan's last drx_decode_windows took (0: none yet) */
#define DRX_WINDOWS_FORM_LANES 1u        /* a lane per waveform */
#define DRX_WINDOWS_FORM_BLOCKS 2u       /* a workgroup per block of a waveform's stream, the lane kernel behind it for listed waveforms */
#define DRX_WINDOWS_FORM_FALLBACK_ALL 4u /* or-ed: DRX_DBG_WINDOWS_ALL_FALLBACK was in force */
uint32_t drx_plan_last_windows_form(const drx_plan *plan);
/* ... and, behind drx_plan_finish while drx_plan_last_decode_path is DRX_PATH_WINDOWS, how many waveforms its block form handed
 * to the lane kernel behind the blocks (flagged or judged suspect by the block parse, or all of them under
 * DRX_DBG_WINDOWS_ALL_FALLBACK): their rows were written again, all of them, and judged there; 0 for the lane form */
uint32_t drx_plan_last_windows_listed(const drx_plan *plan);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, not
 * the plan's own table): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_decode_windows_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                              const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words, const int64_t *d_start,
                                              uint64_t start_wave_stride, uint64_t start_win_stride, const uint32_t *d_count,
                                              uint32_t n_win, int64_t offset, uint32_t width, int16_t pad, int16_t *d_out,
                                              uint64_t out_wave_stride, uint64_t out_win_stride);

/* EVERY PULSE of every waveform, straight from the encoded stream: threshold discrimination -- time over threshold, the number
 * of pulses, and the start, width, peak and integral of each -- without decoding the batch to memory.  What drx_wave_stats (one
 * maximum per waveform) and drx_decode_window (one start per waveform) cannot say of a waveform with two pulses, of a noise
 * spike beside a wide lower pulse, or of a long trace that holds many events.
 *   The threshold.  Waveform g (a global waveform index in the order of drx_plan_wave_words) has the samples y[0 .. len_g), the
 * int16 drx_decode would write, and the threshold t_g = (d_thr ? d_thr[g * thr_stride] : 0) + thr; the sum saturates at the
 * int64 ends.  d_thr: int64 on the device, any 8-byte alignment; thr_stride counts int64 elements, so a column of
 * drx_wave_stats' output, or any expression over it, goes in with no host round trip, as drx_decode_window takes its starts.
 *   A pulse.  Sample i is OVER when polarity > 0 and y[i] > t_g, or polarity < 0 and y[i] < t_g (strictly, both).  A run is a
 * maximal range [s, e) of consecutive over samples; it may begin at sample 0, and one still open at the waveform's last sample
 * ends there, e = len_g.  A pulse is a run with e - s >= min_width; pulses are numbered by s.
 *   The output.  d_count[g] (uint32[total_waves]) receives the number of pulses of waveform g -- all of them, those beyond
 * max_pulses included, so a row that overflowed shows.  d_out is int64[total_waves][max_pulses][DRX_PULSE_COLS]: slot
 * p < min(count_g, max_pulses) holds pulse p, every other slot is all zero.  PEAK is the run's maximum for positive polarity and
 * its minimum for negative, ARGPEAK its first occurrence.  Everything is exact: a waveform has fewer than 2^31 samples, so SUM
 * fits an int64.  max_pulses == 0 is the counting form: only d_count is written and d_out may be NULL.
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: a NULL pointer among d_in, d_chunk_word_off, d_count;
 * d_out == NULL with max_pulses > 0; polarity == 0; min_width == 0; thr_stride == 0 with d_thr != NULL; in the second form a NULL
 * side-band, or the plan's own table passed as the side-band.
 *   Asynchronous on the context's stream like drx_decode; the call clears the plan's status word first and ends a pending
 * drx_gather_encoded sizing call's resume; errors found on the device arrive at drx_plan_finish.  drx_plan_last_decode_path
 * reports DRX_PATH_PULSES alone whichever form ran (drx_plan_last_pulses_form says which), drx_plan_last_timings
 * { header-chain walk, memset and pulse kernels (block form: blocks, stitch and fallback), 0, whole call }.
 *   Validation is drx_wave_stats': the header chain of every chunk is walked and judged (the second form checks the table
 * against the stream instead), and a payload that ends before its samples do, or whose codes do not end in its last payload
 * word, is DRX_ERR_CORRUPT; the outputs are then undefined and the plan stays usable.
 *   The buffers rule at the top of this file holds: any 4-byte alignment of d_in and d_count, any 8-byte alignment of d_thr and
 * d_out; no load leaves [0, in_words); exactly total_waves counts and total_waves * max_pulses * DRX_PULSE_COLS int64 are
 * written, and the result does not depend on what they held before; slot addressing is 64-bit.
 *   Every prediction filter the plan accepts: the delta filter a lane per waveform that parses as drx_wave_stats' lane kernel
 * does and keeps a small state machine (a group of 16 samples that holds nothing over the threshold costs one packed maximum
 * and one compare); any other filter a lane per waveform in a serial kernel, correct but not fast.
 *   Few long waveforms under the delta filter -- the batches drx_wave_stats gives to its block form, a long trace that holds
 * many events among them -- take a block form: a workgroup per block of a waveform's stream parses as the block decoder does,
 * finds the pulses that lie inside its block and publishes the runs that touch the block's first and last sample; a pass behind
 * the blocks joins those runs across the borders, numbers every waveform's pulses by their start and fills the slots.  A block
 * stages the records of at most min(max_pulses, DRX_PULSES_STAGE_CAP) of its own pulses (the staging buffer belongs to the plan:
 * allocated by the first call of this form, grown when a later call asks for more pulses).  A waveform of which a block holds
 * more pulses than that AND needs more than that many of them among its first max_pulses is finished by a second launch of the
 * blocks over such waveforms alone: by then the pass behind the first launch has numbered every block's pulses, and the blocks
 * write them straight to their slots.  The call then costs the blocks twice for those waveforms, not a lane per waveform
 * (measured with one such waveform among 2048 of 500 000 samples: 1.67 ms against 1.32 without one, 24.1 a lane per waveform).
 * Calls with max_pulses <= DRX_PULSES_STAGE_CAP, and the counting form, never need it and do not launch it.  A waveform that
 * the block parse flags (a stream whose blocks do not fall into step) is computed again by the delta filter's lane kernel over
 * a list, exact, at 48 ns per sample: noise and quiet data are never flagged.
 * drx_plan_last_pulses_redone and drx_plan_last_pulses_listed say how many waveforms of the last call went either way.  The
 * results of all forms are the same bit for bit.  DRX_DBG_PULSES_LANES: never the block form; DRX_DBG_PULSES_ALL_FALLBACK: the
 * block form hands every waveform to the lane kernel behind it. */
#define DRX_PULSE_START 0   /* first sample of the run, waveform-relative               */
#define DRX_PULSE_WIDTH 1   /* samples in the run (time over threshold)                  */
#define DRX_PULSE_PEAK 2    /* the extreme sample of the run in the polarity's direction */
#define DRX_PULSE_ARGPEAK 3 /* smallest waveform-relative i with y[i] == PEAK            */
#define DRX_PULSE_SUM 4     /* sum of y[i] over the run                                  */
#define DRX_PULSE_COLS 5
drx_status drx_find_pulses(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                           const int64_t *d_thr, uint64_t thr_stride, int64_t thr, int32_t polarity, uint32_t min_width,
                           uint32_t max_pulses, uint32_t *d_count, int64_t *d_out);
/* which form the plan's last drx_find_pulses took (0: none yet) */
#define DRX_PULSES_FORM_LANES 1u        /* a lane per waveform */
#define DRX_PULSES_FORM_BLOCKS 2u       /* a workgroup per block of a waveform's stream, the stitch behind them */
#define DRX_PULSES_FORM_FALLBACK_ALL 4u /* or-ed: DRX_DBG_PULSES_ALL_FALLBACK was in force */
uint32_t drx_plan_last_pulses_form(const drx_plan *plan);
#define DRX_PULSES_STAGE_CAP 8u /* records a block of the block form stages at most */
/* ... and, behind drx_plan_finish, how many waveforms its block form handed to the lane kernel behind the stitch (flagged by the
 * block parse, or all of them under DRX_DBG_PULSES_ALL_FALLBACK), and how many its second launch of the blocks finished
 * (short of staged records); both 0 for the lane form */
uint32_t drx_plan_last_pulses_listed(const drx_plan *plan);
uint32_t drx_plan_last_pulses_redone(const drx_plan *plan);
/* ... with the encoder's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, not
 * the plan's own table): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_find_pulses_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                           const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words, const int64_t *d_thr,
                                           uint64_t thr_stride, int64_t thr, int32_t polarity, uint32_t min_width,
                                           uint32_t max_pulses, uint32_t *d_count, int64_t *d_out);

/* RE-CODE an encoded batch to another RiceParameter, without decoding it.  Under a fixed prediction filter the codes of one
 * sample at any two RiceParameters carry the same zig-zag value (src/deltaRice.c:207-228), so the stream is parsed, sized, scanned
 * and packed on residuals: no filter arithmetic, no sample in memory, and every prediction filter the plan accepts -- more than
 * four taps and leads other than +-1 included -- takes the same kernels.  The plan describes the SOURCE (geometry, filter, its
 * RiceParameter 2^k); the result is a batch of the same geometry and filter coded at 2^new_rice_k, framed as drx_encode frames it:
 * N_c | { n_i' | payload_i' }, chunks back to back from d_out[0]; d_out_chunk_word_off (uint64[n_chunks + 1]) is written as
 * drx_encode writes it (last entry = total words); d_out_wave_words (uint32[total_waves], or NULL) receives every n_i': the
 * side-band of the result.
 *   Every residual is the int16 the decoders take from its code, in canonical form: an ordinary code whose value exceeds 65535
 * (possible from k = 13 on in a foreign stream) folds as drx_decode folds it, an escape that holds a small value comes out as an
 * ordinary code.  Hence, for a filter with lead +-1, the output is byte for byte drx_encode of the decoded samples at the new
 * parameter -- what the reference's filter gives; for every filter it decodes, under the new parameter, to exactly what the input
 * decodes to under the old.  new_rice_k equal to the plan's own is allowed: a canonical stream comes back word for word.
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: new_rice_k > 15, a NULL pointer among d_in,
 * d_chunk_word_off, d_out_chunk_word_off, d_out == NULL with a capacity.
 *   Sizing, as in drx_gather_encoded: d_out == NULL (with out_cap_words == 0) runs as far as the offsets: both tables are written,
 * drx_plan_finish reports the total, nothing else is touched.  With d_out != NULL and a total above out_cap_words:
 * DRX_ERR_CAPACITY at drx_plan_finish, which still reports the total NEEDED, and not one word of d_out is written.
 * drx_plan_max_encoded_words bounds any result.  The call behind a sizing call starts anew (no resume), so a caller that has a
 * bound does better to pass a buffer of that size.
 *   Asynchronous on the context's stream like drx_decode; the call clears the plan's status word first, errors found on the
 * device arrive at drx_plan_finish.  Validation is drx_wave_stats's: the header chain of every chunk is walked and judged, and a
 * payload that ends before its samples do, or whose codes do not end in its last payload word, is DRX_ERR_CORRUPT; then no word
 * of d_out is written, the tables are undefined and the plan stays usable.  drx_plan_wave_words / drx_plan_wave_word_off
 * describe the SOURCE after the call, as after a decode; the result's n_i' and header positions live in scratch of their own that
 * belongs to the plan (allocated by the first such call).  The plan's RiceParameter does not change.  A pending
 * drx_gather_encoded sizing call's resume is ended.  drx_plan_last_decode_path reports DRX_PATH_TRANSCODE alone.
 *   The buffers rule at the top of this file holds: any 4-byte alignment of d_in and d_out, any alignment of their element type
 * for both tables; nothing is written outside [d_out, d_out + total), the n_chunks + 1 offsets and the total_waves table entries;
 * no load leaves [0, in_words); the result does not depend on what the outputs held before.  d_out must not overlap d_in (not
 * checked).
 *   Few long waveforms -- the batches drx_wave_stats gives to its block form, here under EVERY prediction filter the plan
 * accepts, since a re-code has no filter arithmetic -- take a workgroup per block of a waveform's stream, twice: a sizes launch
 * (the block decoder's parse on residuals; a block adds the code lengths of its samples at the new parameter and leaves its bit
 * count, where its first code starts, its first sample's index and its sample count in a table of the plan), a kernel that
 * turns every waveform's bit counts into n_i' and bit offsets or lists the waveform for the lane kernels (flagged and suspect
 * waveforms, waveforms with samples and no payload word), the lane kernels over that list for their n_i' and their verdict, the
 * scan, then a pack launch in which every block re-codes its samples to its own bit position from the table alone -- no block
 * waits for another there, so the result does not depend on which waveforms a launch flagged -- and the lane pack kernel over the
 * list.  Words that two blocks share are OR-ed into words a kernel of this call has cleared, inside [d_out, d_out + total) and
 * under no error only.  All forms give the same words, tables and verdicts bit for bit.  drx_plan_last_decode_path reports
 * DRX_PATH_TRANSCODE alone whichever form ran (drx_plan_last_transcode_form says which), drx_plan_last_timings keeps its four
 * entries.  DRX_DBG_TRANSCODE_LANES: never the block form; DRX_DBG_TRANSCODE_ALL_FALLBACK: the block form lists every waveform. */
drx_status drx_transcode(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                         uint32_t new_rice_k, uint32_t *d_out, uint64_t out_cap_words, uint64_t *d_out_chunk_word_off,
                         uint32_t *d_out_wave_words);
/* ... with the SOURCE's side-band as drx_decode_with_wave_words takes it (d_wave_words: uint32[total_waves] on the device, neither
 * the plan's own table nor d_out_wave_words): no walk; a table that does not belong to the stream is DRX_ERR_CORRUPT. */
drx_status drx_transcode_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                         const uint32_t *d_wave_words, uint32_t new_rice_k, uint32_t *d_out, uint64_t out_cap_words,
                                         uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words);
/* Re-coding under ANOTHER PREDICTION FILTER as well, still without decoding to memory: d_out receives, byte for byte, what
 * drx_encode writes under the filter new_taps at RiceParameter 2^new_rice_k for the samples drx_decode produces from d_in under the
 * plan's filter and RiceParameter (in the reference's terms: every chunk decoded with the source's options, encoded with the
 * target's, the chunks laid back to back).  The plan describes the SOURCE -- geometry, filter, RiceParameter -- and neither its
 * filter nor its RiceParameter changes.  new_taps: a HOST array of new_n_taps values, 1 <= new_n_taps <= DRX_MAX_TAPS,
 * new_taps[0] != 0, consumed before the call returns; {1, -1} is the delta filter.  A source whose lead is not +-1 decodes with
 * the reference's division towards zero; the result is the encode of those samples, whatever they are.
 *   Everything else is drx_transcode's: the framing, both output tables, the sizing call (d_out == NULL, capacity 0),
 * DRX_ERR_CAPACITY at drx_plan_finish with the total needed and not one word written, drx_wave_stats's validation,
 * DRX_ERR_CORRUPT with d_out untouched, the buffers rule (any 4-byte alignment, every output word stored exactly once, no load
 * outside [0, in_words)), the end of a pending gather resume, DRX_PATH_TRANSCODE reported alone, and drx_plan_last_timings'
 * { walk, sizes + scan + offsets, pack, total }.
 *   DRX_ERR_ARG, with nothing launched and the status word as it was: new_n_taps of 0 or above DRX_MAX_TAPS, new_taps NULL,
 * new_taps[0] == 0, new_rice_k > 15, and drx_transcode's NULL-pointer cases.
 *   Kernels.  A source that is the delta filter or has at most 4 taps with lead +-1, and a target of at most 4 taps with any
 * non-zero lead, take the fast pair: drx_transcode's lane kernels with three samples of history in registers and the two filters
 * as multiply-adds mod 2^16 between the parse and the sink.  Every other pair takes the serial pair (a lane per waveform, global
 * loads, the last 64 samples in LDS; correct, not tuned); DRX_DBG_REFILTER_SERIAL sends every pair there.  Both give the same
 * words, tables and verdicts bit for bit.
 *   ALWAYS a lane per waveform: drx_transcode's block form works on residuals and has no samples at a block's start, so a plan
 * whose geometry takes the block form for drx_transcode takes these lane kernels for a re-filter (the form word is
 * LANES | REFILTER, never BLOCKS).  A waveform of millions of samples in one lane is slow; how slow has not been measured.
 *   Cost (profiles/refilter_notes.md): SLOWER than the route it replaces.  On 1 M waveforms of 7000 samples, delta at m = 8 to
 * {1, -1, 1, -1} at m = 8: 21.2 ms, where drx_decode + drx_plan_set_filter + drx_encode + drx_plan_set_filter back take 13.4 ms.
 * What it saves is the decoded intermediate (14 GB there: 7.4 GB of peak device memory above the source instead of 21.4 GB) and
 * a plan that is never re-filtered (drx_plan_set_filter waits for the stream). */
drx_status drx_transcode_filter(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                uint32_t new_rice_k, uint32_t new_n_taps, const int32_t *new_taps, uint32_t *d_out,
                                uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words);
/* ... with the SOURCE's side-band, as drx_transcode_with_wave_words takes it */
drx_status drx_transcode_filter_with_wave_words(drx_plan *plan, const uint32_t *d_in, uint64_t in_words,
                                                const uint64_t *d_chunk_word_off, const uint32_t *d_wave_words, uint32_t new_rice_k,
                                                uint32_t new_n_taps, const int32_t *new_taps, uint32_t *d_out, uint64_t out_cap_words,
                                                uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words);
/* Which form the plan's last drx_transcode / drx_transcode_filter (the sizing calls included), drx_estimate_words_encoded or
 * drx_estimate_words_encoded_filter took; 0 before the first */
#define DRX_TRANSCODE_FORM_LANES 1u        /* a lane per waveform */
#define DRX_TRANSCODE_FORM_BLOCKS 2u       /* a workgroup per block of a waveform's stream, the lane kernels behind it for listed waveforms */
#define DRX_TRANSCODE_FORM_FALLBACK_ALL 4u /* or-ed: DRX_DBG_TRANSCODE_ALL_FALLBACK was in force */
#define DRX_TRANSCODE_FORM_REFILTER 8u     /* or-ed: the call changed the prediction filter (drx_transcode_filter, drx_estimate_words_encoded_filter) */
#define DRX_TRANSCODE_FORM_REFILTER_SERIAL 16u /* or-ed: ... and its serial kernels ran */
uint32_t drx_plan_last_transcode_form(const drx_plan *plan);
/* ... and, valid behind drx_plan_finish, how many waveforms its block form handed to the lane kernels (flagged or suspect
 * waveforms, waveforms with samples and no payload word, all of them under DRX_DBG_TRANSCODE_ALL_FALLBACK); 0 for the lane form */
uint32_t drx_plan_last_transcode_listed(const drx_plan *plan);
/* drx_estimate_words' sixteen numbers from the STREAM: words_out[k] (host array of 16) is the total words drx_transcode would
 * produce at new_rice_k = k; the plan's filter enters only through the stream.  For a canonical stream the entry at the plan's
 * own k is the stream's total words.  d_wave_words: the source's side-band, or NULL to walk.  SYNCHRONOUS: it clears the status
 * word as a decode does, waits, and returns the verdict itself (a stream that fails drx_transcode's validation:
 * DRX_ERR_CORRUPT, words_out undefined).  Few long waveforms take drx_transcode's block form: the sizes launch with sixteen
 * counts per block, the lane kernel behind it for the waveforms the blocks list. */
drx_status drx_estimate_words_encoded(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                      const uint32_t *d_wave_words, uint64_t words_out[16]);
/* ... under another prediction filter: words_out[k] is the total words drx_transcode_filter would produce with these taps at
 * new_rice_k = k, headers included, k = 0..15.  d_wave_words: the source's side-band, or NULL to walk.  new_taps as
 * drx_transcode_filter takes them (DRX_ERR_ARG likewise).  SYNCHRONOUS like drx_estimate_words_encoded; the sizes kernels of
 * drx_transcode_filter with sixteen counts per lane. */
drx_status drx_estimate_words_encoded_filter(drx_plan *plan, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                             const uint32_t *d_wave_words, uint32_t new_n_taps, const int32_t *new_taps,
                                             uint64_t words_out[16]);

/* RiceParameter optimiser (docs/Optimization.md:5-19 of the reference describes one, the tree does not
 * contain it): exact number of uint32 words drx_encode would emit for this batch with RiceParameter
 * 2^k, for every k = 0..15 (host array of 16), in one pass over the samples.  Synchronous. */
drx_status drx_estimate_words(drx_plan *plan, const int16_t *d_in, uint64_t words_out[16]);

/* Waits for the plan's last encode/decode, reports device-side errors and (for
 * encode) the number of words produced.  total_words may be NULL.
 *   It reports the plan's LAST encode, decode, select, gather, statistics, transcode, window, windows or pulse call only: every such call (a select or gather of no entries
 * and a window of no width excepted, which launch nothing) starts by clearing the plan's one status word, on the stream, so the device-side error
 * (and the word count) of an earlier call that was never finished is not kept.  drx_estimate_words,
 * drx_plan_read_wave_words and drx_plan_set_filter leave the status word as it is: a finish behind them still reports the
 * encode or decode before them.  A caller
 * that needs the verdict of every call finishes each one before the plan's next.  Calls on OTHER plans of the context do not
 * touch this plan's status.  An error reported here leaves the plan usable: the next call starts clean. */
drx_status drx_plan_finish(drx_plan *plan, uint64_t *total_words);

/* Device-side tables of the last call (valid until the next call on the plan):
 * per-waveform payload word counts n_i and header word offsets.  For tests/tools. */
const uint32_t *drx_plan_wave_words(const drx_plan *plan);
const uint64_t *drx_plan_wave_word_off(const drx_plan *plan);
/* Which decoders the plan's last drx_decode used (for tests and tools): the batch's geometry and filter choose among them. */
#define DRX_PATH_LANES_FUSED 1u /* a lane per waveform, header walk inside the launch */
#define DRX_PATH_LANES 2u       /* a lane per waveform behind a separate walk */
#define DRX_PATH_BLOCKS 4u      /* a workgroup per block of a waveform's stream (few long waveforms) */
#define DRX_PATH_LONG 8u        /* a workgroup per waveform */
#define DRX_PATH_SIMPLE 16u     /* the simple kernel (filters the fast kernels do not take) */
#define DRX_PATH_IIR 32u        /* residuals first, then the general filter's inverse in place, parallel inside a waveform */
#define DRX_PATH_IIR_FUSED 64u  /* the general filter's inverse inside the block decoder: one kernel, samples straight to the output */
#define DRX_PATH_SELECT 128u    /* drx_decode_select: a wavefront (general filters: a lane) per selected waveform; reported alone */
#define DRX_PATH_GATHER 256u    /* drx_gather_encoded: word ranges copied, nothing decoded; reported alone */
#define DRX_PATH_STATS 512u     /* drx_wave_stats: a lane per waveform that parses and reduces; reported alone */
#define DRX_PATH_TRANSCODE 1024u /* drx_transcode / drx_estimate_words_encoded: the stream parsed and re-coded, lanes or blocks; reported alone */
#define DRX_PATH_WINDOW 2048u   /* drx_decode_window: a lane per waveform that parses to its window's end; reported alone */
#define DRX_PATH_PULSES 4096u   /* drx_find_pulses: a lane per waveform that parses and discriminates; reported alone */
#define DRX_PATH_WINDOWS 8192u  /* drx_decode_windows: several windows per waveform, lanes or blocks; reported alone */
#define DRX_PATH_BINS 16384u    /* drx_wave_bins: a lane per waveform that parses and reduces bin by bin; reported alone */
#define DRX_PATH_STACK 32768u   /* drx_wave_stack: lanes that parse and add across waveforms through LDS; reported alone */
uint32_t drx_plan_last_decode_path(const drx_plan *plan);
/* ... and which encoder its last drx_encode used (one value; bench.py names the kernel it prices by this, and the tests
 * hold the dispatch to it: the headline batch must take DRX_ENC_STREAM whatever in_words its decodes were given) */
#define DRX_ENC_TWO_PASS 1u    /* sizes, scan, pack (encode_impl 0; more than four taps) */
#define DRX_ENC_SEGMENTS 2u    /* the two-pass segment encoder (the geometries only it serves) */
#define DRX_ENC_FUSED 3u       /* k_encode_fused: a wavefront per waveform, one pass */
#define DRX_ENC_PIECES 4u      /* k_encode_pieces: runs of short waveforms / segments of long ones */
#define DRX_ENC_STREAM 5u      /* k_encode_stream: persistent, a ring per wavefront, a scanner */
#define DRX_ENC_STREAM_SEGS 6u /* k_encode_stream_segs: the same over segments of long waveforms */
uint32_t drx_plan_last_encode_path(const drx_plan *plan);
/* Limits of the encoders (a launch carries fewer than 2^32 threads).  DRX_ENC_FUSED and DRX_ENC_SEGMENTS give every waveform
 * (the segment encoder: every 8192-sample segment slot too) a wavefront of one launch and take batches of at most 2^26 - 8
 * of them; DRX_ENC_PIECES takes fewer than 2^23 workgroups, DRX_ENC_STREAM fewer than 2^32 - 2^16 waveforms and
 * DRX_ENC_STREAM_SEGS as many tickets.  A batch beyond an encoder's limit is not admitted to it, by default or by a
 * DRX_DBG_FORCE_* flag, and takes the next encoder that admits it; DRX_ENC_TWO_PASS (launched in slices of 2^24
 * waveforms) and drx_estimate_words (several waveforms to a wavefront) have no such limit.  drx_plan_last_encode_path says
 * which encoder ran. */
/* Copies n_i of every waveform to host memory (waits for the stream). */
drx_status drx_plan_read_wave_words(drx_plan *plan, uint32_t *host_out);

/* One chunk, host memory, filter semantics (the H5Z callback body):
 * reverse == 0: in = nbytes of int16 samples -> *out = filtered bytes
 * reverse != 0: in = nbytes of filtered bytes -> *out = int16 samples
 * *out is allocated with malloc() (HDF5's allocator for filter buffers,
 * src/deltaRice.c:412,434); the caller owns it.  `in` is not freed. */
drx_status drx_filter_chunk_host(drx_ctx *ctx, int reverse, size_t cd_nelmts,
                                 const unsigned *cd_values, const void *in, size_t nbytes,
                                 void **out, size_t *out_bytes);

/* Kernel times of the plan's last call, measured with HIP events on the context's
 * stream (needs the context option "profile" = 1 before the call; waits for it).
 *   after drx_encode: ms = { size pass, offset scan, pack pass, whole call }
 *   after drx_decode: ms = { header-chain walk, decode kernel, 0, whole call }
 *   after drx_gather_encoded: ms = { header-chain walk, sizes + scan + offsets, copy, whole call }
 *   after drx_wave_stats: ms = { header-chain walk, statistics kernels (block form: blocks + finish + fallback), 0, whole call }
 *   after drx_wave_bins: ms = { header-chain walk, everything behind the walk, 0, whole call }
 *   after drx_wave_stack: ms = { header-chain walk, everything behind the walk, 0, whole call }
 *   after drx_transcode: ms = { header-chain walk, sizes + scan + offsets, pack, whole call }
 *   after drx_decode_window: ms = { header-chain walk, window kernel, 0, whole call }
 *   after drx_decode_windows: ms = { header-chain walk, everything between the walk and the call's end (block form: pads,
 *     blocks, finish and the lane kernel behind them), 0, whole call }
 *   after drx_find_pulses: ms = { header-chain walk, pulse kernel, 0, whole call }; "pulse kernel" is everything between the
 *     walk and the call's end: the output's memset and the lane kernel, or in the block form the blocks, the stitch and the
 *     lane kernel behind them */
drx_status drx_plan_last_timings(drx_plan *plan, float ms[4]);

/* Tuning / diagnostics.  Returns DRX_ERR_ARG for unknown keys or values.
 *   "profile"      1: bracket the kernels with HIP events (drx_plan_last_timings)
 *   "encode_impl"  2 (default): single pass; one wavefront per waveform runs in the persistent form (wavefronts on their own,
 *                  a scanner workgroup for the prefix sum) wherever the standard geometry applies;
 *                  1: single pass with a look-back per workgroup everywhere (round 3's form);  0: size pass + scan + pack pass
 *   "decode_impl"  variant of the lane-per-waveform decode; each is bit-exact and covered by the parity tests:
 *        8 (default)  behind the parallel header walks where a batch takes them (chunks of 8 ... 8192 waveforms longer than 2048
 *                     samples, whatever their number: 64 chains per chunk are chased at once; few chunks of short waveforms);
 *                     otherwise the header walk inside the launch where the batch is large enough to hide it
 *        7            always behind a separate walk kernel
 *        0            simple kernel (also: general filters the staged kernel does not take)
 *   "bins_impl"    0 (default): drx_wave_bins runs a lane per waveform whatever the batch;
 *                  1: the block form (a workgroup per block of a waveform's stream) for the batches drx_wave_stats gives to its
 *                  block form, a lane per waveform elsewhere; the rows are the same (drx_wave_bins above)
 *   "stack_workgroups"  0 (default): drx_wave_stack's lane kernel runs as many persistent workgroups per tile of positions as
 *                  the chip holds; n >= 1: at most n, each walking more waveforms between two flushes of its sums -- the rows
 *                  are the same; for tests of the periodic flush (one workgroup meets it beyond 65 280 waveforms)
 *   "debug_flags"  DRX_DBG_* bits: dispatch overrides that force an alternative (still bit-exact) path, for tests and A/B timing;
 *                  a forcing flag takes its encoder wherever that encoder can run the batch */
#define DRX_DBG_BINS_LANES 64u                   /* drx_wave_bins under "bins_impl" 1: never the block form */
#define DRX_DBG_BINS_ALL_FALLBACK 128u          /* drx_wave_bins, block form: every waveform is listed for the lane kernel behind the blocks */
#define DRX_DBG_NO_LONG_PATHS 256u              /* never the long-waveform paths (segment encoders, block and long decoders) */
#define DRX_DBG_LONG_NOT_BLOCKS 512u            /* long waveforms: one workgroup per waveform, never the block decoder */
#define DRX_DBG_TRANSCODE_LANES 1024u            /* drx_transcode / drx_estimate_words_encoded: never the block form (a lane per waveform whatever the batch) */
#define DRX_DBG_NO_PARALLEL_WALKS 2048u         /* never the parallel header walks */
#define DRX_DBG_NO_PIECES 4096u                 /* never the pieces encoder nor the segment form by default */
#define DRX_DBG_FORCE_SEGMENTS 8192u            /* the two-pass segment encoder */
#define DRX_DBG_TRANSCODE_ALL_FALLBACK 16384u   /* drx_transcode / drx_estimate_words_encoded, block form: every waveform is listed for the lane kernels behind the blocks */
#define DRX_DBG_FORCE_PIECES 32768u             /* the pieces encoder, also where a wavefront per waveform is the default */
#define DRX_DBG_NO_WIDE_FUSED 65536u            /* never the single-pass encoder's larger-buffer geometries (m above 8) */
#define DRX_DBG_RAGGED_ONE_LANES_LAUNCH 131072u /* ragged batches: one decode launch behind both header walks */
#define DRX_DBG_STREAM_THREE_WGS 262144u        /* the persistent encoders on three workgroups (every wavefront goes around its ring) */
#define DRX_DBG_FORCE_STREAM 524288u            /* the persistent encoder (encode_impl 2) whatever the batch's size and code length */
#define DRX_DBG_REFILTER_SERIAL 1048576u         /* drx_transcode_filter / drx_estimate_words_encoded_filter: the serial kernels also for filter pairs the fast kernels take */
#define DRX_DBG_IIR_SEPARATE 2097152u           /* general filters behind the block decoder: always the separate inverse-filter pass */
#define DRX_DBG_FORCE_STREAM_SEGS 4194304u      /* the persistent encoder's segment form (encode_impl 2, uniform), segments of ~1024 samples */
#define DRX_DBG_WALK_BY_SCAN 8388608u           /* the chunk-wide header walk by reading the whole chunk instead of chasing 64 chains */
#define DRX_DBG_WALK_BY_CHAINS 16777216u        /* the chunk-wide header walk by chains also where the scan form is the default */
#define DRX_DBG_GATHER_OTHER_COPY 33554432u      /* drx_gather_encoded: the copy form the batch's code length does NOT choose (a workgroup per run of entries <-> a wavefront per entry) */
#define DRX_DBG_STATS_LANES 67108864u           /* drx_wave_stats: never the block form (a lane per waveform whatever the batch) */
#define DRX_DBG_STATS_ALL_FALLBACK 134217728u   /* drx_wave_stats, block form: every waveform is listed for the lane kernel behind the blocks */
#define DRX_DBG_PULSES_LANES 268435456u         /* drx_find_pulses: never the block form (a lane per waveform whatever the batch) */
#define DRX_DBG_PULSES_ALL_FALLBACK 536870912u  /* drx_find_pulses, block form: every waveform is listed for the lane kernel behind the stitch */
#define DRX_DBG_WINDOWS_LANES 1073741824u        /* drx_decode_windows: never the block form (a lane per waveform whatever the batch) */
#define DRX_DBG_WINDOWS_ALL_FALLBACK 2147483648u /* drx_decode_windows, block form: every waveform is listed for the lane kernel behind the blocks */
drx_status drx_ctx_set_option(drx_ctx *ctx, const char *key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* DELTARICE_HIP_H */
