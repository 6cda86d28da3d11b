// drx_api_stream.hip -- C ABI glue (drx_api.h): the calls that read the whole batch from the encoded stream -- decode, and
// without decoding it wave_stats, wave_bins, wave_stack, decode_window(s), find_pulses, transcode(_filter), estimate_words_encoded(_filter).  Each checks its pointers
// with stream_call_args(), opens with stream_call_begin() and closes with call_end().  Host code only.
#include "drx_api.h"

using namespace drx;

drx_status drx::decode_launch(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, int16_t *d_out,
                              bool tables_ready, const uint32_t *d_sideband) {
    if (!p || !d_in || !d_chunk_word_off || !d_out) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    // (in_words says nothing about how long a waveform's code is -- it may be, and in bench.py IS, the buffer's capacity; round 4
    // took it for the stream's length for a while and sent the headline batch to k_encode_fused)
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, tables_ready, &c)) return st;
    // (d_blk was allocated with the plan, like d_pw)
    DRX_HIP(ctx, launch_decode(c, d_out, (uint64_t *)p->enc.scan.ptr, ctx->decode_impl, p->dec.d_blk, ctx->side.s ? &ctx->side : nullptr,
                               &p->dec.last_path));
    return call_end(p, p->dec.last_path);
}

// A block form's scratch belongs to the plan and is allocated by the first call that takes that form (BlkFormRule, drx_internal.h)
static hipError_t form_scratch(drx_plan *p, const BlkFormRule &r, drx_plan::BlockForm &f, uint64_t (*bytes)(const Geom &)) {
    return blocks_form_batch(p->G, p->dec.d_blk, r) ? p->mem.once(&f.d, bytes(p->G)) : hipSuccess;
}

// per-waveform statistics from the encoded stream (drx_stats.hip)
static drx_status wave_stats(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint32_t *d_sideband, bool sideband, uint32_t head_len, int64_t *d_out) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "wave_stats", d_in && d_chunk_word_off && d_out, d_sideband, sideband)) return st;
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kStatsForm, p->stats, stats_blocks_scratch_bytes));
    DRX_HIP(ctx, launch_wave_stats(c, p->dec.d_blk, p->stats.d, head_len, d_out, &p->stats.last_form));
    return call_end(p, DRX_PATH_STATS);
}

// binned statistics of every waveform from the encoded stream (drx_bins.hip)
static drx_status wave_bins(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                            const uint32_t *d_sideband, bool sideband, const int64_t *d_start, uint64_t start_stride, int64_t offset,
                            uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "wave_bins", d_in && d_chunk_word_off && d_out, d_sideband, sideband)) return st;
    if (bin == 0) return fail(ctx, DRX_ERR_ARG, "wave_bins: bin 0");
    if (d_start && start_stride == 0) return fail(ctx, DRX_ERR_ARG, "wave_bins: start_stride 0");
    if (out_wave_stride < (uint64_t)n_bins * DRX_BIN_COLS)
        return fail(ctx, DRX_ERR_ARG, "wave_bins: waveforms %llu int64 apart do not hold %u rows", (unsigned long long)out_wave_stride, n_bins);
    if (n_bins == 0) return DRX_OK;  // (no row to write: nothing to launch)
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    if (ctx->bins_impl == 1) DRX_HIP(ctx, form_scratch(p, kBinsForm, p->bins, bins_blocks_scratch_bytes));
    DRX_HIP(ctx, launch_wave_bins(c, p->dec.d_blk, p->bins.d, ctx->bins_impl, d_start, start_stride, offset, bin, n_bins, d_out, out_wave_stride,
                                  &p->bins.last_form));
    return call_end(p, DRX_PATH_BINS);
}

// a window of every waveform, at per-waveform offsets (drx_window.hip)
static drx_status decode_window(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                const uint32_t *d_sideband, bool sideband, const int64_t *d_start, uint64_t start_stride,
                                int64_t offset, uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "decode_window", d_in && d_chunk_word_off && d_out, d_sideband, sideband)) return st;
    if (out_stride < width)
        return fail(ctx, DRX_ERR_ARG, "decode_window: rows %llu samples apart do not hold %u", (unsigned long long)out_stride, width);
    if (d_start && start_stride == 0) return fail(ctx, DRX_ERR_ARG, "decode_window: start_stride 0");
    if (width == 0) return DRX_OK;  // (no row receives a sample: nothing to launch)
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, launch_decode_window(c, d_start, start_stride, offset, width, pad, d_out, out_stride));
    return call_end(p, DRX_PATH_WINDOW);
}

// the sum of selected, aligned waveforms (drx_stack.hip)
static drx_status wave_stack(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint32_t *d_sideband, bool sideband, const int64_t *d_start, uint64_t start_stride, int64_t offset,
                             uint32_t width, const uint8_t *d_select, int64_t *d_out, uint64_t out_stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "wave_stack", d_in && d_chunk_word_off && d_out, d_sideband, sideband)) return st;
    if (d_start && start_stride == 0) return fail(ctx, DRX_ERR_ARG, "wave_stack: start_stride 0");
    if (out_stride < (uint64_t)DRX_STACK_COLS)
        return fail(ctx, DRX_ERR_ARG, "wave_stack: rows %llu int64 apart do not hold %d", (unsigned long long)out_stride, DRX_STACK_COLS);
    if (width == 0) return DRX_OK;  // (no row to write: nothing to launch)
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    if (d_select) DRX_HIP(ctx, p->mem.once(&p->stack_list, stack_list_bytes(p->G)));
    DRX_HIP(ctx, launch_wave_stack(c, p->stack_list, ctx->stack_workgroups, d_start, start_stride, offset, width, d_select, d_out, out_stride));
    return call_end(p, DRX_PATH_STACK);
}

// several windows of every waveform, at per-window starts (drx_windows.hip)
static drx_status decode_windows(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                 const uint32_t *d_sideband, bool sideband, const int64_t *d_start, uint64_t start_wave_stride,
                                 uint64_t start_win_stride, const uint32_t *d_count, uint32_t n_win, int64_t offset, uint32_t width,
                                 int16_t pad, int16_t *d_out, uint64_t out_wave_stride, uint64_t out_win_stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "decode_windows", d_in && d_chunk_word_off && d_start && d_out, d_sideband, sideband)) return st;
    if (start_wave_stride == 0 || start_win_stride == 0) return fail(ctx, DRX_ERR_ARG, "decode_windows: a start stride of 0");
    if (out_win_stride < width)
        return fail(ctx, DRX_ERR_ARG, "decode_windows: rows %llu samples apart do not hold %u", (unsigned long long)out_win_stride, width);
    // a waveform's rows must end in front of the next one's: (n_win - 1) * out_win_stride + width samples, in 128 bits
    if (n_win && (unsigned __int128)(n_win - 1u) * out_win_stride + width > (unsigned __int128)out_wave_stride)
        return fail(ctx, DRX_ERR_ARG, "decode_windows: waveforms %llu samples apart do not hold %u rows %llu apart",
                    (unsigned long long)out_wave_stride, n_win, (unsigned long long)out_win_stride);
    if (width == 0 || n_win == 0) return DRX_OK;  // (no row receives a sample: nothing to launch)
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kWindowsForm, p->windows, windows_blocks_scratch_bytes));
    DRX_HIP(ctx, launch_decode_windows(c, p->dec.d_blk, p->windows.d, d_start, start_wave_stride, start_win_stride, d_count, n_win, offset, width,
                                       pad, d_out, out_wave_stride, out_win_stride, &p->windows.last_form));
    return call_end(p, DRX_PATH_WINDOWS);
}

// every pulse of every waveform: threshold discrimination (drx_pulses.hip)
static drx_status find_pulses(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const uint32_t *d_sideband, bool sideband, const int64_t *d_thr, uint64_t thr_stride, int64_t thr,
                              int32_t polarity, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count, int64_t *d_out) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "find_pulses", d_in && d_chunk_word_off && d_count, d_sideband, sideband)) return st;
    if (max_pulses && !d_out) return fail(ctx, DRX_ERR_ARG, "find_pulses: no output for %u pulses per waveform", max_pulses);
    if (polarity == 0) return fail(ctx, DRX_ERR_ARG, "find_pulses: polarity 0");
    if (min_width == 0) return fail(ctx, DRX_ERR_ARG, "find_pulses: min_width 0");
    if (d_thr && thr_stride == 0) return fail(ctx, DRX_ERR_ARG, "find_pulses: thr_stride 0");
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kPulsesForm, p->pulses, pulses_blocks_scratch_bytes));
    // ... and the records its blocks stage: as many as this call needs
    if (blocks_form_batch(p->G, p->dec.d_blk, kPulsesForm)) {
        const size_t bytes = pulses_blocks_staging_bytes(p->G, max_pulses);
        const hipError_t e = p->mem.reserve(p->pulses.stage, bytes, 0, false, Buffers::KeepOld, ctx->stream);
        if (e != hipSuccess) return fail(ctx, DRX_ERR_NOMEM, "find_pulses: staging of %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    DRX_HIP(ctx, launch_find_pulses(c, p->dec.d_blk, p->pulses.d, p->pulses.stage.ptr, d_thr, thr_stride, thr, polarity < 0, min_width, max_pulses,
                                    d_count, d_out, &p->pulses.last_form));
    return call_end(p, DRX_PATH_PULSES);
}

// re-coding to another RiceParameter, and the sizes at every one, from the encoded stream (drx_transcode.hip)
static drx_status trc_scratch(drx_plan *p, TrcScratch *t) {  // (trc_scratch_view(), drx_internal.h)
    const hipError_t e = p->mem.once(&p->trc.d, trc_scratch_view(p->G, nullptr).bytes);
    if (e != hipSuccess) return fail(p->ctx, DRX_ERR_NOMEM, "transcode scratch: %s", hipGetErrorString(e));
    *t = trc_scratch_view(p->G, p->trc.d);
    return DRX_OK;
}

// (what drx_transcode and drx_transcode_filter refuse alike, with nothing launched)
static drx_status transcode_args(drx_plan *p, const char *who, const uint32_t *d_in, const uint64_t *d_chunk_word_off, const uint32_t *d_sideband,
                                 bool sideband, uint32_t new_k, const uint32_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                                 const uint32_t *d_out_wave_words) {
    drx_ctx *ctx = p->ctx;
    if (new_k > 15u) return fail(ctx, DRX_ERR_ARG, "%s: new_rice_k %u (0..15)", who, new_k);
    if (!d_in || !d_chunk_word_off || !d_out_off || (sideband && !d_sideband)) return fail(ctx, DRX_ERR_ARG, "%s: null pointer", who);
    if (!d_out && out_cap) return fail(ctx, DRX_ERR_ARG, "%s: no output buffer but a capacity of %llu words", who, (unsigned long long)out_cap);
    if (sideband && (d_sideband == p->d_wave_words || d_out_wave_words == d_sideband))
        return fail(ctx, DRX_ERR_ARG, "the side-band table must be neither the plan's own nor the output's (copy it first)");
    return DRX_OK;
}
// ... and what every call that names a target filter refuses
static drx_status target_filter_args(drx_plan *p, const char *who, uint32_t n_taps, const int32_t *taps) {
    if (n_taps == 0 || n_taps > DRX_MAX_TAPS) return fail(p->ctx, DRX_ERR_ARG, "%s: new_n_taps %u (1..%d)", who, n_taps, DRX_MAX_TAPS);
    if (!taps) return fail(p->ctx, DRX_ERR_ARG, "%s: null pointer", who);
    if (taps[0] == 0) return fail(p->ctx, DRX_ERR_ARG, "%s: new_taps[0] must not be 0 (the inverse filter divides by it)", who);
    return DRX_OK;
}

static drx_status transcode(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                            const uint32_t *d_sideband, bool sideband, uint32_t new_k, uint32_t *d_out, uint64_t out_cap,
                            uint64_t *d_out_off, uint32_t *d_out_wave_words) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = transcode_args(p, "transcode", d_in, d_chunk_word_off, d_sideband, sideband, new_k, d_out, out_cap, d_out_off, d_out_wave_words))
        return st;
    DRX_ON_DEVICE(ctx);
    TrcScratch t;
    if (const drx_status st = trc_scratch(p, &t)) return st;
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kTranscodeForm, p->trc.blocks, trc_blocks_scratch_bytes));
    DRX_HIP(ctx, launch_transcode(c, new_k, t, EncOut{d_out, out_cap, d_out_off, d_out_wave_words}, p->dec.d_blk, p->trc.blocks.d, &p->trc.blocks.last_form));
    return call_end(p, DRX_PATH_TRANSCODE);
}

// ... to another prediction filter as well (drx_refilter.hip): the plan's filter is the source's.  Always the lane form
static drx_status transcode_filter(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                   const uint32_t *d_sideband, bool sideband, uint32_t new_k, uint32_t new_n_taps, const int32_t *new_taps,
                                   uint32_t *d_out, uint64_t out_cap, uint64_t *d_out_off, uint32_t *d_out_wave_words) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = target_filter_args(p, "transcode_filter", new_n_taps, new_taps)) return st;
    if (const drx_status st = transcode_args(p, "transcode_filter", d_in, d_chunk_word_off, d_sideband, sideband, new_k, d_out, out_cap, d_out_off,
                                             d_out_wave_words))
        return st;
    DRX_ON_DEVICE(ctx);
    TrcScratch t;
    if (const drx_status st = trc_scratch(p, &t)) return st;
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, launch_refilter(c, new_k, RefilterTarget{new_n_taps, new_taps}, t, EncOut{d_out, out_cap, d_out_off, d_out_wave_words},
                                 &p->trc.blocks.last_form));
    return call_end(p, DRX_PATH_TRANSCODE);
}

extern "C" {

drx_status drx_decode(drx_plan *p, const uint32_t *d_in, uint64_t in_words,
                      const uint64_t *d_chunk_word_off, int16_t *d_out) {
    return decode_launch(p, d_in, in_words, d_chunk_word_off, d_out, false);
}

drx_status drx_decode_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                      const uint32_t *d_wave_words, int16_t *d_out) {
    if (!d_wave_words) return DRX_ERR_ARG;
    if (p && d_wave_words == p->d_wave_words) return fail(p->ctx, DRX_ERR_ARG, "the side-band table must not be the plan's own (copy it first)");
    return decode_launch(p, d_in, in_words, d_chunk_word_off, d_out, false, d_wave_words);
}

drx_status drx_wave_stats(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, uint32_t head_len,
                          int64_t *d_out) {
    return wave_stats(p, d_in, in_words, d_chunk_word_off, nullptr, false, head_len, d_out);
}

drx_status drx_wave_stats_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                          const uint32_t *d_wave_words, uint32_t head_len, int64_t *d_out) {
    return wave_stats(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, head_len, d_out);
}

drx_status drx_wave_bins(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, const int64_t *d_start,
                         uint64_t start_stride, int64_t offset, uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride) {
    return wave_bins(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_start, start_stride, offset, bin, n_bins, d_out, out_wave_stride);
}

drx_status drx_wave_bins_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                         const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_stride, int64_t offset,
                                         uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride) {
    return wave_bins(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_start, start_stride, offset, bin, n_bins, d_out,
                     out_wave_stride);
}

drx_status drx_wave_stack(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, const int64_t *d_start,
                          uint64_t start_stride, int64_t offset, uint32_t width, const uint8_t *d_select, int64_t *d_out, uint64_t out_stride) {
    return wave_stack(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_start, start_stride, offset, width, d_select, d_out, out_stride);
}

drx_status drx_wave_stack_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                          const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_stride, int64_t offset,
                                          uint32_t width, const uint8_t *d_select, int64_t *d_out, uint64_t out_stride) {
    return wave_stack(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_start, start_stride, offset, width, d_select, d_out,
                      out_stride);
}

drx_status drx_decode_window(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width, int16_t pad,
                             int16_t *d_out, uint64_t out_stride_samples) {
    return decode_window(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_start, start_stride, offset, width, pad, d_out,
                         out_stride_samples);
}

drx_status drx_decode_window_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                             const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_stride,
                                             int64_t offset, uint32_t width, int16_t pad, int16_t *d_out,
                                             uint64_t out_stride_samples) {
    return decode_window(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_start, start_stride, offset, width, pad, d_out,
                         out_stride_samples);
}

drx_status drx_decode_windows(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const int64_t *d_start, uint64_t start_wave_stride, uint64_t start_win_stride, const uint32_t *d_count,
                              uint32_t n_win, int64_t offset, uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_wave_stride,
                              uint64_t out_win_stride) {
    return decode_windows(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_start, start_wave_stride, start_win_stride, d_count, n_win,
                          offset, width, pad, d_out, out_wave_stride, out_win_stride);
}

drx_status drx_decode_windows_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                              const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_wave_stride,
                                              uint64_t start_win_stride, const uint32_t *d_count, uint32_t n_win, int64_t offset,
                                              uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_wave_stride,
                                              uint64_t out_win_stride) {
    return decode_windows(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_start, start_wave_stride, start_win_stride, d_count,
                          n_win, offset, width, pad, d_out, out_wave_stride, out_win_stride);
}

drx_status drx_find_pulses(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                           const int64_t *d_thr, uint64_t thr_stride, int64_t thr, int32_t polarity, uint32_t min_width,
                           uint32_t max_pulses, uint32_t *d_count, int64_t *d_out) {
    return find_pulses(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_thr, thr_stride, thr, polarity, min_width, max_pulses,
                       d_count, d_out);
}

drx_status drx_find_pulses_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                           const uint32_t *d_wave_words, const int64_t *d_thr, uint64_t thr_stride, int64_t thr,
                                           int32_t polarity, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count,
                                           int64_t *d_out) {
    return find_pulses(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_thr, thr_stride, thr, polarity, min_width,
                       max_pulses, d_count, d_out);
}

drx_status drx_transcode(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, uint32_t new_rice_k,
                         uint32_t *d_out, uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return transcode(p, d_in, in_words, d_chunk_word_off, nullptr, false, new_rice_k, d_out, out_cap_words, d_out_chunk_word_off,
                     d_out_wave_words);
}

drx_status drx_transcode_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                         const uint32_t *d_wave_words, uint32_t new_rice_k, uint32_t *d_out, uint64_t out_cap_words,
                                         uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return transcode(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, new_rice_k, d_out, out_cap_words, d_out_chunk_word_off,
                     d_out_wave_words);
}

drx_status drx_estimate_words_encoded(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                      const uint32_t *d_wave_words, uint64_t words_out[16]) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    const bool sideband = d_wave_words != nullptr;
    if (const drx_status st = stream_call_args(p, "estimate_words_encoded", d_in && d_chunk_word_off && words_out, d_wave_words, sideband)) return st;
    DRX_ON_DEVICE(ctx);
    TrcScratch t;
    if (const drx_status st = trc_scratch(p, &t)) return st;
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_wave_words, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kTranscodeForm, p->trc.blocks, trc_blocks_scratch_bytes));
    DRX_HIP(ctx, launch_estimate_words_encoded(c, t.est, p->dec.d_blk, p->trc.blocks.d, &p->trc.blocks.last_form));
    (void)call_end(p, DRX_PATH_TRANSCODE);
    DRX_HIP(ctx, hipMemcpyAsync(words_out, t.est, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return drx_plan_finish(p, nullptr);  // (waits; a stream that failed validation: DRX_ERR_CORRUPT, words_out undefined)
}

drx_status drx_transcode_filter(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, uint32_t new_rice_k,
                                uint32_t new_n_taps, const int32_t *new_taps, uint32_t *d_out, uint64_t out_cap_words,
                                uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return transcode_filter(p, d_in, in_words, d_chunk_word_off, nullptr, false, new_rice_k, new_n_taps, new_taps, d_out, out_cap_words,
                            d_out_chunk_word_off, d_out_wave_words);
}

drx_status drx_transcode_filter_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                                const uint32_t *d_wave_words, uint32_t new_rice_k, uint32_t new_n_taps,
                                                const int32_t *new_taps, uint32_t *d_out, uint64_t out_cap_words,
                                                uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return transcode_filter(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, new_rice_k, new_n_taps, new_taps, d_out, out_cap_words,
                            d_out_chunk_word_off, d_out_wave_words);
}

drx_status drx_estimate_words_encoded_filter(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                             const uint32_t *d_wave_words, uint32_t new_n_taps, const int32_t *new_taps,
                                             uint64_t words_out[16]) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    const bool sideband = d_wave_words != nullptr;
    if (const drx_status st = target_filter_args(p, "estimate_words_encoded_filter", new_n_taps, new_taps)) return st;
    if (const drx_status st = stream_call_args(p, "estimate_words_encoded_filter", d_in && d_chunk_word_off && words_out, d_wave_words, sideband)) return st;
    DRX_ON_DEVICE(ctx);
    TrcScratch t;
    if (const drx_status st = trc_scratch(p, &t)) return st;
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_wave_words, false, &c)) return st;
    DRX_HIP(ctx, launch_estimate_words_refiltered(c, RefilterTarget{new_n_taps, new_taps}, t.est, &p->trc.blocks.last_form));
    (void)call_end(p, DRX_PATH_TRANSCODE);
    DRX_HIP(ctx, hipMemcpyAsync(words_out, t.est, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return drx_plan_finish(p, nullptr);  // (waits, as drx_estimate_words_encoded does)
}

}  // extern "C"
