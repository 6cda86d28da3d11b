// drx_internal.h -- types shared by the kernels and the C ABI glue (not installed).
#ifndef DRX_INTERNAL_H
#define DRX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <vector>

#include "../../include/deltarice_hip.h"

namespace drx {

// One HDF5 chunk of the batch (device resident table, ragged batches only).
struct ChunkDesc {
    uint64_t sample_off;  // first sample of the chunk in the raw int16 batch
    uint64_t wave_base;   // global index of the chunk's first waveform
    uint32_t n_samples;   // N  (u32 header word of the encoded chunk, src/deltaRice.c:415)
    uint32_t wave_len;    // L  (>= 1; "whole chunk" already resolved to N)
    uint32_t n_waves;     // ceil(N / L)
    uint32_t pad_;
};

// Passed to kernels by value.  Its device tables are buffers of the plan (drx_api.h), which keeps no other pointer to them;
// a ragged plan's tables are what each path's planner (*_plan_ragged() below) computed from the host's chunk table.
struct Geom {
    const ChunkDesc *chunks;  // device pointer, n_chunks entries (unused when uniform)
    uint64_t n_chunks;
    uint64_t total_waves;
    uint32_t uniform;  // all chunks share (n_samples, wave_len): pure arithmetic mapping
    uint32_t u_n_samples, u_wave_len, u_n_waves;
    uint32_t k;  // log2(M)
    // prediction filter (src/deltaRice.c:49-76,78-103).  n_taps == 0: the default [1,-1] (delta), which
    // the fast kernels implement; otherwise taps (device pointer, n_taps entries) select the general
    // FIR / IIR kernels.
    uint32_t n_taps;
    const int32_t *taps;
    // general filters the fast kernels take: at most 4 taps with taps[0] = +-1 (the inverse filter then has no
    // division); fast_t0neg = (taps[0] == -1), fast_nt[j-1] = -taps[j] (0 beyond n_taps)
    uint32_t fast_taps, fast_t0neg;
    uint32_t fast_nt[3];
    // forward filter in the single-pass encoder: at most 4 taps, any taps[0]; enc_t[j] = taps[j] mod 2^16
    uint32_t enc_fast;
    uint32_t enc_t[4];
    uint64_t total_samples;  // of the batch
    // pinned host word (device-visible) that every encoder writes the batch's encoded word count to beside DevStatus: the host
    // reads it -- without waiting for anything -- when it chooses the NEXT encode's kernel (drx_api_encode.hip, stream_encoder_suits())
    uint64_t *host_words;
    uint32_t dbg;  // "debug_flags" context option (DRX_DBG_* of include/deltarice_hip.h); 0 in normal use
    // ragged batches, walk inside the decode launch: chunk indices, short-waveform chunks first
    // (walk_short[n_short], then walk_long[n_long]: walk_plan_ragged()), and the largest ceil(n_waves / 64) of any chunk
    // (decode_plan_ragged())
    const uint32_t *walk_short, *walk_long;
    uint32_t n_short, n_long, max_groups;
    uint64_t max_wave_len64;  // ragged batches: 64 x the longest WaveformLength (how far apart a wavefront's 64 lines can lie)
    // ragged batches of few long waveforms: the block-parallel decoder takes them (decided when the plan is made, from the
    // host's chunk table: drx_blocks.hip); lanes per block and look-back slots per waveform for the longest of them
    uint32_t rag_blocks, rag_blk_nt, rag_blk_slots;
    // ... launched once per class of WaveformLengths (floor(log2 L): the waveforms of a launch differ by less than 2x, so
    // that run-major tickets over them are rarely empty): rag_blk_list = waveform indices class by class (device),
    // class c = entries [rag_blk_class_off[c], rag_blk_class_off[c + 1]), its longest WaveformLength in rag_blk_class_len[c]
    const uint32_t *rag_blk_list;
    uint32_t rag_blk_classes;
    uint32_t rag_blk_class_off[33], rag_blk_class_len[32];
    // general prediction filter behind the block decoder (drx_iir.hip): tables, tiles and their look-back state
    const uint32_t *iir_tab;
    const uint32_t *blk_iir_tab;  // ... and inside the block decoder (FUSE): blocks_iir_tables()
    const uint64_t *iir_chunk_tile_base;  // ragged: first tile of every chunk, n_chunks + 1 entries
    uint64_t iir_n_tiles;
    uint64_t *iir_state;                  // uint64[iir_n_tiles + 1]
    // ragged batches that the segment encoder takes (some chunk has short or long waveforms): first unit (waveform x
    // segment slot) of every chunk, n_chunks + 1 entries, and their total (segments_plan_ragged())
    const uint64_t *seg_unit_base;
    uint64_t seg_units;
    // ragged batches small enough for the parallel header walks (drx_walk.hip): set when the plan is made (walk_plan_ragged());
    // rag_bw_blocks_max = 4096-word blocks of the largest short-waveform chunk at 25 bits per sample
    uint32_t rag_par, rag_bw_blocks_max;
    uint32_t rag_bw_min_len;  // ... and the smallest WaveformLength among those chunks (bounds the headers of a block)
    uint32_t rag_pw_min_waves;  // ... and the fewest waveforms any LONG-waveform chunk has (k_walk_sparse: from 64 on)
    // ragged batches, lane-per-waveform decode outside the fused launch: {chunk, group of 64 waveforms} of every
    // wavefront, longest WaveformLength first; rag_groups entries
    const uint2 *rag_order;
    uint32_t rag_groups;
    uint32_t rag_groups_long;  // ... of which the first ones belong to chunks of WaveformLength > 2048 (the chunk-wide walk's)
    // ragged batches the pieces encoder takes (pieces_plan_ragged()): first workgroup of every chunk, n_chunks + 1 entries
    const uint32_t *pc_wg_base;
    uint32_t pc_super;  // ... and every chunk's WaveformLength is above kPcMaxLen (waveforms over several workgroups)
    uint32_t pc_packed;  // ... or every chunk's WaveformLength is piece_packable()
};

struct DevStatus {
    uint32_t err;  // kErr* bits, OR-ed by kernels
    uint32_t listed;  // drx_find_pulses / drx_decode_windows / drx_transcode / drx_wave_bins, block form: the waveforms handed to the lane kernel(s) behind the blocks
    uint64_t total_words;  // encode: words of the encoded batch
    uint32_t redone;       // drx_find_pulses, block form: the waveforms whose blocks its second launch ran again
    uint32_t pad_;
};

constexpr uint32_t kErrCapacity = 1u;
constexpr uint32_t kErrCorrupt = 2u;
constexpr uint32_t kErrInternal = 4u;

// ---------------------------------------------------------------------------
// Call frames: what the host launchers below are given in front of a call's own arguments.  Plain aggregates that the C ABI
// glue fills from the plan once per call (call_begin(), drx_api.h); they stop at the <<< >>>, kernels take loose arguments.
// ---------------------------------------------------------------------------
// A call on an ENCODED batch.  tables_ready: wave_off / wave_words are already filled in (the one-chunk host path walks the
// header chain on the CPU while the chunk is in flight to the device; the side-band forms derive them from the caller's
// table): no walk
struct StreamCall {
    const Geom *G;
    const uint32_t *d_in;  // the encoded batch: its words, their count, the chunk offsets
    uint64_t in_words;
    const uint64_t *d_chunk_word_off;
    uint64_t *d_wave_off;  // the plan's header tables
    uint32_t *d_wave_words;
    bool tables_ready;
    void *d_pw;  // scratch of the parallel walks (nullptr: the plan has none)
    DevStatus *d_status;
    hipEvent_t *ev;  // optional: the call's four profiling events
    hipStream_t s;
    // the same call on another stream, or over a view of its geometry (launch_decode(): side stream, split lanes launch)
    StreamCall on(hipStream_t st) const { StreamCall c = *this; c.s = st; return c; }
    StreamCall view(const Geom &Gv) const { StreamCall c = *this; c.G = &Gv; return c; }
};
// What the encoders, launch_gather() and launch_transcode() write: the words, the chunk offsets, the n_i table
struct EncOut {
    uint32_t *d_out;
    uint64_t out_cap;
    uint64_t *d_chunk_word_off;
    uint32_t *d_wave_words;
};
// A call that encodes raw samples
struct EncodeCall {
    const Geom *G;
    const int16_t *d_in;
    EncOut out;
    DevStatus *d_status;
    hipEvent_t *ev;
    hipStream_t s;
};

hipError_t launch_encode(const EncodeCall &c, uint32_t *d_wave_rel, uint64_t *d_chunk_words);

// launch_decode() takes the workgroup-per-waveform decoder for uniform batches whose lane-per-waveform decode would leave most of
// the 98 304 lane slots empty and the block decoder does not take: at most 16 384 waveforms of at least 65 536 samples, or at most
// 4 096 of at least 16 384 (measured crossover at 350 M samples: L = 32 768 lanes 2.2 ms / long 2.9 ms, L = 65 536 3.6 / 2.4 ms);
// the same test sends such batches to the segment encoder where the pieces encoder does not apply
__host__ __device__ inline bool long_waveform_batch(uint64_t total_waves, uint32_t wave_len) {
    return (wave_len >= 65536u && total_waves <= 16384u) || (wave_len >= 16384u && total_waves <= 4096u);
}
// A launch carries fewer than 2^32 threads (the HIP runtime refuses more): a kernel that gives every waveform a wavefront in
// workgroups of up to eight takes at most this many waveforms in one launch
constexpr uint64_t kMaxWavefrontWaves = (1ull << 26) - 8u;
static inline unsigned blocks_for(uint64_t items, unsigned per_block) { return (unsigned)((items + per_block - 1) / per_block); }
static inline void mark(hipEvent_t *ev, int i, hipStream_t s) {  // (optional profiling events of a launch)
    if (ev) (void)hipEventRecord(ev[i], s);
}

// a chunk's worst-case word count: its header, 25 bits per sample rounded up per waveform, the waveforms' headers
inline uint64_t chunk_max_words(uint32_t n_samples, uint32_t n_waves) { return 1u + 2ull * n_waves + (((uint64_t)n_samples * 25u + 31u) >> 5); }

// The header walk in front of the decoders (drx_walk.hip): fills wave_off / wave_words and judges the chain.
// Which parallel walks take the batch (neither: the serial walk, or the walk inside the lanes launch -- route_decode())
struct WalkRoute {
    bool chunk_wide, blocks;  // the chunk-wide walk, the block-parallel walk (ragged batches: both)
    bool by_chains;           // ... the chunk-wide walk by chains, not by reading the chunks
};
WalkRoute route_walk(const Geom &G, bool tables_ready, bool have_scratch);
// ragged plans: sets n_short / n_long and the parallel walks' rag_par / rag_bw_* / rag_pw_* fields; returns the host copy of
// the walk lists (walk_short = the first n_short entries, walk_long the rest)
std::vector<uint32_t> walk_plan_ragged(Geom &G, const ChunkDesc *host_chunks);
uint64_t walk_scratch_bytes(const Geom &G);  // d_pw of the launchers below (0: the batch takes neither parallel walk)
hipError_t walk_scratch_reset(const Geom &G, void *d_pw, hipStream_t s);  // in front of the parallel walks of a call
void launch_walk_chunk_wide(const StreamCall &c, bool by_chains);
void launch_walk_blocks(const StreamCall &c);
void launch_walk_serial(const StreamCall &c);
// The walk in front of a call that reads the WHOLE batch behind it (drx_wave_stats, drx_decode_window, drx_find_pulses,
// drx_transcode, drx_estimate_words_encoded): route_walk()'s choice, all of it on the call's stream
hipError_t launch_batch_walk(const StreamCall &c);
// ... as those calls open: event 0, the walk unless the tables are ready, event 1
inline hipError_t batch_walk_prologue(const StreamCall &c) {
    mark(c.ev, 0, c.s);
    const hipError_t e = c.tables_ready ? hipSuccess : launch_batch_walk(c);
    if (e == hipSuccess) mark(c.ev, 1, c.s);
    return e;
}
// ... and the launches of those calls' kernels, a lane per waveform: the wavefronts of the batch -- rag_order's groups for a
// ragged plan that has them under the kernels that follow it (by_rag_order: lane_wave(), drx_lane_stream.h), 64 consecutive
// waveforms each otherwise -- in slices of at most 2^25 per launch (a launch carries fewer than 2^32 threads).
// go(first wavefront, wavefronts)
template <class F> inline void for_wavefront_slices(const Geom &G, bool by_rag_order, F go) {
    constexpr uint64_t max_grid = 1ull << 25;
    const uint64_t n_wf = (by_rag_order && !G.uniform && G.rag_order) ? (uint64_t)G.rag_groups : (G.total_waves + 63u) / 64u;
    for (uint64_t base = 0; base < n_wf; base += max_grid) go(base, (unsigned)(n_wf - base < max_grid ? n_wf - base : max_grid));
}
// ... no walk: the tables from the n_i table an encode left behind, checked against the stream
hipError_t launch_sideband_tables(const StreamCall &c, const uint32_t *d_n, const uint32_t *d_list = nullptr,
                                  uint32_t n_list = 0);  // d_list: these chunks only
// drx_decode_select (drx_select.hip): the walk over the chunks a selection touches (select_walk_class(): which of its three
// lists a chunk belongs to), then a wavefront per selected waveform
int select_walk_class(uint32_t n_waves, uint32_t wave_len);
hipError_t launch_select_walk(const StreamCall &c, const uint32_t *d_lists, uint32_t n_sparse, uint32_t n_block, uint32_t n_chain,
                              uint32_t *d_fail);
hipError_t launch_decode_select(const StreamCall &c, const uint64_t *d_sel, uint64_t n_sel, int16_t *d_out, uint64_t stride);
// drx_gather_encoded (drx_gather.hip): behind the same walk, sizes + scan + offsets, then the copy of the entries' word ranges
// (tiles: a workgroup per run of short entries; otherwise a wavefront per entry, or per piece of a long one; resume: the walk's
// tables, the sizes and the scanned block sums of the last call with this list are still in place -- the call behind a sizing call)
uint64_t gather_scan_blocks(uint64_t n_sel);
// its device-only scratch, a buffer of the plan: uint64 ent_pos[n_sel] | uint64 block_sum[blocks + 2] (the last two: total,
// status) | uint32 ent_words[n_sel] | uint32 ctrl[1]
struct GatherScratch {
    uint64_t *ent_pos, *block_sum;
    uint32_t *ent_words, *ctrl;
    uint64_t bytes;
};
inline GatherScratch gather_scratch_view(void *base, uint64_t n_sel) {
    GatherScratch t;
    t.ent_pos = (uint64_t *)base;
    t.block_sum = t.ent_pos + n_sel;
    t.ent_words = (uint32_t *)(t.block_sum + gather_scan_blocks(n_sel) + 2);
    t.ctrl = t.ent_words + n_sel;
    t.bytes = (n_sel + gather_scan_blocks(n_sel) + 2) * sizeof(uint64_t) + (n_sel + 1) * sizeof(uint32_t);
    return t;
}
// d_sel: the list; d_chunk_samples: N_c of every output chunk of chunk_waves entries; mean_words: the batch's words per
// waveform, roughly (sizes the wavefront form's grid).  ev: {start, walk's end, offsets' end, end}, of which the caller
// records all but the third
hipError_t launch_gather(const StreamCall &c, const uint64_t *d_sel, uint64_t n_sel, uint64_t chunk_waves,
                         const uint32_t *d_chunk_samples, const EncOut &out, const GatherScratch &t, bool tiles, uint64_t mean_words,
                         bool resume);
// The block forms of drx_wave_stats, drx_find_pulses, drx_decode_windows, drx_transcode and drx_wave_bins (drx_*_blocks.hip): few long waveforms under
// the delta filter (any_filter: under every filter) give a workgroup a block of a waveform's stream, as the block decoder does (d_blk = its scratch), with the call's lane
// kernel behind the blocks for the waveforms they list.  One rule says which batches: the decoder's own test, blocks against
// lanes by their cost (blocks_batch(), drx_blocks.hip), with the rate of THIS call's lane kernel, on a plan that has d_blk, unless
// a debug flag keeps the batch on lanes (DRX_DBG_NO_LONG_PATHS, DRX_DBG_LONG_NOT_BLOCKS, the call's own lanes_flag).  A ragged
// plan's choice was made from the host's chunk table when the plan was created: the decoder's.  Each form's scratch beyond d_blk
// belongs to the plan and is allocated by the first call that takes the form (form_scratch(), drx_api_stream.hip).
struct BlkFormRule {
    double lane_us;  // what the call's lane kernel takes per sample
    uint32_t lanes_flag, all_fallback_flag;  // DRX_DBG_*: never the block form; the block form lists every waveform
    bool any_filter = false;  // the form works on residuals: every prediction filter the plan accepts, not the delta filter alone
};
// k_wave_stats takes 52 ns per sample and lane where k_decode_lanes takes 60, so a uniform batch at the
// decoder's break-even -- 4 chunks of 2100 x 7000: one block per waveform, 393 us of blocks against 420 us of decoding lanes, but
// 364 us of reducing lanes -- stays a lane per waveform there
constexpr double kStatsLaneUs = 0.052;
constexpr BlkFormRule kStatsForm{kStatsLaneUs, DRX_DBG_STATS_LANES, DRX_DBG_STATS_ALL_FALLBACK};
// k_find_pulses on rare pulses takes 24.1 ms for a lane of 500 000 samples (profiles/find_pulses_bench.txt): 0.048 us per sample
constexpr double kPulsesLaneUs = 0.048;
constexpr BlkFormRule kPulsesForm{kPulsesLaneUs, DRX_DBG_PULSES_LANES, DRX_DBG_PULSES_ALL_FALLBACK};
// k_decode_windows on sparse windows takes 25.7 ms for a lane of 500 000 samples, 700 ms for one of 14 M and 4.67 ms for one of
// 81 920 (profiles/decode_windows_bench.txt): 0.050 - 0.057 us per sample, the NOPTREX shape's 0.051 taken
constexpr double kWindowsLaneUs = 0.051;
constexpr BlkFormRule kWindowsForm{kWindowsLaneUs, DRX_DBG_WINDOWS_LANES, DRX_DBG_WINDOWS_ALL_FALLBACK};
// drx_transcode / drx_estimate_words_encoded: the re-code has no filter arithmetic, so its form admits every filter.  Its lane
// kernels parse twice and emit once: 102.3 ms for lanes of 500 000 samples, 0.2045 us per sample (profiles/transcode_blocks_bench.txt,
// row `noptrex`, lane form; 0.204 on `nedm`, 0.211 on `long25`).  blocks_batch() prices the DECODER's blocks, and this form runs
// the blocks twice and re-codes every sample in the second run (a second parse and the emission): the same row's block form takes
// 4.06 ms where the block decoder takes 1.26 - 1.31 ms for that batch, 3.2 times as long at m' = 16.  Four
// times a decoder's block is charged (a smaller m' expands the result and the pack drains it in more passes: not measured) -- the
// rule is given a quarter of the lane rate, and "blocks < lanes" is then the comparison of 4 x the decoder's blocks with this
// call's lanes.
constexpr double kTranscodeLaneUs = 0.2045;
constexpr double kTranscodeBlockFactor = 4.0;
constexpr BlkFormRule kTranscodeForm{kTranscodeLaneUs / kTranscodeBlockFactor, DRX_DBG_TRANSCODE_LANES, DRX_DBG_TRANSCODE_ALL_FALLBACK, true};
// drx_wave_bins: the block form (drx_bins_blocks.hip) is taken only under the context option "bins_impl" = 1 -- launch_wave_bins()
// asks blocks_form_batch() with this rule only then, and with the default 0 every batch stays a lane per waveform and the rule's
// two flags are inert (the form word of today's calls is pinned by tests; making the block form the default is a follow-up).
// k_wave_bins takes 28.53 ms for a lane of 500 000 samples at 1000 bins (profiles/wave_bins_bench.txt, row `noptrex`): 0.057 us
// per sample
constexpr double kBinsLaneUs = 0.057;
// blocks_batch() prices the DECODER's blocks, and this form costs 1.40 (NOPTREX), 1.71 (nEDM) and 1.32 (25 x 14 M) times what
// plan.decode takes for the same batch in the same process (profiles/wave_bins_bench.txt, the rows `impl 1`): the fill, the walk
// over the bins and the merge.  Near break-even that misroutes: 4 chunks of 2100 x 7000 are 393 us of decoder's blocks against 399
// us of these lanes, and would take a block form that costs 520 us or more.  The smallest of the three ratios is charged (row
// `long25 impl 1`: 0.780 / 0.592) -- the rule is given the lane rate divided by it, as kTranscodeForm's is.
constexpr double kBinsBlockFactor = 1.32;
constexpr BlkFormRule kBinsForm{kBinsLaneUs / kBinsBlockFactor, DRX_DBG_BINS_LANES, DRX_DBG_BINS_ALL_FALLBACK};
bool blocks_form_batch(const Geom &G, const void *d_blk, const BlkFormRule &r);
// the form word of a call, one set of values under five names: LANES, or BLOCKS | FALLBACK_ALL under the rule's all_fallback_flag
static_assert(DRX_STATS_FORM_LANES == DRX_PULSES_FORM_LANES && DRX_STATS_FORM_LANES == DRX_WINDOWS_FORM_LANES &&
                  DRX_STATS_FORM_BLOCKS == DRX_PULSES_FORM_BLOCKS && DRX_STATS_FORM_BLOCKS == DRX_WINDOWS_FORM_BLOCKS &&
                  DRX_STATS_FORM_FALLBACK_ALL == DRX_PULSES_FORM_FALLBACK_ALL && DRX_STATS_FORM_FALLBACK_ALL == DRX_WINDOWS_FORM_FALLBACK_ALL &&
                  DRX_STATS_FORM_LANES == DRX_TRANSCODE_FORM_LANES && DRX_STATS_FORM_BLOCKS == DRX_TRANSCODE_FORM_BLOCKS &&
                  DRX_STATS_FORM_FALLBACK_ALL == DRX_TRANSCODE_FORM_FALLBACK_ALL && DRX_STATS_FORM_LANES == DRX_BINS_FORM_LANES &&
                  DRX_STATS_FORM_BLOCKS == DRX_BINS_FORM_BLOCKS && DRX_STATS_FORM_FALLBACK_ALL == DRX_BINS_FORM_FALLBACK_ALL,
              "blocks_form_word() serves the five calls");
uint32_t blocks_form_word(const Geom &G, bool blocks, const BlkFormRule &r);
// The waveforms a block form leaves to the lane kernel behind it, a list on the device, part of the form's scratch:
// u32 n_listed (+ pad to 8 bytes) | u32 listed[W].  (blk_listed() and blk_list_append(), drx_blocks.h, fill it.)
struct BlkFallbackList {
    uint32_t *n_listed, *listed;
    static constexpr uint64_t bytes(uint64_t W) { return 8u + 4u * W; }
    static BlkFallbackList at(void *base) { return {reinterpret_cast<uint32_t *>(base), reinterpret_cast<uint32_t *>(base) + 2}; }
};
// drx_wave_stats (drx_stats.hip): behind the whole batch's walk (tables_ready: the side-band's tables are in place), a lane per
// waveform that parses and reduces: int64 d_out[total_waves][DRX_STAT_COLS].  ev: {start, walk's end, kernel's end, end}
// form_out: DRX_STATS_FORM_* of include/deltarice_hip.h.  The block form: d_sacc = stats_blocks_scratch_bytes() of accumulators and list
hipError_t launch_wave_stats(const StreamCall &c, void *d_blk, void *d_sacc, uint32_t head_len, int64_t *d_out, uint32_t *form_out);
uint64_t stats_blocks_scratch_bytes(const Geom &G);
hipError_t launch_stats_blocks(const StreamCall &c, void *d_blk, void *d_sacc, uint32_t head_len, int64_t *d_out, BlkFallbackList *list_out);
// drx_wave_bins (drx_bins.hip): behind the whole batch's walk (tables_ready as above), a lane per waveform that parses and
// reduces bin by bin: row (g, b) = d_out + g * out_wave_stride + b * DRX_BIN_COLS holds the samples of waveform g with index in
// [a + b * bin, a + (b + 1) * bin), a = d_start[g * start_stride] + offset (saturating; d_start == nullptr: 0); every one of
// the n_bins rows of every waveform is written, an empty bin as (0, 0, 32767, -32768).  ev: {start, walk's end, kernel's end, end}
// form_out: DRX_BINS_FORM_* of include/deltarice_hip.h.  bins_impl (drx_ctx): 0 a lane per waveform whatever the batch, 1 the block
// form where blocks_form_batch() admits the batch under kBinsForm: d_list = bins_blocks_scratch_bytes() of list
hipError_t launch_wave_bins(const StreamCall &c, void *d_blk, void *d_list, int bins_impl, const int64_t *d_start, uint64_t start_stride,
                            int64_t offset, uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride, uint32_t *form_out);
uint64_t bins_blocks_scratch_bytes(const Geom &G);
hipError_t launch_bins_blocks(const StreamCall &c, void *d_blk, void *d_list, const int64_t *d_start, uint64_t start_stride, int64_t offset,
                              uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride);
// drx_decode_window (drx_window.hip): behind the whole batch's walk (tables_ready as above), a lane per waveform that parses as
// far as its window's end and writes `width` samples from start[g * start_stride] + offset on (pad outside the waveform) to row
// g of d_out, rows out_stride samples apart.  d_start == nullptr: 0.  ev: {start, walk's end, kernel's end, end}
hipError_t launch_decode_window(const StreamCall &c, const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width,
                                int16_t pad, int16_t *d_out, uint64_t out_stride);
// drx_wave_stack (drx_stack.hip): behind the whole batch's walk (tables_ready as above), the `width` rows of DRX_STACK_COLS int64,
// out_stride elements apart, set to zero; COUNT from the geometry, the origins (as drx_wave_bins takes them) and the selection
// (d_select: uint8[total_waves], nullptr: every waveform) alone; then persistent workgroups of lanes that parse every selected
// waveform as far as its window's end and add SUM and SUMSQ through an accumulator in LDS.  ev: {start, walk's end, kernels' end, end}
// d_list: stack_list_bytes() of scratch where d_select != nullptr (u64 n_listed | u64 listed[W]: the selected waveforms that add
// something, for the delta filter's lanes), which may be nullptr otherwise
inline uint64_t stack_list_bytes(const Geom &G) { return 8u * (G.total_waves + 1u); }
// max_wgs: the context option "stack_workgroups" (0: the resident grid; otherwise at most so many workgroups per tile of positions)
hipError_t launch_wave_stack(const StreamCall &c, void *d_list, uint32_t max_wgs, const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width,
                             const uint8_t *d_select, int64_t *d_out, uint64_t out_stride);
// drx_decode_windows (drx_windows.hip): behind the whole batch's walk (tables_ready as above), a lane per waveform that parses as
// far as the end of its last live window and writes every window slot's row of `width` samples: slot p < min(d_count[g], n_win)
// (d_count == nullptr: every slot) from d_start[g * start_wave_stride + p * start_win_stride] + offset on, pad outside the waveform
// and all over a slot that is not live; row (g, p) = d_out + g * out_wave_stride + p * out_win_stride.
// ev: {start, walk's end, kernels' end, end}
// form_out: DRX_WINDOWS_FORM_* of include/deltarice_hip.h.  The block form: d_wtab = windows_blocks_scratch_bytes() of list
struct WinList;  // drx_window_rows.h
hipError_t launch_decode_windows(const StreamCall &c, void *d_blk, void *d_wtab, const int64_t *d_start, uint64_t start_wave_stride,
                                 uint64_t start_win_stride, const uint32_t *d_count, uint32_t n_win, int64_t offset, uint32_t width,
                                 int16_t pad, int16_t *d_out, uint64_t out_wave_stride, uint64_t out_win_stride, uint32_t *form_out);
uint64_t windows_blocks_scratch_bytes(const Geom &G);
hipError_t launch_windows_blocks(const StreamCall &c, void *d_blk, void *d_wtab, const WinList &wl, BlkFallbackList *list_out);
// drx_find_pulses (drx_pulses.hip): behind the whole batch's walk (tables_ready as above), the output zeroed by one memset, a lane
// per waveform that parses, compares every sample with thr[g * thr_stride] + thr (d_thr == nullptr: 0; neg: below it, otherwise
// above it) and writes the records of the first max_pulses runs of at least min_width samples to int64
// d_out[total_waves][max_pulses][DRX_PULSE_COLS] and the number of all such runs to d_count[total_waves].
// ev: {start, walk's end, kernel's end, end}
// form_out: DRX_PULSES_FORM_* of include/deltarice_hip.h.  The block form: d_ptab = pulses_blocks_scratch_bytes() of block summaries
// and lists, d_pstage = pulses_blocks_staging_bytes(max_pulses) of staged records, which may be nullptr where that is 0
hipError_t launch_find_pulses(const StreamCall &c, void *d_blk, void *d_ptab, void *d_pstage, const int64_t *d_thr, uint64_t thr_stride,
                              int64_t thr, bool neg, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count, int64_t *d_out,
                              uint32_t *form_out);
uint64_t pulses_blocks_scratch_bytes(const Geom &G);
uint64_t pulses_blocks_staging_bytes(const Geom &G, uint32_t max_pulses);
hipError_t launch_pulses_blocks(const StreamCall &c, void *d_blk, void *d_ptab, void *d_pstage, const int64_t *d_thr, uint64_t thr_stride,
                                int64_t thr, bool neg, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count, int64_t *d_out,
                                BlkFallbackList *list_out);
hipError_t launch_estimate_words(const Geom &G, const int16_t *d_in, unsigned long long *d_words16, hipStream_t s);
// k_chunk_scan + k_chunk_offsets (drx_encode_kernels.hip) over a table of n_i that is not an encode's: header positions relative
// to the chunk, chunk offsets, DevStatus::total_words and kErrCapacity against out_cap
hipError_t launch_chunk_offsets(const Geom &G, const uint32_t *d_wave_words, uint32_t *d_wave_rel, uint64_t *d_chunk_words,
                                uint64_t *d_chunk_word_off, uint64_t out_cap, DevStatus *d_status, hipStream_t s);
// drx_transcode / drx_estimate_words_encoded (drx_transcode.hip).  Their scratch, a buffer of the plan: uint64
// chunk_words[n_chunks + 1] | uint64 est[16] | uint32 n_i'[W] | uint32 header positions[W] of the RESULT (the plan's own tables
// describe the source)
struct TrcScratch {
    uint64_t *chunk_words;
    unsigned long long *est;
    uint32_t *words, *rel;
    uint64_t bytes;
};
inline TrcScratch trc_scratch_view(const Geom &G, void *base) {
    const uint64_t W = G.total_waves ? G.total_waves : 1, C = G.n_chunks + 1;
    TrcScratch t;
    t.chunk_words = (uint64_t *)base;
    t.est = (unsigned long long *)(t.chunk_words + C);
    t.words = (uint32_t *)(t.est + 16);
    t.rel = t.words + W;
    t.bytes = (C + 16) * sizeof(uint64_t) + 2 * W * sizeof(uint32_t);
    return t;
}
// Behind the whole batch's walk, a lane per waveform that parses and sizes at RiceParameter 2^k2, the scan above over the new
// table, then a lane per waveform that parses and packs.  out.d_out == nullptr: as far as the offsets.
// ev: {start, walk's end, offsets' end, end}
// form_out: DRX_TRANSCODE_FORM_* of include/deltarice_hip.h.  The block form (drx_transcode_blocks.hip): d_blk = the block
// decoder's scratch, d_tb = trc_blocks_scratch_bytes() of accumulators, list and block-slot table
hipError_t launch_transcode(const StreamCall &c, uint32_t k2, const TrcScratch &t, const EncOut &out, void *d_blk, void *d_tb, uint32_t *form_out);
// drx_estimate_words_encoded: behind the same walk, the words at every k alone (d_est: uint64[16], cleared here).
// ev: {start, walk's end, kernel's end, end}
hipError_t launch_estimate_words_encoded(const StreamCall &c, unsigned long long *d_est, void *d_blk, void *d_tb, uint32_t *form_out);
uint64_t trc_blocks_scratch_bytes(const Geom &G);
// The block form's launches in front of the scan: the blocks' sizes launch and the kernel behind it.  d_est == nullptr: the
// waveforms it keeps have n_i' in t.words / d_out_wave_words and their blocks' bit offsets in the slot table; otherwise they
// have added their words at every k to d_est.  list_out: the waveforms left to k_recode_sizes
hipError_t launch_trc_blocks_sizes(const StreamCall &c, void *d_blk, void *d_tb, uint32_t k2, const TrcScratch &t, uint32_t *d_out_wave_words,
                                   unsigned long long *d_est, BlkFallbackList *list_out);
// ... and behind it (and behind no error): the headers, the words blocks share cleared, and the blocks' pack launch
hipError_t launch_trc_blocks_pack(const StreamCall &c, void *d_blk, void *d_tb, uint32_t k2, const TrcScratch &t, const EncOut &out);
// drx_transcode_filter / drx_estimate_words_encoded_filter (drx_refilter.hip): launch_transcode()'s steps, tables and events with
// the change of filter between the parse and the sink -- the plan's filter is the source's, T the target's (host memory, read
// before the launcher returns).  Always a lane per waveform: form_out = DRX_TRANSCODE_FORM_LANES | _REFILTER, and
// _REFILTER_SERIAL where the pair of filters (or DRX_DBG_REFILTER_SERIAL) takes the serial kernels
struct RefilterTarget {
    uint32_t n_taps;  // 1 .. DRX_MAX_TAPS, taps[0] != 0
    const int32_t *taps;
};
hipError_t launch_refilter(const StreamCall &c, uint32_t k2, const RefilterTarget &T, const TrcScratch &t, const EncOut &out, uint32_t *form_out);
hipError_t launch_estimate_words_refiltered(const StreamCall &c, const RefilterTarget &T, unsigned long long *d_est, uint32_t *form_out);

// wide: fused_wide() as the route decided it.  d_scan: uint64[total_waves + 2] (one look-back entry per workgroup, the ticket behind them)
hipError_t launch_encode_fused(const EncodeCall &c, int wide, uint64_t *d_scan);

// the persistent form of the single pass (drx_encode_stream.hip): a ring of kEsRingWords LDS words per wavefront, a scanner
// wavefront.  d_scan: uint64[2 * tickets + 32], tickets <= total_waves (32 words of control)
constexpr uint32_t kEsRingWords = 2496;
constexpr uint64_t kEsMinUnits = 8192;  // waveforms (segments) from which the persistent forms suit a batch: its 4096 wavefronts a few each
hipError_t launch_encode_stream(const EncodeCall &c, uint64_t *d_scan);

// ... and its form for LONG waveforms (k_encode_stream_segs): the unit a wavefront codes into its ring is a SEGMENT of a
// waveform, a ticket is kEsSegWaves consecutive segments of ONE waveform, places are bit positions.
// d_scan: uint64[3 * tickets + 32], tickets = total_waves x es_seg_shape().tpw.  The shape is a function of WaveformLength and
// the segment length the caller aims at (what a ring holds with room for most of the next segment, from the bits per sample
// the plan expects).
constexpr uint32_t kEsSegWaves = 4;
constexpr uint32_t kEsSegMinLen = 1024, kEsSegMaxLen = 7168;  // samples per segment the host may aim at
struct EsSegShape { uint32_t seg_len, nseg, tpw; };           // samples per segment (a multiple of 8), segments and tickets per waveform
__host__ __device__ inline EsSegShape es_seg_shape(uint32_t L, uint32_t seg_target) {
    EsSegShape sh;
    uint32_t n = (L + seg_target - 1u) / seg_target;
    n = n ? n : 1u;
    // whole tickets: fewer, longer segments or more, shorter ones -- whichever costs less.  Measured on 50 chunks of 14 M samples
    // (profiles/r04_notes.md section 10): segments 17 % above the target (a ring then holds little of the next one) +9.5 %, 22 %
    // below it (a ticket's fixed costs per fewer samples) +9 %, 41 % below +16 %; never above 67 / 57 of the target (what
    // k_encode_stream accepts of a ring, stream_encoder_suits()).
    const uint32_t dn = n / kEsSegWaves * kEsSegWaves, up = (n + kEsSegWaves - 1u) / kEsSegWaves * kEsSegWaves;
    n = up;
    if (dn && dn != up) {
        const uint64_t sd = (L + dn - 1u) / dn, su = (L + up - 1u) / up;  // (sd > seg_target >= su)
        const uint64_t pen_dn = sd > seg_target ? (sd - seg_target) * 55u : 0u, pen_up = su < seg_target ? (seg_target - su) * 40u : 0u;
        if (sd * 57u <= (uint64_t)seg_target * 67u && pen_dn < pen_up) n = dn;
    }
    sh.seg_len = (((L + n - 1u) / n) + 7u) & ~7u;                     // equal segments, 16-byte steps
    sh.nseg = (L + sh.seg_len - 1u) / sh.seg_len;
    sh.tpw = (sh.nseg + kEsSegWaves - 1u) / kEsSegWaves;
    return sh;
}
// the segment form can run the batch: uniform, delta or a forward filter of up to four taps, tickets of the shortest segments
// below 2^32 - 2^16; it is the default choice from kEsSegsFromLen on (16 384: k_encode_pieces 0.61 ms, this 0.66; 24 000: 0.69 / 0.61)
inline bool stream_segs_admits(const Geom &G) { return G.uniform && (G.n_taps == 0 || G.enc_fast) && G.u_wave_len >= 64u &&
                                                       G.total_waves * es_seg_shape(G.u_wave_len, kEsSegMinLen).tpw < 0xffff0000ull; }
constexpr uint32_t kEsSegsFromLen = 20480;
inline uint64_t segs_scan_words(const Geom &G, uint32_t seg_target) { return 3 * G.total_waves * es_seg_shape(G.u_wave_len, seg_target).tpw + 192; }
hipError_t launch_encode_stream_segs(const EncodeCall &c, uint32_t seg_target, uint64_t *d_scan);

// few long waveforms (WaveformLength = -1): a wavefront per 8192-sample segment, see drx_encode_kernels.hip.  Admission (the
// encoder can run the batch) and preference (it is the default choice)
bool long_batch_admits(const Geom &G);
bool long_batch(const Geom &G);
uint64_t long_batch_units(const Geom &G);
// ragged plans: sets seg_units and returns seg_unit_base's host copy (empty: the encoder does not take the batch)
std::vector<uint64_t> segments_plan_ragged(Geom &G, const ChunkDesc *host_chunks);
hipError_t launch_encode_long(const EncodeCall &c, uint32_t *d_wave_rel, uint64_t *d_chunk_words, uint32_t *d_seg_bits,
                              uint64_t *d_seg_pos);

// a second stream of the context, for kernels of one call that do not depend on each other (fork / join through events).
// One per CONTEXT, shared by all its plans: it relies on the rule of include/deltarice_hip.h that a context and its plans are
// driven by one thread at a time (a second thread decoding another plan of the same context would re-record fork / join
// in the middle of this call).  Every path out of launch_decode() after the fork joins, or synchronises the side stream.
struct SideStream {
    hipStream_t s;
    hipEvent_t fork, join;
};
// path_out (optional): which decoders the call used, DRX_PATH_* bits of include/deltarice_hip.h
hipError_t launch_decode(const StreamCall &c, int16_t *d_out, uint64_t *d_granules, int impl, void *d_blk, const SideStream *side,
                         uint32_t *path_out = nullptr);
// block-parallel decoder for batches of few waveforms (drx_blocks.hip): a workgroup per block of a waveform's stream
bool blocks_batch(const Geom &G, double lane_us = 0.06, bool any_filter = false);  // any_filter: no test of the plan's filter
// ragged plans: decides rag_blocks / rag_blk_nt / rag_blk_slots and the classes from the host's chunk table (call once, when
// the plan is made); returns rag_blk_list's host copy (empty: the decoder does not take the batch)
std::vector<uint32_t> blocks_plan_ragged(Geom &G, const ChunkDesc *host_chunks);
uint64_t blocks_scratch_bytes(const Geom &G);
uint64_t blocks_total_slots(const Geom &G);  // look-back slots of the whole batch: every waveform's blocks at 25 bits per sample
// resid: leave the residuals (not their running sums) in d_out: a general prediction filter's inverse follows (launch_iir)
// fused_out: a general filter's inverse ran inside the kernel (no k_iir_tiles pass is needed behind it)
hipError_t launch_decode_blocks(const StreamCall &c, void *d_blk, int16_t *d_out, const uint32_t **fail_out,
                                const uint32_t **suspect_out, bool resid, bool *fused_out);
// ... and for the other kernels of its scheme (drx_blocks.h; k_stats_blocks): the scratch's tables, and what one launch -- a
// uniform batch, or one length class of a ragged one -- is given.  blocks_prepare() resets the scratch on the stream, chooses
// the delta filter's geometry as launch_decode_blocks() does and has launched k_blk_max for every entry's info words.
constexpr uint32_t kBlkMaxClasses = 32;  // ragged batches: one launch per class of WaveformLengths floor(log2 L)
struct BlkTables {
    uint32_t *fail, *suspect, *ends;
    uint64_t *state;
};
struct BlkClassLaunch {
    uint32_t *info;        // {most blocks of a waveform, tickets, the launch's ticket word, -}
    const uint32_t *list;  // the launch's waveforms (nullptr: all of the batch)
    uint32_t n_waves;
    int nt, sw;            // lanes per block, words per lane
    uint32_t spw, run_len; // look-back slots per waveform, blocks per ticket
    unsigned grid;         // resident workgroups
};
// The kernels of the scheme are templates over both: f(lanes per block, words per lane) as std::integral_constant tags
template <class F> inline void blk_dispatch(int nt, int sw, F f) {
    auto by_sw = [&](auto nt_tag) {
        switch (sw) {
            case 9: f(nt_tag, std::integral_constant<int, 9>{}); break;
            case 11: f(nt_tag, std::integral_constant<int, 11>{}); break;
            case 15: f(nt_tag, std::integral_constant<int, 15>{}); break;
            default: f(nt_tag, std::integral_constant<int, 19>{}); break;
        }
    };
    if (nt == 64) by_sw(std::integral_constant<int, 64>{});
    else if (nt == 128) by_sw(std::integral_constant<int, 128>{});
    else by_sw(std::integral_constant<int, 256>{});
}
hipError_t blocks_prepare(const Geom &G, uint64_t in_words, const uint32_t *d_wave_words, void *d_blk, hipStream_t s, BlkTables *T,
                          BlkClassLaunch *launches, uint32_t *n_launches);
uint32_t blocks_iir_tab_words();
void blocks_iir_tables(const uint32_t fast_nt[3], uint32_t t0neg, uint32_t *tab);
// single-pass encoder for short and long waveforms (drx_pieces.hip): a wavefront takes a PIECE, either a run of whole
// short waveforms or one segment of a long one; the pieces of a chunk fill whole workgroups of kPcWaves wavefronts
constexpr uint32_t kPcWaves = 8;
constexpr uint32_t kPcRunSamples = 7168;  // samples of a run of short waveforms (9.1 bits per sample fit the LDS buffer)
constexpr uint32_t kPcMaxRun = 16;        // waveforms of a run
constexpr uint32_t kPcSegSamples = 8192;  // most samples of a segment
constexpr uint32_t kPcWholeLen = 10240;   // WaveformLengths up to here stay whole (6.4 bits per sample fit the buffer)
constexpr uint32_t kPcMinLen = 64;        // WaveformLengths it takes: from here
// A piece's code must fit its wavefront's 2048-word LDS buffer, or the piece is coded a second time, tile by tile, straight
// to its place (6 x slower: NOPTREX at sigma = 40, m = 32 -- 8.5 bits per sample -- encoded in 5.7 ms instead of 0.93; the
// headline shape at sigma = 80, m = 64 in 2.2 ms per 100 chunks instead of 1.25).  With the RiceParameter that suits the data a
// sample takes about k + 3.5 bits, so the pieces are sized for k + 4.5: the constants above are the measured geometry for
// k <= 3 (m <= 8), beyond that a segment holds 131072 / (2 k + 9) samples in whole tiles.
__host__ __device__ inline uint32_t pc_seg_samples(uint32_t k) {
    if (k <= 3u) return kPcSegSamples;
    const uint32_t s = (131072u / (2u * k + 9u)) & ~511u;
    return s < 512u ? 512u : s;
}
__host__ __device__ inline uint32_t pc_run_samples(uint32_t k) { return k <= 3u ? kPcRunSamples : pc_seg_samples(k) - 512u; }
// a waveform stays whole (one wavefront, and k_encode_fused's range stays k_encode_fused's) while it fits at k + 4 bits per
// sample: two segments of 3500 samples cost a quarter of the rate (100 chunks of 2000 x 7000, sigma = 40, m = 32: 1.84 against 1.26 ms)
__host__ __device__ inline uint32_t pc_whole_len(uint32_t k) { return k <= 3u ? kPcWholeLen : 65536u / (k + 4u); }
__host__ __device__ inline uint32_t pc_max_len(uint32_t k) { return pc_seg_samples(k) * kPcWaves; }  // beyond: several workgroups per waveform
struct PieceShape {
    uint32_t run;      // waveforms per piece (> 1: runs of short waveforms)
    uint32_t segs;     // pieces per waveform and workgroup (a power of two <= kPcWaves; > 1: long waveforms)
    uint32_t parts;    // workgroups per waveform (> 1: waveforms longer than kPcMaxLen, kPcWaves segments per workgroup)
    uint32_t seg_len;  // samples per segment (a multiple of 512)
    uint32_t pieces;   // of the chunk
    uint32_t wgs;      // workgroups of the chunk
};
// waveforms of fewer than 512 samples, a multiple of 8 (a lane's 8 samples never straddle two waveforms): PACKED runs, whose
// tiles span waveform boundaries
__host__ __device__ inline bool piece_packable(uint32_t L) { return L >= 8u && L < 512u && (L & 7u) == 0u; }
__host__ __device__ inline PieceShape piece_shape(uint32_t L, uint32_t W, uint32_t k, bool packed) {
    PieceShape s;
    s.parts = 1u;
    const uint32_t run_samples = pc_run_samples(k), seg_samples = pc_seg_samples(k), max_len = pc_max_len(k);
    if (packed) {
        // as many waveforms as fill ~7000 samples AND leave the 2048-word buffer room at 9 (k + 6) bits per sample + a header each
        const uint32_t bits = k <= 3u ? 9u : k + 6u;
        uint32_t by_samples = run_samples / L, by_words = 2000u / (1u + (bits * L + 31u) / 32u);
        by_samples = by_samples ? by_samples : 1u;
        by_words = by_words ? by_words : 1u;
        s.run = by_samples < by_words ? by_samples : by_words;
        s.segs = 1u;
        s.seg_len = L;
        s.pieces = (W + s.run - 1u) / s.run;
        s.wgs = (s.pieces + kPcWaves - 1u) / kPcWaves;
    } else if (L <= run_samples / 2u) {
        s.run = run_samples / L < kPcMaxRun ? run_samples / L : kPcMaxRun;
        s.segs = 1u;
        s.seg_len = L;
        s.pieces = (W + s.run - 1u) / s.run;
        s.wgs = (s.pieces + kPcWaves - 1u) / kPcWaves;
    } else if (L <= max_len) {
        const uint32_t need = L <= pc_whole_len(k) ? 1u : (L + seg_samples - 1u) / seg_samples;
        s.run = 1u;
        s.segs = 1u;
        while (s.segs < need) s.segs <<= 1;
        s.seg_len = s.segs == 1u ? L : ((((L + s.segs - 1u) / s.segs) + 511u) & ~511u);
        s.pieces = W * s.segs;
        s.wgs = (s.pieces + kPcWaves - 1u) / kPcWaves;
    } else {
        // a waveform over several workgroups ("parts"): kPcWaves segments each, as even as whole tiles allow (full 8192-sample
        // segments with a short last part instead were measured slower: nEDM 0.90 against 0.77 ms)
        s.run = 1u;
        s.segs = kPcWaves;
        s.parts = (uint32_t)(((uint64_t)L + max_len - 1u) / max_len);
        const uint32_t per_part = (uint32_t)(((uint64_t)L + s.parts - 1u) / s.parts);
        s.seg_len = (((per_part + kPcWaves - 1u) / kPcWaves) + 511u) & ~511u;
        s.pieces = 0u;  // (not used: every workgroup of the chunk is full)
        s.wgs = W * s.parts;  // (the plan checks that this fits 31 bits)
    }
    return s;
}
// k_encode_fused's own range of WaveformLengths (uniform batches), a RiceParameter beyond the measured geometry, and a waveform
// that would not stay whole in the standard 2048-word buffer: larger buffers, fewer waveforms per workgroup --
// 1 = 8 waveforms x 2496 words, 2 = 4 x 3072, 3 = 4 x 4096 -- where the waveform fits at k + 4.4 bits per sample; 0 = the
// standard geometry (or, beyond all of them, the pieces encoder's segments).  100 chunks of 2000 x 7000, sigma = 80, m = 64
// (9.5 bits per sample): coded twice 2.17 ms, two segments 1.87, 4 x 3072 1.56, 8 x 3072 (one workgroup per CU) 1.64, 6 x 3072 2.08.
constexpr uint32_t kEncWide1Words = 2496, kEncWide2Words = 3072, kEncWide3Words = 4096;
inline int fused_wide(const Geom &G) {
    if (!G.uniform || G.k <= 3u) return 0;
    const uint32_t L = G.u_wave_len;
    if (L <= kPcRunSamples / 2u || L > kPcWholeLen || L <= pc_whole_len(G.k)) return 0;
    const uint64_t bits10 = (uint64_t)L * (10u * G.k + 44u);
    return bits10 <= 320ull * kEncWide1Words ? 1 : (bits10 <= 320ull * kEncWide2Words ? 2 : (bits10 <= 320ull * kEncWide3Words ? 3 : 0));
}
bool pieces_admits(const Geom &G);            // the encoder can run the batch (delta or a forward filter of up to four taps)
bool pieces_batch(const Geom &G, int wide);   // ... and is its default choice
uint64_t pieces_workgroups(const Geom &G);     // uniform batches it admits
// ragged plans: sets pc_super / pc_packed and returns pc_wg_base's host copy, whose last entry is the workgroup total (empty:
// the encoder does not take the batch)
std::vector<uint32_t> pieces_plan_ragged(Geom &G, const ChunkDesc *host_chunks);
uint64_t pieces_scan_words(const Geom &G, uint64_t total_wgs);  // uint64 words of its look-back state, the two of its ticket included
hipError_t launch_encode_pieces(const EncodeCall &c, uint64_t in_samples, uint64_t *d_scan, uint64_t total_wgs);
// in-place inverse of a general prediction filter over decoded residuals (drx_iir.hip): tiles of kIirThreads lanes x kIirRun
// samples, decoupled look-back over kIirWin tiles per poll (drx_lookback.h: its window), tables of kIirTabWords uint32 per filter;
// d_state: uint64[n_tiles + 1], the ticket in the last word
constexpr uint32_t kIirRun = 64, kIirThreads = 512, kIirTile = kIirRun * kIirThreads, kIirWin = 128;
constexpr uint32_t kIirTabWords = (7 + 64 + (kIirWin + 1)) * 9 + 4;
void iir_tables(const uint32_t fast_nt[3], uint32_t t0neg, uint32_t *tab);
uint64_t iir_tiles(const Geom &G, const ChunkDesc *host_chunks, uint64_t *chunk_tile_base);  // (chunk_tile_base: n_chunks + 1, ragged only)
hipError_t launch_iir(const Geom &G, const uint64_t *d_chunk_tile_base, uint64_t n_tiles, const uint32_t *d_tab, uint64_t *d_state,
                      const uint32_t *d_skip, DevStatus *d_status, int16_t *d_out, hipStream_t s);
// ragged plans: sets max_groups, max_wave_len64, rag_groups / rag_groups_long; returns rag_order's host copy (empty: more
// wavefronts than 31 bits count)
std::vector<uint2> decode_plan_ragged(Geom &G, const ChunkDesc *host_chunks);

}  // namespace drx
#endif
