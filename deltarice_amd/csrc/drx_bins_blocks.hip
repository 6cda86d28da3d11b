// drx_bins_blocks.hip -- drx_wave_bins for few long waveforms: a WORKGROUP per block of a waveform's stream.
//
// A lane per waveform (k_wave_bins, drx_bins.hip) takes 57 ns per sample whatever else runs, and the reference's default options
// (one waveform per chunk) keep a few dozen of the chip's lanes busy.  Under the context option "bins_impl" = 1 the batches that
// drx_wave_stats gives to its block form (blocks_form_batch() under kBinsForm) take this form:
//
//   k_bins_fill           every one of the call's total_waves x n_bins rows = the identity (0, 0, 32767, -32768): the caller's rows
//                         are the accumulators of the blocks.  Nothing between the rows of different waveforms is written.
//   k_bins_blocks         the block decoder's phase 1, look-back and flags, word for word (drx_blocks_body.inc).  Phase 2
//                         (drx_blocks_bins.inc): once a lane knows the index of its first sample, how many of its codes are samples
//                         and the running sum in front of them, it reduces its samples bin by bin -- from the running sums phase 1
//                         staged, or, where some lane holds more codes than its share of the staging buffer, from a second parse --
//                         and the block merges the partial rows into the caller's with 64-bit integer atomics (add, add, signed
//                         min, signed max: the same answer in any order), reduced on chip first: by shuffles where the block lies
//                         in one bin, in an LDS table where it meets up to a few hundred.  Where it meets more (bins of a few
//                         samples) every lane sends its partial rows to memory itself: correct, NOT tuned -- as the lane kernel's
//                         bin < 16 is not.
//   k_bins_blocks_finish  a thread per waveform: one that is flagged or suspect goes on a list on the device.
//   k_wave_bins_list      a lane per listed waveform: serial_frame() (drx_lane_stream.h), every one of the waveform's rows written
//                         again by plain stores, and the waveform JUDGED.  Correct and slow: a flagged 14 M-sample waveform costs
//                         here what it costs a lane.  Noise and quiet data are never flagged.
// Delta filter only, as the block decoder's phase 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_blocks.h"
#include "drx_lane_stream.h"

namespace drx {

template <int NT, int SW>
__global__ __launch_bounds__(NT) void k_bins_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                    const uint64_t *__restrict__ wave_off,
                                                    const uint32_t *__restrict__ wave_words,
                                                    const uint32_t *__restrict__ info, uint32_t slots_per_wave,
                                                    uint32_t run_len, uint64_t *__restrict__ state,
                                                    uint32_t *__restrict__ ends, uint32_t *__restrict__ ticket,
                                                    uint32_t *__restrict__ fail, uint32_t *__restrict__ suspect,
                                                    DevStatus *st, BlkBinsArgs ba, uint32_t n_list,
                                                    const uint32_t *__restrict__ wave_list) {
    constexpr bool RESID = false, FUSE = false, STATS = false, PULSES = false, WINDOWS = false, TRANSCODE = false, BINS = true;
    // what the decoder's phase 2, its fused inverse filter and the other forms take: not used here
    int16_t *const out = nullptr;
    const uint32_t *const itab = nullptr;
    uint64_t *const xstate = nullptr;
    const BlkStatsArgs sa{0u, nullptr};
    const BlkPulseArgs pa{};
    const BlkWindowArgs wa{};
    const BlkTrcArgs ta{};
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
#include "drx_blocks_body.inc"
}

// a row by 8-byte stores (the ABI asks 8-byte alignment of d_out)
__device__ __forceinline__ void bins_store_row(int64_t *row, int64_t sum, uint64_t sq, int32_t mn, int32_t mx) {
    static_assert(DRX_BIN_SUM == 0 && DRX_BIN_SUMSQ == 1 && DRX_BIN_MIN == 2 && DRX_BIN_MAX == 3 && DRX_BIN_COLS == 4, "the row's order");
    row[0] = sum;
    row[1] = (int64_t)sq;
    row[2] = mn;
    row[3] = mx;
}

// Every row of the call = the identity.  A thread per row (rows beyond the grid by a stride); row addressing is 64-bit.
__global__ __launch_bounds__(256) void k_bins_fill(uint64_t total_waves, uint32_t n_bins, int64_t *__restrict__ rows, uint64_t wave_stride,
                                                   uint32_t *__restrict__ n_listed, const DevStatus *st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_listed = 0u;
    if (st->err) return;
    const uint64_t n_rows = total_waves * (uint64_t)n_bins;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t g = r / n_bins;
        bins_store_row(rows + g * wave_stride + (r - g * n_bins) * (uint64_t)DRX_BIN_COLS, 0, 0u, 32767, -32768);
    }
}

// A thread per waveform: flagged or suspect waveforms, and those no block has judged (samples and no payload word), go on the
// list of the lane kernel behind this one.  all_listed: DRX_DBG_BINS_ALL_FALLBACK.
__global__ __launch_bounds__(256) void k_bins_blocks_finish(Geom G, const uint32_t *__restrict__ wave_words,
                                                            const uint32_t *__restrict__ fail, const uint32_t *__restrict__ suspect,
                                                            uint32_t all_listed, uint32_t *__restrict__ n_listed,
                                                            uint32_t *__restrict__ listed, const DevStatus *st) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (st->err) return;  // (as k_bins_blocks)
    if (g >= G.total_waves) return;
    if (blk_listed(all_listed, fail, suspect, g, [&] { return wave_words[g] == 0u && locate(G, g).len != 0u; }))
        blk_list_append(n_listed, listed, (uint32_t)g);
}

// The waveforms list[0 .. *n_list): a lane each, the serial parse, every row of the waveform by plain stores (what the blocks
// merged into them is overwritten), the verdict.  The list and its length are written on the device by the kernel in front; the
// launch is sized for the whole batch.  Lane 0 of the launch leaves the list's length in the status word for
// drx_plan_last_bins_listed.
__global__ __launch_bounds__(64) void k_wave_bins_list(Geom G, const uint32_t *__restrict__ in, const uint64_t *__restrict__ wave_off,
                                                       const uint32_t *__restrict__ wave_words, BlkBinsArgs ba, DevStatus *st,
                                                       const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->listed = *n_list;
    BinCursor c = {kNoBorder, 0u, false};
    int64_t *rows = nullptr;
    int32_t mn = 32767, mx = -32768;
    int64_t sum = 0;
    uint64_t sq = 0;
    uint32_t len = 0;
    auto empty = [&](uint32_t from, uint32_t to) __attribute__((always_inline)) {
        for (uint32_t b = from; b < to; ++b) bins_store_row(rows + (uint64_t)b * (uint64_t)DRX_BIN_COLS, 0, 0u, 32767, -32768);
    };
    serial_frame(
        G, in, wave_off, wave_words, 0, list, (uint64_t)*n_list, st,
        [&](uint64_t g, const WaveRef &r) __attribute__((always_inline)) {
            len = r.len;
            rows = ba.rows + g * ba.wave_stride;
            empty(0u, bins_begin(c, bins_origin(ba.start, ba.start_stride, ba.offset, g), ba.bin, ba.n_bins, len, 0u));
            return len;
        },
        [&](uint32_t i, int16_t y16) __attribute__((always_inline)) {
            if (i == c.nb) {
                if (c.live) bins_store_row(rows + (uint64_t)c.cur * (uint64_t)DRX_BIN_COLS, sum, sq, mn, mx);
                bins_border(c, ba.bin, ba.n_bins, len);
                sum = 0;
                sq = 0;
                mn = 32767;
                mx = -32768;
            }
            const int32_t y = y16;
            sum += y;
            sq += (uint64_t)(uint32_t)(y * y);
            mn = y < mn ? y : mn;
            mx = y > mx ? y : mx;
        },
        [&](uint64_t, const WaveRef &) __attribute__((always_inline)) {
            if (c.live) bins_store_row(rows + (uint64_t)c.cur * (uint64_t)DRX_BIN_COLS, sum, sq, mn, mx);
            empty(c.cur + (c.live ? 1u : 0u), ba.n_bins);
        });
}

// the plan's scratch of this form: the fallback list
uint64_t bins_blocks_scratch_bytes(const Geom &G) { return BlkFallbackList::bytes(G.total_waves); }

// On the stream: k_bins_fill, k_bins_blocks per launch of the block scheme, k_bins_blocks_finish, k_wave_bins_list.  The block
// decoder's scratch is used as the decoder uses it (calls on a plan are ordered on one stream) and reset on the stream first;
// d_list is the plan's scratch of this form.
hipError_t launch_bins_blocks(const StreamCall &call, void *d_blk, void *d_list, const int64_t *d_start, uint64_t start_stride, int64_t offset,
                              uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    const BlkFallbackList A = BlkFallbackList::at(d_list);
    const BlkBinsArgs ba{d_start, start_stride, offset, bin, n_bins, d_out, out_wave_stride};
    const uint64_t fill_blocks = (G.total_waves * (uint64_t)n_bins + 255u) / 256u;
    k_bins_fill<<<(unsigned)(fill_blocks < (1ull << 20) ? fill_blocks : (1ull << 20)), 256, 0, s>>>(G.total_waves, n_bins, d_out, out_wave_stride,
                                                                                                   A.n_listed, call.d_status);
    BlkTables T;
    BlkClassLaunch cls[kBlkMaxClasses];
    uint32_t n_cls = 0;
    const hipError_t e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls);
    if (e != hipSuccess) return e;
    for (uint32_t i = 0; i < n_cls; ++i) {
        const BlkClassLaunch &c = cls[i];
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            k_bins_blocks<NT, SW><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw, c.run_len,
                                                        T.state, T.ends, c.info + 2, T.fail, T.suspect, call.d_status, ba, c.n_waves, c.list);
        });
    }
    k_bins_blocks_finish<<<blocks_for(G.total_waves, 256), 256, 0, s>>>(G, call.d_wave_words, T.fail, T.suspect,
                                                                        (G.dbg & kBinsForm.all_fallback_flag) ? 1u : 0u, A.n_listed, A.listed,
                                                                        call.d_status);
    k_wave_bins_list<<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, call.d_in, call.d_wave_off, call.d_wave_words, ba, call.d_status, A.listed,
                                                                  A.n_listed);
    return hipGetLastError();
}

}  // namespace drx
