// drx_windows_blocks.hip -- drx_decode_windows for few long waveforms: a WORKGROUP per block of a waveform's stream.
//
// A lane per waveform (k_decode_windows, drx_windows.hip) takes about 50 ns per sample whatever else runs, and a window deep in a
// long trace costs the whole trace in front of it.  The batches that drx_wave_stats gives to its block form
// (blocks_form_batch() under kWindowsForm) take this form:
//
//   k_windows_pads           every row of the call, whole, is filled with `pad`: the blocks overwrite what the windows hold of
//                            their waveforms.
//   k_windows_blocks         the block decoder's phase 1, look-back and flags, word for word (drx_blocks_body.inc), and the decoder's
//                            phase 2 under `if constexpr (WINDOWS)`: once a block knows its first sample and how many it holds,
//                            the workgroup decides as one whether any live window of its waveform meets them.  If none does the
//                            block is done -- no reorder, no store: sparse pulses cost the parse alone.  Otherwise the samples are
//                            put in output order in LDS as the decoder puts them (its second-parse path included), and in place of
//                            the copy to a decoded batch every window that meets the staged range receives its share of it.
//   k_windows_blocks_finish  a thread per waveform: one that is flagged or suspect goes on a list on the device.
// Listed waveforms are written again -- all their rows -- and JUDGED by k_decode_windows_list (drx_windows.hip), the delta filter's
// lane kernel over that list, which parses to e_g and no further: a waveform damaged only behind its last window is suspect here
// (the blocks parse every waveform to its end) and ends with the lane form's verdict.  Noise and quiet data are never flagged.
// Delta filter only, as the block decoder's phase 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_blocks.h"

namespace drx {

template <int NT, int SW>
__global__ __launch_bounds__(NT) void k_windows_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                       const uint64_t *__restrict__ wave_off,
                                                       const uint32_t *__restrict__ wave_words,
                                                       const uint32_t *__restrict__ info, uint32_t slots_per_wave,
                                                       uint32_t run_len, uint64_t *__restrict__ state,
                                                       uint32_t *__restrict__ ends, uint32_t *__restrict__ ticket,
                                                       uint32_t *__restrict__ fail, uint32_t *__restrict__ suspect,
                                                       DevStatus *st, BlkWindowArgs wa, uint32_t n_list,
                                                       const uint32_t *__restrict__ wave_list) {
    constexpr bool RESID = false, FUSE = false, STATS = false, PULSES = false, WINDOWS = true, TRANSCODE = false, BINS = false;
    // what the decoder's copy-out, its fused inverse filter, the statistics and the pulse form take: not used here
    int16_t *const out = nullptr;
    const uint32_t *const itab = nullptr;
    uint64_t *const xstate = nullptr;
    const BlkStatsArgs sa{0u, nullptr};
    const BlkPulseArgs pa{};
    const BlkTrcArgs ta{};
    const BlkBinsArgs ba{};
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
#include "drx_blocks_body.inc"
}

// Every row of the call = pad.  A workgroup per row (rows beyond the grid by a stride): 2-byte stores, a wavefront's next to one
// another.  Row addressing is 64-bit.
__global__ __launch_bounds__(256) void k_windows_pads(uint64_t total_waves, WinList wl, uint32_t *__restrict__ n_listed,
                                                      const DevStatus *st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_listed = 0u;
    if (st->err) return;
    const uint64_t rows = total_waves * (uint64_t)wl.n_win;
    for (uint64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint64_t g = r / wl.n_win;
        int16_t *row = wl.row(g, (uint32_t)(r - g * wl.n_win));
        for (uint32_t j = threadIdx.x; j < wl.width; j += 256u) row[j] = (int16_t)wl.pad2;
    }
}

// A thread per waveform: flagged or suspect waveforms, and those no block has judged (samples and no payload word), go on the
// list of the lane kernel behind this one.  all_listed: DRX_DBG_WINDOWS_ALL_FALLBACK.
__global__ __launch_bounds__(256) void k_windows_blocks_finish(Geom G, const uint32_t *__restrict__ wave_words,
                                                               const uint32_t *__restrict__ fail, const uint32_t *__restrict__ suspect,
                                                               uint32_t all_listed, uint32_t *__restrict__ n_listed,
                                                               uint32_t *__restrict__ listed, const DevStatus *st) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (st->err) return;  // (as k_windows_blocks)
    if (g >= G.total_waves) return;
    if (blk_listed(all_listed, fail, suspect, g, [&] { return wave_words[g] == 0u && locate(G, g).len != 0u; }))
        blk_list_append(n_listed, listed, (uint32_t)g);
}

// the plan's scratch of this form: the fallback list
uint64_t windows_blocks_scratch_bytes(const Geom &G) { return BlkFallbackList::bytes(G.total_waves); }

// k_windows_pads, k_windows_blocks per launch of the block scheme, then k_windows_blocks_finish.  The block decoder's scratch is
// used as the decoder uses it (calls on a plan are ordered on one stream) and reset on the stream first; d_wtab is the plan's
// scratch of this form.  list_out: the device list of the waveforms left to the lane kernel.
hipError_t launch_windows_blocks(const StreamCall &call, void *d_blk, void *d_wtab, const WinList &wl, BlkFallbackList *list_out) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    const BlkFallbackList A = BlkFallbackList::at(d_wtab);
    const uint64_t rows = G.total_waves * (uint64_t)wl.n_win;
    k_windows_pads<<<(unsigned)(rows < (1ull << 20) ? rows : (1ull << 20)), 256, 0, s>>>(G.total_waves, wl, A.n_listed, call.d_status);
    BlkTables T;
    BlkClassLaunch cls[kBlkMaxClasses];
    uint32_t n_cls = 0;
    const hipError_t e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls);
    if (e != hipSuccess) return e;
    const BlkWindowArgs wa{wl};
    for (uint32_t i = 0; i < n_cls; ++i) {
        const BlkClassLaunch &c = cls[i];
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            k_windows_blocks<NT, SW><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw, c.run_len,
                                                           T.state, T.ends, c.info + 2, T.fail, T.suspect, call.d_status, wa, c.n_waves, c.list);
        });
    }
    k_windows_blocks_finish<<<blocks_for(G.total_waves, 256), 256, 0, s>>>(G, call.d_wave_words, T.fail, T.suspect,
                                                                           (G.dbg & kWindowsForm.all_fallback_flag) ? 1u : 0u, A.n_listed, A.listed,
                                                                           call.d_status);
    *list_out = A;
    return hipGetLastError();
}

}  // namespace drx
