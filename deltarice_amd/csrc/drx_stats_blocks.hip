// drx_stats_blocks.hip -- drx_wave_stats for few long waveforms: a WORKGROUP per block of a waveform's stream.
//
// A lane per waveform (k_wave_stats, drx_stats.hip) parses 17 samples per microsecond whatever else runs; 2048 waveforms of
// 500 000 samples keep 2048 of the chip's 98 304 lane slots busy, and the reference's default options (one waveform per chunk)
// a few dozen.  The batches that drx_decode gives to the block decoder (blocks_batch(), drx_blocks.hip) take this form instead:
//
//   k_stats_blocks         the block decoder's phase 1, look-back and flags, word for word (drx_blocks_body.inc): the block image
//                          in LDS, the run-up and the count parse, settle() with its creep detection, tickets dealt run-major,
//                          the predecessor's end one hop back, {status | count | sum} entries for what lies in front of a
//                          block, fail[] / suspect[], bounded spins that raise kErrInternal.  Phase 2 is replaced: once a lane
//                          knows the index of its first sample, how many of its codes are samples and the running sum in front
//                          of them, it reduces its samples -- from the running sums phase 1 staged, or, where some lane holds
//                          more codes than its share of the staging buffer, from a second parse -- and the block folds the
//                          result into the waveform's 48-byte accumulator with six 64-bit integer atomics (keys that order by
//                          value, then by the earliest index; integer atomics give the same answer in any order).  No sample
//                          is put in output order or stored.
//   k_stats_blocks_finish  a thread per waveform: the accumulator unpacked into the caller's row, or -- the waveform is flagged
//                          or suspect -- its index appended to a list on the device.
// Listed waveforms are computed again, and JUDGED, by k_wave_stats_serial (drx_stats.hip) given that list: a lane per waveform,
// correct and slow -- a flagged 14 M-sample waveform costs there what it cost before this form existed.  Noise and quiet data
// are never flagged; a stream whose block had to correct its start after it published its end is.
// Delta filter only, as the block decoder's phase 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_blocks.h"

namespace drx {

template <int NT, int SW>
__global__ __launch_bounds__(NT) void k_stats_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                     const uint64_t *__restrict__ wave_off,
                                                     const uint32_t *__restrict__ wave_words,
                                                     const uint32_t *__restrict__ info, uint32_t slots_per_wave,
                                                     uint32_t run_len, uint64_t *__restrict__ state,
                                                     uint32_t *__restrict__ ends, uint32_t *__restrict__ ticket,
                                                     uint32_t *__restrict__ fail, uint32_t *__restrict__ suspect,
                                                     DevStatus *st, uint32_t head_len, unsigned long long *__restrict__ acc,
                                                     uint32_t n_list, const uint32_t *__restrict__ wave_list) {
    constexpr bool RESID = false, FUSE = false, STATS = true, PULSES = false, WINDOWS = false, TRANSCODE = false, BINS = false;
    // what the decoder's phase 2 and its fused inverse filter take: not used here
    int16_t *const out = nullptr;
    const uint32_t *const itab = nullptr;
    uint64_t *const xstate = nullptr;
    const BlkStatsArgs sa{head_len, acc};
    const BlkPulseArgs pa{};
    const BlkWindowArgs wa{};
    const BlkTrcArgs ta{};
    const BlkBinsArgs ba{};
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
#include "drx_blocks_body.inc"
}

// the accumulators of a call: nothing seen yet
__global__ __launch_bounds__(256) void k_stats_blocks_reset(uint64_t total_waves, unsigned long long *__restrict__ acc,
                                                            uint32_t *__restrict__ n_listed) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g == 0) *n_listed = 0u;
    if (g >= total_waves) return;
    unsigned long long *a = acc + 6u * g;
    a[0] = (unsigned long long)INT64_MAX;
    a[1] = (unsigned long long)INT64_MIN;
    a[2] = a[3] = a[4] = a[5] = 0ull;
}

// A thread per waveform: its row from its accumulator (the stores of drx_stats.hip's rows), or its place on the list of
// the waveforms that the lane kernel behind this one computes and judges.  all_listed: DRX_DBG_STATS_ALL_FALLBACK.
__global__ __launch_bounds__(256) void k_stats_blocks_finish(uint64_t total_waves, const unsigned long long *__restrict__ acc,
                                                             const uint32_t *__restrict__ fail, const uint32_t *__restrict__ suspect,
                                                             uint32_t all_listed, uint32_t *__restrict__ n_listed,
                                                             uint32_t *__restrict__ listed, const DevStatus *st,
                                                             int64_t *__restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (st->err) return;  // (as k_stats_blocks)
    if (g >= total_waves) return;
    // (a waveform with samples and no payload word is not asked about here, as it is in the other forms)
    if (blk_listed(all_listed, fail, suspect, g)) {
        blk_list_append(n_listed, listed, (uint32_t)g);
        return;
    }
    const unsigned long long *a = acc + 6u * g;
    const uint64_t kmin = a[0], kmax = a[1];
    const int64_t v[DRX_STAT_COLS] = {(int64_t)(int32_t)(uint32_t)(kmin >> 32), (int64_t)(uint32_t)kmin,
                                      (int64_t)(int32_t)(uint32_t)(kmax >> 32), (int64_t)(0x7fffffffu - (uint32_t)kmax),
                                      (int64_t)a[2], (int64_t)a[3], (int64_t)a[4], (int64_t)a[5]};
    // (a row is 64 bytes: every row of a 16-byte aligned buffer is aligned)
    store_i64_row(out + g * (uint64_t)DRX_STAT_COLS, ((uintptr_t)out & 15u) == 0, v);
}

// the plan's scratch of this form: u64 acc[W][6] | the fallback list
struct StatsBlkScratch {
    unsigned long long *acc;
    BlkFallbackList list;
    uint64_t bytes;
};
static StatsBlkScratch stats_blocks_layout(const Geom &G, void *base) {
    StatsBlkScratch L;
    L.acc = reinterpret_cast<unsigned long long *>(base);
    L.list = BlkFallbackList::at(L.acc + 6u * G.total_waves);
    L.bytes = 48u * G.total_waves + BlkFallbackList::bytes(G.total_waves);
    return L;
}
uint64_t stats_blocks_scratch_bytes(const Geom &G) { return stats_blocks_layout(G, nullptr).bytes; }

// k_stats_blocks per launch of the block scheme, then k_stats_blocks_finish.  The block decoder's scratch is used as the decoder
// uses it (calls on a plan are ordered on one stream) and reset on the stream first; d_sacc is the plan's scratch of this form.
// list_out: the device list of the waveforms left to the lane kernel.
hipError_t launch_stats_blocks(const StreamCall &call, void *d_blk, void *d_sacc, uint32_t head_len, int64_t *d_out, BlkFallbackList *list_out) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    const StatsBlkScratch A = stats_blocks_layout(G, d_sacc);
    const unsigned nb = blocks_for(G.total_waves, 256);
    k_stats_blocks_reset<<<nb, 256, 0, s>>>(G.total_waves, A.acc, A.list.n_listed);
    BlkTables T;
    BlkClassLaunch cls[kBlkMaxClasses];
    uint32_t n_cls = 0;
    const hipError_t e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls);
    if (e != hipSuccess) return e;
    for (uint32_t i = 0; i < n_cls; ++i) {
        const BlkClassLaunch &c = cls[i];
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            k_stats_blocks<NT, SW><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw, c.run_len,
                                                         T.state, T.ends, c.info + 2, T.fail, T.suspect, call.d_status, head_len, A.acc, c.n_waves, c.list);
        });
    }
    k_stats_blocks_finish<<<nb, 256, 0, s>>>(G.total_waves, A.acc, T.fail, T.suspect, (G.dbg & kStatsForm.all_fallback_flag) ? 1u : 0u, A.list.n_listed,
                                             A.list.listed, call.d_status, d_out);
    *list_out = A.list;
    return hipGetLastError();
}

}  // namespace drx
