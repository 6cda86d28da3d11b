// drx_blocks.h -- the block-parallel parse shared by the kernels that give a WORKGROUP a block of a waveform's stream
// (not installed): the block geometry, the parse, and (drx_blocks_body.inc) the body of k_decode_blocks (drx_blocks.hip: the samples,
// in output order, to HBM), of k_stats_blocks (drx_stats_blocks.hip: the samples reduced to a waveform's statistics), of
// k_pulses_blocks (drx_pulses_blocks.hip: the runs of samples over a threshold, per block, stitched behind the kernel), of
// k_windows_blocks (drx_windows_blocks.hip: the samples, in output order, to the rows of the windows that meet the block) and of
// k_trc_blocks (drx_transcode_blocks.hip: the residuals sized, then re-coded, at another RiceParameter), and of k_bins_blocks
// (drx_bins_blocks.hip: the samples reduced bin by bin into the caller's rows).
// drx_blocks.hip's head comment describes the scheme.  A kernel that takes this route for another purpose adds its own
// phase 2 behind the same phase 1, look-back and flags, as the STATS and PULSES forms do.
// The host side of such a kernel is shared too: blocks_prepare() (drx_blocks.hip: the scratch reset and one BlkClassLaunch per
// launch of the scheme, from blk_classes()), blk_dispatch() (the NT x SW instantiation of a launch), BlkFormRule with
// blocks_form_batch() / blocks_form_word() (which batches take a call's block form, and its form word), BlkFallbackList (the
// waveforms left to the lane kernel behind the blocks; all drx_internal.h) and, below, blk_listed() / blk_list_append().
#ifndef DRX_BLOCKS_H
#define DRX_BLOCKS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "drx_bin_cursor.h"
#include "drx_device.h"
#include "drx_internal.h"
#include "drx_iir_math.h"
#include "drx_lookback.h"
#include "drx_pulse_runs.h"
#include "drx_window_rows.h"

namespace drx {

// Words per lane (odd: the lanes' windows fall on different banks) and the samples a lane can leave in its share of the
// staging buffer.  A block is a fixed number of BITS and costs about the same whatever it holds, so one geometry for all
// data loses both ways: with 352 bits per lane noisy data (12.75 bits per sample: 27 samples per lane) decoded at 0.18
// instead of 0.25 of the roofline, and quiet data under the reference's default RiceParameter (4 bits per sample: 88
// samples per lane, more than the 76 its share holds, so EVERY block took the second parse) at 0.16.  The class is chosen
// per decode from what the caller states about the stream -- 32 in_words / total_samples bits per sample, so a
// RiceParameter that does not suit the data is covered too -- for ~50 samples per lane with 15 % to spare, and every class
// takes 48-50 dwords of LDS per lane:
//   words per lane        9      11      15      19
//   samples staged       76      76      68      60
//   bits per sample   < 5.4   < 8.2  < 11.7    above
// Plan-time estimates (which decoder a batch takes, lanes per block) assume the class that suits the RiceParameter;
// scratch is sized for the smallest blocks.
constexpr int kBlkSegWMin = 9;
__host__ __device__ constexpr int blk_segw_plan(uint32_t k) { return k <= 4u ? 11 : (k <= 7u ? 15 : 19); }
__host__ __device__ constexpr int blk_segw_bits10(uint64_t b10) { return b10 >= 117u ? 19 : (b10 >= 82u ? 15 : (b10 >= 54u ? 11 : 9)); }
__host__ __device__ constexpr uint32_t blk_lane_cap(int segw) { return segw <= 11 ? 76u : (segw == 15 ? 68u : 60u); }
constexpr uint32_t kBlkPre = 8;          // words kept in front of a block: lane 0's run-up
constexpr uint32_t kBlkGuessBits = 128;  // run-up in front of a segment (a parse is in step after a few codes; 96, 128,
                                         // 160 and 224 bits measured: within 4 % of one another, profiles/r02_notes.md)
constexpr int kBlkGateSleep = 4;         // s_sleep between two polls of the nearest predecessor's entry (drx_lookback.h)
constexpr uint32_t kBlkRounds = 8;       // tickets per resident workgroup a launch should at least have (see run_len)
constexpr uint32_t kBlkTail = 4;         // words behind a block: a code that starts inside may end 24 bits behind it,
                                         // and a window reads three words

template <int NT, int SW>
struct BlkGeom {
    static constexpr int kSegW = SW;
    static constexpr uint32_t kLaneCap = blk_lane_cap(SW);                  // samples a lane can stage
    static constexpr uint32_t kLaneStride = kLaneCap / 2u + 1u;             // dwords per lane: the samples + a dump slot (odd: no bank conflicts)
    static constexpr uint32_t kWords = NT * SW;                             // payload words per block
    static constexpr uint32_t kLdsWords = kBlkPre + kWords + kBlkTail + 4;  // + up to 3 words of 16-byte alignment
    static constexpr uint32_t kOutCap = NT * kLaneCap;                      // samples staged per copy-out
    static constexpr uint32_t kStageWords = NT * kLaneStride;               // the staging buffer, lane-major or output order
    static_assert(kLdsWords % 4 == 0, "the image is filled by 16-byte pieces");
};

__host__ __device__ inline uint32_t blk_words(uint32_t nt, uint32_t k) { return nt * (uint32_t)blk_segw_plan(k); }  // plan-time estimates
__host__ __device__ inline uint32_t blk_words_min(uint32_t nt) { return nt * (uint32_t)kBlkSegWMin; }               // scratch sizing
inline int nt_for_len(uint32_t wave_len, uint32_t k) {
    // lanes per block: a waveform of about (k + 3.5) bits per sample should fill most of its last block
    const uint64_t typ_words = ((uint64_t)wave_len * (2u * k + 7u)) >> 6;
    return typ_words <= blk_words(64, k) ? 64 : (typ_words <= blk_words(128, k) ? 128 : 256);
}

// Workgroup barrier for data exchanged through LDS only.  __syncthreads() also fences global memory, i.e. waits for
// every global load and store the wave has in flight (s_waitcnt vmcnt(0)): the image and the ticket fetched ahead and
// the output lines being written would all be waited for at the next barrier, which is exactly what fetching ahead is
// meant to avoid.  Nothing this kernel exchanges between the waves of a workgroup goes through global memory.
__device__ __forceinline__ void blk_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

enum { kBlkSkip = 0, kBlkCount = 1, kBlkValue = 2 };

// count-leading-zeros that is defined for 0: v_ffbh_u32 returns -1 there, which with the escape's 16 payload bits moves the
// parse on by 15 + 1 bits -- any progress will do (an all-zero window is the padding behind a waveform or a corrupt stream)
__device__ __forceinline__ uint32_t clz_nz(uint32_t x) { return ffbh(x); }
// the 32 bits at Qp of a block's image (see blk_pair)
__device__ __forceinline__ uint32_t blk_window(const uint32_t *W, uint32_t Qp) {
    const uint32_t idx = Qp >> 5;
    return __builtin_amdgcn_alignbit(W[idx + 2u], W[idx + 1u], Qp);
}

// Two codes from the 64-bit window at Qp (three words: a 64-bit window always holds two codes of at most 25 bits).
// W: the block's LDS image; word w of the image sits at W[K + 1 - w] and Qp = 32 K - (bit position), so that
// W[Qp >> 5 .. + 2] are the window's words, last one first, and v_alignbit(hi, lo, Qp) is its first half -- also on a
// word boundary (as in k_decode_lanes).  nu = minus the code length; v_bfe_u32 / v_alignbit_b32 read 5 bits of their
// offset / shift, ~t == 31 - t (mod 32) serves both.
struct BlkPair { uint32_t nu1, nu2, z1, z2; bool pad1, pad2; };
template <bool VALUES>
__device__ __forceinline__ BlkPair blk_pair(const uint32_t *W, uint32_t k, uint32_t Qp) {
    const uint32_t idx = Qp >> 5;
    const uint32_t lo2 = W[idx], lo = W[idx + 1u], hi = W[idx + 2u];
    const uint32_t winA = __builtin_amdgcn_alignbit(hi, lo, Qp);
    const uint32_t winB = __builtin_amdgcn_alignbit(lo, lo2, Qp);
    const uint32_t q1 = clz_nz(winA);
    const uint32_t kk1 = (winA < (1u << 24)) ? 16u : k;  // escape: eight zeros (:223-228)
    BlkPair r;
    r.nu1 = ~(q1 + kk1);
    const uint32_t win2 = __builtin_amdgcn_alignbit(winA, winB, r.nu1);
    const uint32_t q2 = clz_nz(win2);
    const uint32_t kk2 = (win2 < (1u << 24)) ? 16u : k;
    r.nu2 = ~(q2 + kk2);
    r.pad1 = winA < (1u << 23);  // nine zero bits: not a code
    r.pad2 = win2 < (1u << 23);
    r.z1 = r.z2 = 0;
    if (VALUES) {
        r.z1 = (q1 << kk1) + __builtin_amdgcn_ubfe(winA, r.nu1, kk1);
        r.z2 = (q2 << kk2) + __builtin_amdgcn_ubfe(win2, r.nu2, kk2);
    }
    return r;
}
__device__ __forceinline__ uint32_t unzigzag(uint32_t z) { return (z >> 1) ^ (0u - (z & 1u)); }  // :172-177

// The parse.
//   kBlkSkip / kBlkCount: codes are taken while they START before the limit (Qp > qlim);
//     kBlkCount also leaves the running sums (:80-89, from 0 at the lane's first code) in `stage`, two per dword,
//     pair c / 2 at stage[min(c / 2, kBlkLaneCap / 2)] (the last dword is a dump slot), and stops at a window that
//     opens with nine zero bits: no code does (q < 8: '1' within nine bits, escape: eight zeros then '1',
//     :215-228), so that is the zero padding behind the waveform's last code, not a sample;
//   kBlkValue: exactly `cmax` codes (c counts them), each running sum stored as int16 at outp[c].
// A lane that is not enabled keeps its state.  (A variant that ran a wave without per-code masks while every lane had
// room for two more codes, and only the last few codes masked, was measured 4-8 % SLOWER: the vote per pair and the
// second loop cost what the masks had: profiles/r02_notes.md.)
// RESID: the RESIDUALS themselves are staged / stored instead of their running sums (general prediction filters: the inverse
// filter runs afterwards, in place, k_iir_tiles).
// qpad (kBlkCount): a window of nine zero bits is the waveform's padding only where padding can be -- inside its LAST payload
// word (Qp <= qpad; 0 = that word is not in this block).  Anywhere else it is what a parse that is not yet in step sees inside
// an escape's payload (z < 128 has nine leading zeros in its sixteen bits); a lane that stopped there reported a wrong END, its
// successor restarted from that end and stopped there too, and the correction crept through the block one lane per settle
// round: 256 rounds per block at m = 4 (25 % escapes), NOPTREX 26 ms instead of 2, 25 x 14 M samples 106 ms (round 3).
// PAD = false: the caller knows that qpad = 0 (every block but a waveform's last), and the padding test is compiled away.
template <int MODE, bool RESID = false, bool PAD = true>
__device__ __forceinline__ void blk_parse(const uint32_t *W, uint32_t k, bool enable, uint32_t &Qp, uint32_t qlim,
                                          uint32_t &c, uint32_t &sum, uint32_t cmax, uint16_t *outp, uint32_t *stage = nullptr,
                                          uint32_t qpad = 0u, uint32_t cap2 = 0u) {  // cap2: the dump slot = half the lane's share
    auto more = [&](uint32_t q, uint32_t cc) __attribute__((always_inline)) {
        return enable && (MODE == kBlkValue ? cc < cmax : (int32_t)(q - qlim) > 0);
    };
    // staging slot of the next pair (kBlkCount; c is even whenever a pair is staged): a dword index that saturates at the dump slot
    uint32_t slot = (c >> 1) < cap2 ? (c >> 1) : cap2;
    while (__builtin_amdgcn_ballot_w64(more(Qp, c)) != 0ull) {  // (__any() costs a v_cndmask and a v_cmp more)
#pragma unroll
        for (int u = 0; u < 2; ++u) {  // one vote per four codes
            const BlkPair p = blk_pair<MODE != kBlkSkip>(W, k, Qp);
            bool act1 = more(Qp, c);
            const uint32_t Qa = Qp + p.nu1;
            bool act2 = act1 && more(Qa, c + 1u);
            if (MODE == kBlkCount && PAD) {
                if (act1 && p.pad1 && (int32_t)(Qp - qpad) <= 0) { act1 = act2 = false; qlim = Qp; }  // (Qp stays: where the padding starts)
                if (act2 && p.pad2 && (int32_t)(Qa - qpad) <= 0) { act2 = false; qlim = Qa; }
            }
            if (MODE != kBlkSkip) {
                const uint32_t s1 = RESID ? unzigzag(p.z1) : sum + unzigzag(p.z1);
                const uint32_t s2 = RESID ? unzigzag(p.z2) : s1 + unzigzag(p.z2);
                if (MODE == kBlkValue) {
                    if (act1) outp[c] = (uint16_t)s1;
                    if (act2) outp[c + 1u] = (uint16_t)s2;
                }
                if (MODE == kBlkCount) {  // c is even here: only a lane's last pair can end after its first code
                    if (act1) stage[slot] = __builtin_amdgcn_perm(s2, s1, 0x05040100u);
                    slot = slot + 1u < cap2 ? slot + 1u : cap2;
                }
                sum = act2 ? s2 : (act1 ? s1 : sum);
            }
            c += (act1 ? 1u : 0u) + (act2 ? 1u : 0u);
            Qp = act2 ? Qa + p.nu2 : (act1 ? Qa : Qp);
        }
    }
}

// The count parse of a block that does not hold its waveform's last payload word (no padding to recognise): the limit is
// tested once per PAIR of codes and the pair's work runs under the lane's exec mask; a lane whose last pair's second code
// started at or behind the limit takes that code back after the loop.  (The general form above tests every code: a
// quarter more VALU instructions per sample.)  Qp stays far above zero in a block's image (C - bend >= 224 bits), so the
// limit test is an unsigned compare.
template <bool RESID>
__device__ __forceinline__ void blk_count_pairs(const uint32_t *W, uint32_t k, bool enable, uint32_t &Qp, uint32_t qlim,
                                                uint32_t &c, uint32_t &sum, uint32_t *stage, uint32_t cap2) {
    uint32_t slot = 0, Qa_l = Qp, s1_l = sum;  // (c = 0 on entry)
    // A lane that is not enabled gets a limit no position exceeds: the loop's condition is then ONE compare that is the exec
    // mask.  The loop is ROTATED (test at the bottom): with the test at the top the compiler kept the values used behind the
    // loop apart from the loop-carried ones and copied five registers there and back per trip (ten v_mov per four codes, a
    // seventh of the parse's VALU instructions).
    const uint32_t ql = enable ? qlim : 0xffffffffu;
    if (__builtin_amdgcn_ballot_w64(Qp > ql) != 0ull) {
        do {
#pragma unroll
            for (int u = 0; u < 2; ++u) {  // one vote per four codes
                if (Qp > ql) {
                    const BlkPair p = blk_pair<true>(W, k, Qp);
                    const uint32_t s1 = RESID ? unzigzag(p.z1) : sum + unzigzag(p.z1);
                    const uint32_t s2 = RESID ? unzigzag(p.z2) : s1 + unzigzag(p.z2);
                    stage[slot] = __builtin_amdgcn_perm(s2, s1, 0x05040100u);
                    Qa_l = Qp + p.nu1;
                    s1_l = s1;
                    sum = s2;
                    c += 2u;
                    Qp = Qa_l + p.nu2;
                }
                slot = slot + 1u < cap2 ? slot + 1u : cap2;
            }
        } while (__builtin_amdgcn_ballot_w64(Qp > ql) != 0ull);
    }
    if (enable && c != 0u && !(Qa_l > qlim)) { c -= 1u; Qp = Qa_l; sum = s1_l; }
}

// The run-up in the same form: codes are skipped, a pair at a time, while they start in front of the limit.
__device__ __forceinline__ void blk_skip_pairs(const uint32_t *W, uint32_t k, bool enable, uint32_t &Qp, uint32_t qlim) {
    uint32_t Qa_l = Qp;
    const uint32_t ql = enable ? qlim : 0xffffffffu;  // (as in blk_count_pairs: one compare, a rotated loop)
    if (__builtin_amdgcn_ballot_w64(Qp > ql) != 0ull) {
        do {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (Qp > ql) {
                    const BlkPair p = blk_pair<false>(W, k, Qp);
                    Qa_l = Qp + p.nu1;
                    Qp = Qa_l + p.nu2;
                }
            }
        } while (__builtin_amdgcn_ballot_w64(Qp > ql) != 0ull);
    }
    if (enable && !(Qa_l > qlim)) Qp = Qa_l;  // (no pair taken: Qa_l is Qp)
}

// The modes of the kernel body (drx_blocks_body.inc), behind RESID (residuals, not their running sums):
// FUSE (with RESID): the inverse of a general prediction filter (at most four taps, taps[0] = +-1; src/deltaRice.c:91-102) runs
// INSIDE this kernel, over a block's residuals while they sit in LDS in output order: samples, not residuals, are what reaches
// HBM, and no second pass (k_iir_tiles: 2 + 2 more bytes of traffic per sample) follows.  The recurrence is linear over
// Z / 2^16 (drx_iir.hip has the algebra): lane t owns samples [t M, (t + 1) M) of the staging buffer (M = its lane share, so
// equal run lengths and matrices from a table), pass 1 = zero-state response of every run (lane 0 starts from the state in
// front of the block instead), a scan over the lanes with A^(M 2^d), pass 2 = the runs again from their true states.  The state
// behind a block is its last three samples: it stays with thread 0 through a run of blocks, and goes from a run's last block
// to the next run's first through `xstate` (one 8-byte word per block slot, its own flag).  That hand-over is a serial chain
// along a waveform, so the host fuses only where runs of ONE waveform are rarely in flight together (as many waveforms as
// resident workgroups); elsewhere the two-pass form stays.
// STATS (delta filter only): phase 2 reduces the block's samples instead of writing them out (drx_stats_blocks.hip); `out`,
// `itab` and `xstate` are not used.
struct BlkStatsArgs {
    uint32_t head_len;        // DRX_STAT_HEAD_* cover the samples in front of min(head_len, len)
    unsigned long long *acc;  // [waveform][6]: min key, max key, sum, sum of squares, head sum, head sum of squares
};
// PULSES (delta filter only): phase 2 looks for runs of samples over the waveform's threshold instead (drx_pulses_blocks.hip):
// the block's own pulses go to its staging slots, the runs that touch its first and its last sample into its summary.
constexpr uint32_t kPulseTabWords = 8;  // uint64 words of a block's published summary (drx_pulses_blocks.hip has the layout)
struct BlkPulseArgs {
    const int64_t *thr_tab;  // per-waveform thresholds (nullptr: none), thr_stride entries apart, + thr
    uint64_t thr_stride;
    int64_t thr;
    uint32_t neg, min_width;
    uint32_t cap;       // records a block stages: min(max_pulses, kPulseStageCap); 0: the counting form
    uint64_t *table;    // [block slot][kPulseTabWords]
    int64_t *staging;   // [block slot][cap][DRX_PULSE_COLS]
    // the second launch, over the waveforms whose blocks staged too few records (n_redo != nullptr): the launch's waveforms
    // are wave_list[0 .. *n_redo), a count written on the device; word kPulseSegWords of a block's table entry holds the number
    // of the block's first pulse in its waveform (k_pulses_stitch wrote it), and the block stores pulse r straight to slot
    // first + r < max_pulses of the caller's records
    const uint32_t *n_redo;
    uint32_t max_pulses;
    int64_t *out;
};
// WINDOWS (delta filter only): phase 2 is the decoder's -- the block's samples in output order in LDS -- but only where a live
// window of the waveform meets the block, and in place of the copy to the decoded batch every window that meets the staged
// samples receives its share of them in its own row (drx_windows_blocks.hip); `out`, `itab` and `xstate` are not used.
struct BlkWindowArgs {
    WinList wl;  // drx_window_rows.h: the starts, the counts and the rows of drx_decode_windows
};

// BINS (delta filter only): phase 2 reduces the block's samples bin by bin and merges the partial rows into the caller's
// rows, which a fill kernel has set to the identity in front of the blocks (drx_bins_blocks.hip, drx_blocks_bins.inc); `out`,
// `itab` and `xstate` are not used.
struct BlkBinsArgs {
    const int64_t *start;  // per-waveform origins (nullptr: none), start_stride entries apart, + offset (drx_bin_cursor.h)
    uint64_t start_stride;
    int64_t offset;
    uint32_t bin, n_bins;
    int64_t *rows;  // row (g, b) = rows + g * wave_stride + b * DRX_BIN_COLS
    uint64_t wave_stride;
};

// TRANSCODE (any filter: RESID, nothing is filtered): phase 2 sizes or re-codes the block's residuals at another RiceParameter
// (drx_transcode_blocks.hip).  The scheme runs twice.  The SIZES launch is the full scheme; a block leaves in its slot of a table
// its bit count at the new parameter and everything its second run needs to start without its neighbours: where its first code
// starts, its first sample's index, its sample count.  The PACK launch (pack != 0) takes those from the slot -- lane 0's start is
// exact, nothing is looked back for, no end is waited for, nothing is flagged -- and skips the waveforms that `keep` does not
// name; `out`, `itab` and `xstate` are not used.
constexpr uint32_t kTrcSlotWords = 6;  // u32 per block slot: bit offset in the waveform's payload (lo, hi; the sizes launch: bits, 0),
                                       // bits, first code's start in bits behind the block's first, first sample's index, samples
struct BlkTrcArgs {
    static constexpr bool kAllK = false;
    uint32_t k2;    // the new parameter
    uint32_t pack;  // 0: the sizes launch, 1: the pack launch
    uint32_t *slots;             // [block slot][kTrcSlotWords]
    uint32_t *n_blocks;          // [waveform]: written by its last block (the sizes launch)
    unsigned long long *acc16;   // kAllK: [waveform][16] bits at every parameter
    const uint32_t *keep;        // pack: [waveform] != 0: the blocks write it
    const uint32_t *new_rel;     // pack: the result's header positions relative to the chunk, its chunk offsets, its words
    const uint64_t *out_chunk_off;
    uint32_t *outw;
};
struct BlkTrcAllKArgs : BlkTrcArgs { static constexpr bool kAllK = true; };  // the sizes launch with sixteen counts per lane (the estimate)

// a residual's canonical zig-zag value (what the lane kernels' canon() gives: wide foreign codes folded, small escapes ordinary)
__device__ __forceinline__ uint32_t trc_canon16(uint32_t d16) {
    const int32_t d = (int32_t)(int16_t)(uint16_t)d16;
    return (((uint32_t)d << 1) ^ (uint32_t)(d >> 15)) & 0xffffu;
}
// length of z's code at parameter k2
__device__ __forceinline__ uint32_t trc_code_bits(uint32_t z, uint32_t k2) {
    const uint32_t q = z >> k2;
    return q < 8u ? q + 1u + k2 : 25u;
}

// The fallback list (BlkFallbackList), in the kernel behind the blocks: waveform g goes to the lane kernel if every waveform does
// (all_listed: the form's *_ALL_FALLBACK flag), if the blocks flagged it, or -- where the caller asks -- if no block has judged
// it: unjudged(), the caller's test for "samples and no payload word", evaluated last.
__device__ __forceinline__ bool blk_listed(uint32_t all_listed, const uint32_t *fail, const uint32_t *suspect, uint64_t g) {
    return all_listed || fail[g] || suspect[g];
}
template <class F>
__device__ __forceinline__ bool blk_listed(uint32_t all_listed, const uint32_t *fail, const uint32_t *suspect, uint64_t g, F unjudged) {
    return blk_listed(all_listed, fail, suspect, g) || unjudged();
}
__device__ __forceinline__ void blk_list_append(uint32_t *n_listed, uint32_t *listed, uint32_t g) { listed[atomicAdd(n_listed, 1u)] = g; }

}  // namespace drx
#endif
