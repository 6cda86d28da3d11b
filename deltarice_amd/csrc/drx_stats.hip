// drx_stats.hip -- per-waveform statistics straight from the encoded stream (drx_wave_stats): every waveform is parsed as
// drx_decode parses it, and reduced to eight int64 values (DRX_STAT_* of include/deltarice_hip.h) instead of being written out.
// The batch is read once (the stream) and 64 bytes per waveform are written; no sample goes to memory.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_wave_stats(): the walks of drx_walk.hip, or the side-band's tables).
//
//   k_wave_stats         delta filter: one LANE per waveform, 64 waveforms per wavefront, the stream side the shared reader's
//                        (drx_lane_reader.inc): a lane starts at its first sample and stops behind its last, and
//                        the reader's ring (16 896 bytes) is all the LDS there is.
//   k_wave_stats_serial  every other prediction filter: one lane per waveform, the serial parse of the same header inside the
//                        serial kernels' frame (serial_frame(), drx_lane_stream.h).  Correct, not tuned.
//
// Few long waveforms (the nEDM / NOPTREX shapes, the reference's default one waveform per chunk) under the delta filter do NOT
// run here: a lane per waveform is 50-60 ns per sample and lane whatever else runs, with most of the chip idle (2048 waveforms of
// 500 000 samples: 26 ms).  The batches that drx_decode gives to the block decoder take the block form of drx_stats_blocks.hip --
// a workgroup per block of a waveform's stream -- and this file's launcher runs k_wave_stats_serial behind it over the waveforms
// that form lists (flagged or suspect ones: computed again and judged here, a lane each).  General filters, and batches under
// DRX_DBG_STATS_LANES, stay a lane per waveform whatever their shape (DESIGN.md section 4.2f has the measured rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"

namespace drx {

// (a lane's row, eight int64: store_i64_row() of drx_device.h; s16x2, as_pair(), as_word(), kNarrow: drx_lane_stream.h)
// Lanes map by LANE_WAVE_G_ACTIVE_LEN (drx_lane_stream.h).  wf_base: first wavefront of this launch (a batch whose wavefronts one launch cannot carry goes
// out in slices: for_wavefront_slices()).
//
// A group is 16 samples, as in the decoder.  A lane whose group lies inside its waveform, is not its first and does not hold
// the end of the head window runs the UNMASKED group: eight pairs, reduced in registers as packed pairs of int16 (v_pk_min /
// v_pk_max, v_dot2 against {1, 1} for the sum and against itself for the sum of squares).  The first group of a waveform, the
// group in which it ends and the group in which its head window ends (h in [i, i + 16): the sums are copied in front of
// sample h) run the masked form, a sample per ring access; lanes behind their last sample run neither (both forms sit under
// the exec mask, and a wavefront none of whose lanes takes a form branches round it).  A uniform batch runs the masked form
// two or three times per waveform.
//
// First occurrences.  The unmasked group folds its pairs into PACKED running extremes (the samples of even and of odd index
// apart) and looks no further while neither register moves: one compare per group.  Where one moves the group may hold a new
// extreme of the waveform; only then are the group's own minimum and maximum formed and compared with the lane's, STRICTLY, so
// that an earlier group keeps a tie, and only where one wins are the sixteen values looked through, from the last to the first,
// for its position.  On noise that happens O(log len) times per waveform; on a ramp in every group.  The first group goes
// through the masked form so that the scalar extremes start from a sample (a constant 32767 never moves the packed ones).
//
// Sums.  A group's sum of samples is below 2^20 in magnitude: a 32-bit v_dot2 chain, added to the 64-bit sum once per group.
// A PAIR's sum of squares reaches 2^31 (two samples of -32768) and a group's 2^34; while every sample so far lies within
// +-kNarrow (a flag kept where the extremes are) a group's fits 32 bits and is one chain and one 64-bit add, otherwise the
// pairs' are added one by one.
__global__ __launch_bounds__(64) void k_wave_stats(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                   const uint64_t *__restrict__ wave_off,
                                                   const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                   uint32_t head_len, DevStatus *st, int64_t *__restrict__ out) {
    constexpr int GS = kGS;
    __shared__ uint32_t ring_all[kInRingWords];
    const int lane = lane_id();
    const uint32_t k = G.k;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
    LANE_WAVE_G_ACTIVE_LEN(G, wf_base + blockIdx.x, lane)
    uint32_t n = 0;
    uint64_t S = 1;
    if (active) {
        S = wave_off[g] + 1u;
        n = wave_words[g];
    }
    uint32_t *const ring = ring_all + 64;
#include "drx_lane_reader.inc"

    const uint32_t steps = wave_max_u32(len);
    const uint32_t h = head_len < len ? head_len : len;  // the head window ends in front of sample h
    int32_t acc = 0;                                     // running sum of the deltas: the sample in its low 16 bits
    int32_t mn = 0x7fffffff, mx = -0x7fffffff - 1;       // (any sample beats them)
    uint32_t amn = 0, amx = 0;
    int64_t sum = 0, hsum = 0;
    uint64_t sq = 0, hsq = 0;
    // what the unmasked group keeps instead of mn / mx: packed extremes of the samples so far, those of even and of odd index
    // apart (every sample is in one of the halves, so a new extreme of the waveform moves one of them), and whether all
    // samples so far lie within +-kNarrow
    s16x2 rmn = {32767, 32767}, rmx = {-32768, -32768};
    bool narrow = true;
    set_limits();
    for (uint32_t i = 0; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (i != 0u && i + (uint32_t)GS <= len && h - i >= (uint32_t)GS) {  // (h < i wraps: the window ended earlier)
            // ---- the unmasked group: eight pairs, two samples per ring access
            LANE_GROUP_PAIRS(acc, pr, 0u)  // the group's samples, two to a register (the earlier one in the low half)
            s16x2 nmn = rmn, nmx = rmx;
            int32_t gsum = 0, gsq = 0;
#pragma unroll
            for (int j = 0; j < GS / 2; ++j) {
                const s16x2 p = as_pair(pr[j]);
                nmn = __builtin_elementwise_min(nmn, p);
                nmx = __builtin_elementwise_max(nmx, p);
                gsum = __builtin_amdgcn_sdot2(p, (s16x2){1, 1}, gsum, false);
                gsq = __builtin_amdgcn_sdot2(p, p, gsq, false);
            }
            if (((as_word(nmn) ^ as_word(rmn)) | (as_word(nmx) ^ as_word(rmx))) != 0u) {
                // a running extreme of one of the halves moved: the group may hold a new minimum or maximum of the waveform
                rmn = nmn;
                rmx = nmx;
                s16x2 pmn = as_pair(pr[0]), pmx = pmn;
#pragma unroll
                for (int j = 1; j < GS / 2; ++j) {
                    pmn = __builtin_elementwise_min(pmn, as_pair(pr[j]));
                    pmx = __builtin_elementwise_max(pmx, as_pair(pr[j]));
                }
                const int32_t gmn = pmn.x < pmn.y ? (int32_t)pmn.x : (int32_t)pmn.y;
                const int32_t gmx = pmx.x > pmx.y ? (int32_t)pmx.x : (int32_t)pmx.y;
                if (gmn < mn) {  // STRICTLY: an earlier group keeps a tie.  Its first position, looking from the last sample to the first
                    const uint32_t want = (uint32_t)gmn & 0xffffu;
                    uint32_t pos = 0;
#pragma unroll
                    for (int j = GS / 2 - 1; j >= 0; --j) {
                        pos = (pr[j] >> 16) == want ? 2u * (uint32_t)j + 1u : pos;
                        pos = (pr[j] & 0xffffu) == want ? 2u * (uint32_t)j : pos;
                    }
                    mn = gmn;
                    amn = i + pos;
                }
                if (gmx > mx) {
                    const uint32_t want = (uint32_t)gmx & 0xffffu;
                    uint32_t pos = 0;
#pragma unroll
                    for (int j = GS / 2 - 1; j >= 0; --j) {
                        pos = (pr[j] >> 16) == want ? 2u * (uint32_t)j + 1u : pos;
                        pos = (pr[j] & 0xffffu) == want ? 2u * (uint32_t)j : pos;
                    }
                    mx = gmx;
                    amx = i + pos;
                }
                narrow = mn >= -kNarrow && mx <= kNarrow;
            }
            sum += (int64_t)gsum;
            if (narrow) {
                sq += (uint64_t)(uint32_t)gsq;  // sixteen squares of at most kNarrow^2: below 2^32
            } else {
#pragma unroll
                for (int j = 0; j < GS / 2; ++j) sq += (uint64_t)(uint32_t)__builtin_amdgcn_sdot2(as_pair(pr[j]), as_pair(pr[j]), 0, false);
            }
        } else if (i < len) {
            // ---- the masked group: the lane's waveform or its head window ends inside it.  One sample per ring access.
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)GS; ++u) {
                const uint32_t idx = i + u;
                if (idx < len) {
                    if (idx == h) { hsum = sum; hsq = sq; }
                    LANE_ONE(z)
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    const int32_t y = (int32_t)(int16_t)(uint16_t)acc;
                    sum += y;
                    sq += (uint64_t)(uint32_t)(y * y);
                    if (y < mn) { mn = y; amn = idx; }
                    if (y > mx) { mx = y; amx = idx; }
                    const s16x2 yy = {(short)y, (short)y};
                    rmn = __builtin_elementwise_min(rmn, yy);
                    rmx = __builtin_elementwise_max(rmx, yy);
                    narrow = mn >= -kNarrow && mx <= kNarrow;
                }
            }
        }
        round_end(i);
    }
    if (!active) return;
    if (h == len) { hsum = sum; hsq = sq; }  // the window holds the whole waveform
    if (len && LANE_MISSES_LAST_WORD()) atomicOr(&st->err, kErrCorrupt);
    const int64_t v[DRX_STAT_COLS] = {(int64_t)mn, (int64_t)amn, (int64_t)mx, (int64_t)amx, sum, (int64_t)sq, hsum, (int64_t)hsq};
    const bool vec = ((uintptr_t)out & 15u) == 0;  // (in front of the row's address: the kernel keeps its instructions)
    store_i64_row(out + g * (uint64_t)DRX_STAT_COLS, vec, v);
}

// General prediction filters: serial_frame() (drx_lane_stream.h) with the same eight reductions, a sample at a time.
// list != nullptr: the waveforms list[0 .. *n_list) instead of all of them (behind the block form, drx_stats_blocks.hip: the
// list and its length are written on the device by the kernel in front; the launch is sized for the whole batch).
__global__ __launch_bounds__(64) void k_wave_stats_serial(Geom G, const uint32_t *__restrict__ in,
                                                          const uint64_t *__restrict__ wave_off,
                                                          const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                          uint32_t head_len, DevStatus *st, int64_t *__restrict__ out,
                                                          const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    uint32_t h = 0;  // the head window ends in front of sample h
    int32_t mn = 0x7fffffff, mx = -0x7fffffff - 1;
    uint32_t amn = 0, amx = 0;
    int64_t sum = 0, hsum = 0;
    uint64_t sq = 0, hsq = 0;
    serial_frame(
        G, in, wave_off, wave_words, wf_base, list, list ? (uint64_t)*n_list : 0u, st,
        [&](uint64_t, const WaveRef &r) __attribute__((always_inline)) {
            h = head_len < r.len ? head_len : r.len;
            return r.len;
        },
        [&](uint32_t i, int16_t y16) __attribute__((always_inline)) {
            if (i == h) { hsum = sum; hsq = sq; }
            const int32_t y = y16;
            sum += y;
            sq += (uint64_t)(uint32_t)(y * y);
            if (y < mn) { mn = y; amn = i; }
            if (y > mx) { mx = y; amx = i; }
        },
        [&](uint64_t g, const WaveRef &r) __attribute__((always_inline)) {
            if (h == r.len) { hsum = sum; hsq = sq; }
            const int64_t v[DRX_STAT_COLS] = {(int64_t)mn, (int64_t)amn, (int64_t)mx, (int64_t)amx, sum, (int64_t)sq, hsum, (int64_t)hsq};
            store_i64_row(out + g * (uint64_t)DRX_STAT_COLS, ((uintptr_t)out & 15u) == 0, v);
        });
}

hipError_t launch_wave_stats(const StreamCall &c, void *d_blk, void *d_sacc, uint32_t head_len, int64_t *d_out, uint32_t *form_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    const bool blocks = d_sacc != nullptr && blocks_form_batch(G, d_blk, kStatsForm);
    if (form_out) *form_out = blocks_form_word(G, blocks, kStatsForm);
    if (G.total_waves == 0) return hipSuccess;
    // ---- the walk (drx_walk.hip), all of it on this stream: nothing here is worth a fork
    hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    if (blocks) {
        // ---- few long waveforms: a workgroup per block of a waveform's stream, then a lane per waveform that form lists (the
        // launch is sized from here, at most a lane per waveform of the batch; the list's length is read on the device)
        BlkFallbackList fl;
        if ((e = launch_stats_blocks(c, d_blk, d_sacc, head_len, d_out, &fl)) != hipSuccess) return e;
        k_wave_stats_serial<<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, 0, head_len, c.d_status, d_out, fl.listed, fl.n_listed);
    } else {
        // ---- the kernel: a wavefront per 64 waveforms
        const bool serial = G.n_taps != 0;
        for_wavefront_slices(G, !serial, [&](uint64_t base, unsigned nb) {
            if (serial)
                k_wave_stats_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, head_len, c.d_status, d_out, nullptr, nullptr);
            else
                k_wave_stats<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, head_len, c.d_status, d_out);
        });
    }
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
