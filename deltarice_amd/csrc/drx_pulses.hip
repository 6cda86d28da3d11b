// drx_pulses.hip -- every pulse of every waveform straight from the encoded stream (drx_find_pulses): threshold discrimination.
// Waveform g is parsed as drx_decode parses it; its samples are compared with a per-waveform threshold t_g, every maximal run of
// consecutive samples over it that is at least min_width long is a pulse, and the first max_pulses of them go out as records of
// DRX_PULSE_COLS int64 (start, width, peak, where the peak sits, integral) beside the count of all of them.  The batch is read
// once and no sample goes to memory.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_find_pulses(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   k_find_pulses         delta filter: one LANE per waveform, 64 waveforms per wavefront, the stream side the shared reader's
//                         (drx_lane_reader.inc) with its end-of-payload check.  This file's own is what happens to a
//                         group's 16 samples: a small state machine per lane instead of eight running reductions, behind a
//                         fast reject.  The reader's ring (16 896 bytes) is all the LDS there is.
//   k_find_pulses_serial  every other prediction filter: one lane per waveform, the serial parse of the same header
//                         (serial_wave()) with the filter's history in an LDS column and the same state machine.  Correct,
//                         not tuned.
//
// Few long waveforms (the nEDM / NOPTREX shapes, the reference's default of one waveform per chunk) under the delta filter do
// NOT run here: a lane per waveform is 50-60 ns per sample and lane whatever else runs, with most of the chip idle.  The batches
// that drx_wave_stats gives to its block form take the block form of drx_pulses_blocks.hip -- a workgroup per block of a
// waveform's stream, the runs stitched across the blocks' borders behind it -- and this file's launcher runs
// k_find_pulses_list, the delta filter's lane kernel over a list, behind that over the waveforms it lists (flagged or suspect
// ones, and those whose blocks staged too few records: computed again and judged here, a lane each).  General filters, and batches under DRX_DBG_PULSES_LANES, stay a
// lane per waveform whatever their shape (DESIGN.md section 4.2i has the measured rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_pulse_runs.h"

namespace drx {

// One polarity.  A sample y enters the state machine as v = y ^ flip, flip = 0 for positive polarity and -1 for negative:
// ~y = -1 - y reverses the order of the int16 values without leaving them, so "y < t" is "v > -1 - t" and the minimum of a run
// is the complement of the maximum of its v.  The lane's threshold tv is clamped so that it compares as an int32 with any
// int16: positive polarity t to [-32769, 32767] (at the top nothing is over, at the bottom everything), negative polarity t to
// [-32768, 32768] and then tv = -1 - t, the same range.  The sum d_thr + thr saturates at the int64 ends.
__device__ __forceinline__ int32_t lane_threshold(const int64_t *__restrict__ thr_tab, uint64_t thr_stride, int64_t thr, bool neg,
                                                  uint64_t g) {
    return pulse_threshold(thr_tab != nullptr, thr_tab ? thr_tab[g * thr_stride] : 0, thr, neg);  // (drx_pulse_runs.h: sum and clamp)
}

// A lane's state: whether a run is open, where it began, its largest v and the first place of that, the sum of its v, and
// how many pulses the waveform has had.  step() takes sample idx; close() ends the open run in front of sample e.
struct PulseLane {
    int32_t tv;        // v > tv: over
    uint32_t min_width, max_pulses;
    int64_t flip;      // 0 / -1
    int64_t *slots;    // the waveform's max_pulses records
    bool open;
    uint32_t s, apk;
    int32_t peak;
    int64_t sum;
    uint32_t count;

    __device__ __forceinline__ void close(uint32_t e) {
        const uint32_t w = e - s;
        if (w >= min_width) {
            if (count < max_pulses) {  // rare: plain 8-byte stores
                int64_t *rec = slots + (uint64_t)count * (uint64_t)DRX_PULSE_COLS;
                rec[DRX_PULSE_START] = (int64_t)s;
                rec[DRX_PULSE_WIDTH] = (int64_t)w;
                rec[DRX_PULSE_PEAK] = (int64_t)peak ^ flip;
                rec[DRX_PULSE_ARGPEAK] = (int64_t)apk;
                rec[DRX_PULSE_SUM] = flip ? -sum - (int64_t)w : sum;  // y = -1 - v
            }
            ++count;
        }
        open = false;
    }
    __device__ __forceinline__ void step(int32_t v, uint32_t idx) {
        if (v > tv) {
            if (!open) {
                open = true;
                s = idx;
                apk = idx;
                peak = v;
                sum = 0;
            } else if (v > peak) {  // STRICTLY: the first occurrence keeps a tie
                peak = v;
                apk = idx;
            }
            sum += v;
        } else if (open) {
            close(idx);
        }
    }
};

// Lanes map by LANE_WAVE_G_ACTIVE_LEN (drx_lane_stream.h).  wf_base: first wavefront of this launch (for_wavefront_slices()).
//
// A group is 16 samples.  A lane whose group lies inside its waveform, i + 16 <= len, runs the UNMASKED group: eight pairs of
// samples in eight registers, two to a register.  The fast reject: while the lane has no run open, a packed maximum over the
// eight pairs (of v = y ^ flip: one v_xor and one v_pk_max_i16 per pair) and one compare of its larger half with the lane's
// threshold say that the group holds nothing over it, and the group is done -- on ordinary data almost every group.  Only a
// group that holds an over sample, or is entered with a run open, goes sample by sample through the state machine: a rolled
// loop over the eight registers, which rotate so that every index is a constant (no scratch).  The group in which the
// waveform ends runs the masked form, a sample per ring access and a step of the state machine each.  A run still open behind
// the last sample is closed there, e = len.
//
// The zero slots come from one hipMemsetAsync of the output in front of the launch (launch_find_pulses()); a lane stores the
// records of its first max_pulses pulses as they close and its count at its end.
__global__ __launch_bounds__(64) void k_find_pulses(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                    const uint64_t *__restrict__ wave_off,
                                                    const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                    const int64_t *__restrict__ thr_tab, uint64_t thr_stride, int64_t thr,
                                                    uint32_t neg, uint32_t min_width, uint32_t max_pulses, DevStatus *st,
                                                    uint32_t *__restrict__ count_out, int64_t *__restrict__ out) {
    constexpr bool LIST = false;
    const uint32_t *const list = nullptr, *const n_list = nullptr;
#include "drx_pulses_lane_body.inc"
}

// The same kernel over the waveforms list[0 .. *n_list) instead of all of them (behind the block form, drx_pulses_blocks.hip: the
// list and its length are written on the device by the kernel in front; the launch is sized for the whole batch).  Every lane
// reads its own stream through its own ring column, so the lanes of a wavefront may hold any waveforms.  Lane 0 of the launch
// leaves the list's length in the status word for drx_plan_last_pulses_listed.
__global__ __launch_bounds__(64) void k_find_pulses_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                         const uint64_t *__restrict__ wave_off,
                                                         const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                         const int64_t *__restrict__ thr_tab, uint64_t thr_stride, int64_t thr,
                                                         uint32_t neg, uint32_t min_width, uint32_t max_pulses, DevStatus *st,
                                                         uint32_t *__restrict__ count_out, int64_t *__restrict__ out,
                                                         const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    constexpr bool LIST = true;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->listed = *n_list;
#include "drx_pulses_lane_body.inc"
}

// General prediction filters: a lane per waveform, serial_wave() (global loads); the last 64 outputs of every
// lane in an LDS column (taps <= DRX_MAX_TAPS = 64).
// Not on serial_frame() (drx_lane_stream.h): through it this kernel was measured 2.8 % slower, profiles/serial_frame_refactor_ab.txt.
__global__ __launch_bounds__(64) void k_find_pulses_serial(Geom G, const uint32_t *__restrict__ in,
                                                           const uint64_t *__restrict__ wave_off,
                                                           const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                           const int64_t *__restrict__ thr_tab, uint64_t thr_stride, int64_t thr,
                                                           uint32_t neg, uint32_t min_width, uint32_t max_pulses, DevStatus *st,
                                                           uint32_t *__restrict__ count_out, int64_t *__restrict__ out) {
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    const uint32_t lane = threadIdx.x;
    const uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;  // (as k_find_pulses)
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    const uint32_t *s = in + wave_off[g] + 1;
    const uint32_t n = wave_words[g];
    PulseLane P;
    P.tv = lane_threshold(thr_tab, thr_stride, thr, neg != 0u, g);
    P.min_width = min_width;
    P.max_pulses = max_pulses;
    P.flip = neg ? -1 : 0;
    P.slots = out + g * (uint64_t)max_pulses * (uint64_t)DRX_PULSE_COLS;
    P.open = false;
    P.s = P.apk = 0;
    P.peak = 0;
    P.sum = 0;
    P.count = 0;
    const int32_t fm = neg ? -1 : 0;
    // the sample drx_decode writes, flipped for negative polarity
    const uint64_t words = serial_wave(G, s, n, r.len, &hist[0][lane], 64u,
                                       [&](uint32_t i, int16_t y) __attribute__((always_inline)) { P.step((int32_t)y ^ fm, i); });
    if (P.open) P.close(r.len);
    if (r.len && words != n) atomicOr(&st->err, kErrCorrupt);
    count_out[g] = P.count;
}

hipError_t launch_find_pulses(const StreamCall &c, void *d_blk, void *d_ptab, void *d_pstage, const int64_t *d_thr, uint64_t thr_stride,
                              int64_t thr, bool neg, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count, int64_t *d_out,
                              uint32_t *form_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    const bool blocks = d_ptab != nullptr && (d_pstage != nullptr || max_pulses == 0u) && blocks_form_batch(G, d_blk, kPulsesForm);
    if (form_out) *form_out = blocks_form_word(G, blocks, kPulsesForm);
    if (G.total_waves == 0) return hipSuccess;
    // ---- the walk (drx_walk.hip): launch_batch_walk()
    hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    // ---- the zero slots: the whole output, once (the lanes then store the records alone)
    if (max_pulses && (e = hipMemsetAsync(d_out, 0, (size_t)(G.total_waves * (uint64_t)max_pulses * DRX_PULSE_COLS * sizeof(int64_t)), s)) != hipSuccess)
        return e;
    if (blocks) {
        // ---- few long waveforms: a workgroup per block of a waveform's stream and the stitch behind it, then a lane per waveform
        // that form lists (the launch is sized from here, at most a lane per waveform of the batch; the list's length is read on
        // the device)
        BlkFallbackList fl;
        if ((e = launch_pulses_blocks(c, d_blk, d_ptab, d_pstage, d_thr, thr_stride, thr, neg, min_width, max_pulses, d_count, d_out, &fl)) != hipSuccess)
            return e;
        k_find_pulses_list<<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, 0, d_thr, thr_stride, thr,
                                                                       neg ? 1u : 0u, min_width, max_pulses, c.d_status, d_count, d_out, fl.listed,
                                                                       fl.n_listed);
    } else {
        // ---- the kernel: a wavefront per 64 waveforms
        const bool serial = G.n_taps != 0;
        for_wavefront_slices(G, !serial, [&](uint64_t base, unsigned nb) {
            if (serial)
                k_find_pulses_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, d_thr, thr_stride, thr, neg ? 1u : 0u, min_width,
                                                       max_pulses, c.d_status, d_count, d_out);
            else
                k_find_pulses<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, d_thr, thr_stride, thr, neg ? 1u : 0u,
                                                min_width, max_pulses, c.d_status, d_count, d_out);
        });
    }
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
