// drx_window.hip -- a window of every waveform, at per-waveform offsets, straight from the encoded stream (drx_decode_window):
// waveform g is parsed as drx_decode parses it, from its first code to the last code of its window and no further, and the
// `width` samples from a_g = start[g] + offset on go to row g of the output (`pad` where the window leaves the waveform).
// The batch is not decoded to memory: a lane reads the head of its payload and writes its own row.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_decode_window(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   k_decode_window         delta filter: one LANE per waveform, 64 waveforms per wavefront.  The stream side is the shared
//                           reader's early-ending form (drx_lane_reader.inc with DRX_LANE_EARLY): a lane ENDS EARLY, behind sample
//                           e_g = min(a_g + width, len_g), and requests no piece once it is through -- a wavefront runs
//                           wave_max(e_g) samples, so a head window fetches the head of every payload.  The reader's ring
//                           (16 896 bytes) is all the LDS there is: the stores need no staging.
//   k_decode_window_serial  every other prediction filter: one lane per waveform, the serial parse of the same header
//                           (serial_wave()) with the filter's history in an LDS column, stopping at the window's end.
//                           Correct, not tuned.
//
// Few long waveforms (the nEDM / NOPTREX shapes: a few thousand waveforms of 10^5 - 10^6 samples) go through the same
// lane-per-waveform kernels.  That is correct and slow, 50-60 ns per sample and lane whatever else runs, with most of the
// chip idle.  drx_decode_windows with n_win = 1 (drx_windows_blocks.hip) is the form for such batches: a workgroup per block of
// a waveform's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_window_rows.h"

namespace drx {

// Win, window_at() and fill_pad(): drx_window_rows.h (shared with drx_decode_windows' kernels)
__device__ __forceinline__ Win window_of(const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset, uint32_t width,
                                         uint64_t g, uint32_t len) {
    // (window_at(window_start()) of that header, written out: through the two functions the kernels' prologues were scheduled
    // another way, and this call keeps its instructions)
    int64_t a = offset;
    if (start) {
        const int64_t v = start[g * start_stride];
        if (__builtin_add_overflow(v, offset, &a)) a = v < 0 ? INT64_MIN : INT64_MAX;  // the sum saturates
    }
    Win w = {0u, 0u, width};
    if (a >= (int64_t)len) return w;
    const int64_t t = a + (int64_t)width;  // (a < 2^31: no overflow)
    if (t <= 0) return w;
    w.e = t < (int64_t)len ? (uint32_t)t : len;
    w.s = a < 0 ? 0u : (uint32_t)a;
    w.pf = a < 0 ? (uint32_t)(0 - a) : 0u;  // (0 < -a < width here)
    return w;
}

// Lanes map by LANE_WAVE_G_ACTIVE_LEN (drx_lane_stream.h).  wf_base: first wavefront of this launch (for_wavefront_slices()).
//
// A group is 16 samples.  A lane whose group lies inside its parse range, i + 16 <= e, runs the UNMASKED group: eight pairs of
// samples in eight registers, two to a register.  The group in which the range ends runs the masked form, a sample per ring
// access; lanes that are through run neither (both forms sit under the exec mask).
//
// Stores.  The lane writes its own row; rs + idx is where sample idx goes, so the parity p of rs (in int16 elements) is the
// parity of every group's first destination.  A group that lies inside the window goes out as eight DWORD stores at even
// elements: the pairs as they are where p = 0; where p = 1 shifted by one sample, with the group's last sample CARRIED to the
// next group's first dword (v_alignbit of neighbouring pairs) -- consecutive dwords, which the compiler is free to widen.
// 2-byte stores write the ends of a row only: the group in which the window begins (or whose first dword would need a sample
// in front of the window), the carried sample of a lane's last unmasked group, and the masked group.  The pads go out first,
// by fill_pad().
//
// Verdict.  A lane whose range reaches its waveform's last sample makes the reader's end-of-payload check.  Any other lane
// asks only that its codes lay inside its payload, bits <= 32 n: nothing behind the window's last code is looked at, though a
// piece that was requested ahead may have fetched it.  The stream position Q counts mod 2^32; flw (words fetched) does not
// wrap, and while a lane has words to come its position stays within a ring of flw, so `over` (the position passed flw: seen
// at the group where it happens, a group eats at most 13 words) and the distance to flw at the end give the exact position.
__global__ __launch_bounds__(64) void k_decode_window(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                      const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset,
                                                      uint32_t width, uint32_t pad2, DevStatus *st, int16_t *out,
                                                      uint64_t out_stride) {
    constexpr int GS = kGS;
    __shared__ uint32_t ring_all[kInRingWords];
    const int lane = lane_id();
    const uint32_t k = G.k;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
    LANE_WAVE_G_ACTIVE_LEN(G, wf_base + blockIdx.x, lane)
    uint32_t n = 0;
    uint64_t S = 1;
    Win w = {0u, 0u, 0u};
    int16_t *row = out;
    if (active) {
        w = window_of(start, start_stride, offset, width, g, len);
        row = out + g * out_stride;
        fill_pad(row, 0u, w.pf, pad2);
        fill_pad(row, w.pf + (w.e - w.s), width, pad2);
    }
    const uint32_t s = w.s, e = w.e;  // the lane parses samples [0, e) and stores [s, e)
    if (e) {
        S = wave_off[g] + 1u;
        n = wave_words[g];
    }
    int16_t *const rs = row + ((int64_t)w.pf - (int64_t)s);  // sample idx goes to rs[idx]
    const uint32_t p = (uint32_t)((uintptr_t)rs >> 1) & 1u;
    uint32_t *const ring = ring_all + 64;
#define DRX_LANE_EARLY
#include "drx_lane_reader.inc"
#undef DRX_LANE_EARLY

    const uint32_t steps = wave_max_u32(e);
    int32_t acc = 0;     // running sum of the deltas: the sample in its low 16 bits
    uint32_t carry = 0;  // the last pair of the group before
    bool over = false;   // the position passed the words the lane fetched
    set_limits();
    for (; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (i + (uint32_t)GS <= e) {
            // ---- the unmasked group: eight pairs, two samples per ring access
            LANE_GROUP_PAIRS(acc, pr, 0u)  // the group's samples, two to a register (the earlier one in the low half)
            if (i + (uint32_t)GS > s) {  // some of the group lies in the window
                const bool last = i + 2u * (uint32_t)GS > e;  // the lane's last unmasked group: nobody takes its carry
                if (i >= s + p) {
                    // inside the window, the sample in front of it included where the first dword holds it
                    uint32_t *q = (uint32_t *)(rs + i - p);
                    uint32_t prev = carry;
#pragma unroll
                    for (int j = 0; j < GS / 2; ++j) {
                        q[j] = p ? __builtin_amdgcn_alignbit(pr[j], prev, 16u) : pr[j];
                        prev = pr[j];
                    }
                    if (p && last) rs[i + (uint32_t)GS - 1u] = (int16_t)(pr[GS / 2 - 1] >> 16);
                } else {
                    // the window begins here: 2-byte stores (the last sample rides with the next group's first dword)
                    const bool keep = !p || last;
#pragma unroll
                    for (int u = 0; u < GS; ++u) {
                        const uint32_t v = (u & 1) ? pr[u / 2] >> 16 : pr[u / 2];
                        if (i + (uint32_t)u >= s && (u < GS - 1 || keep)) rs[i + (uint32_t)u] = (int16_t)v;
                    }
                }
            }
            carry = pr[GS / 2 - 1];
        } else if (i < e) {
            // ---- the masked group: the lane's parse range ends inside it.  One sample per ring access, 2-byte stores.
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)GS; ++u) {
                const uint32_t idx = i + u;
                if (idx < e) {
                    LANE_ONE(z)
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    if (idx >= s) rs[idx] = (int16_t)(uint16_t)acc;
                }
            }
        }
        over |= ((flw - ((~Q) >> 5)) & kWMask) > (uint32_t)kRW;
        round_end(i);
    }
    if (!e) return;
    const uint32_t used_words = LANE_USED_WORDS();
    bool bad;
    if (e == len) {
        bad = LANE_MISSES_LAST_WORD_AT(used_words);
    } else {
        // the window's codes lay inside the payload: the exact end position from its distance to flw (at most a ring)
        const uint32_t d = (flw - (s0 + used_words)) & kWMask;
        const int32_t sd = (int32_t)(d << 5) >> 5;
        bad = over || (uint64_t)flw - (uint64_t)(int64_t)sd > (uint64_t)s0 + n;
    }
    if (bad) atomicOr(&st->err, kErrCorrupt);
}

// General prediction filters: a lane per waveform, serial_wave() (global loads); the last 64 outputs of every
// lane in an LDS column (taps <= DRX_MAX_TAPS = 64).  2-byte stores.
// Not on serial_frame() (drx_lane_stream.h): through it this kernel was measured 0.9 % slower, profiles/serial_frame_refactor_ab.txt.
__global__ __launch_bounds__(64) void k_decode_window_serial(Geom G, const uint32_t *__restrict__ in,
                                                             const uint64_t *__restrict__ wave_off,
                                                             const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                             const int64_t *__restrict__ start, uint64_t start_stride,
                                                             int64_t offset, uint32_t width, uint32_t pad2, DevStatus *st,
                                                             int16_t *out, uint64_t out_stride) {
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    const uint32_t lane = threadIdx.x;
    const uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;  // (as k_decode_window)
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    const Win w = window_of(start, start_stride, offset, width, g, r.len);
    int16_t *row = out + g * out_stride;
    fill_pad(row, 0u, w.pf, pad2);
    fill_pad(row, w.pf + (w.e - w.s), width, pad2);
    if (!w.e) return;
    int16_t *const rs = row + ((int64_t)w.pf - (int64_t)w.s);
    const uint32_t *s = in + wave_off[g] + 1;
    const uint32_t n = wave_words[g];
    // the sample drx_decode writes; the payload words the codes took
    const uint64_t words = serial_wave(G, s, n, w.e, &hist[0][lane], 64u,
                                       [&](uint32_t i, int16_t y) __attribute__((always_inline)) { if (i >= w.s) rs[i] = y; });
    if (w.e == r.len ? words != n : words > n) atomicOr(&st->err, kErrCorrupt);
}

hipError_t launch_decode_window(const StreamCall &c, const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width,
                                int16_t pad, int16_t *d_out, uint64_t out_stride) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    if (G.total_waves == 0) return hipSuccess;
    // ---- the walk (drx_walk.hip): launch_batch_walk()
    const hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    // ---- the kernel: a wavefront per 64 waveforms
    const bool serial = G.n_taps != 0;
    const uint32_t pad2 = (uint32_t)(uint16_t)pad * 0x10001u;
    for_wavefront_slices(G, !serial, [&](uint64_t base, unsigned nb) {
        if (serial)
            k_decode_window_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, d_start, start_stride, offset, width, pad2,
                                                     c.d_status, d_out, out_stride);
        else
            k_decode_window<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, d_start, start_stride, offset, width,
                                              pad2, c.d_status, d_out, out_stride);
    });
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
