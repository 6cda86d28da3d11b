// drx_select.hip -- decode SELECTED waveforms of a batch (drx_decode_select): the unit of work is one waveform of the
// caller's list, not 64 consecutive waveforms (k_decode_lanes) or every block of every waveform (drx_blocks.hip).
//
// The header tables (wave_off / wave_words) are valid for the chunks the selection touches: the host walks those chunks
// alone (launch_select_walk(), drx_walk.hip) before this launch.
//
//   k_decode_select   delta filter: one WAVEFRONT per selected waveform, the parse parallel inside the waveform by the
//                     method of k_decode_long (a lane per 16-word segment of a 1024-word block: guess, re-synchronise from
//                     the predecessor's end until no start changes, prefix sums, emit), with the workgroup's barriers
//                     and LDS exchanges replaced by what a single wavefront has: lock step, DPP scans, lane reads.
//   k_select_serial   every other prediction filter: one LANE per selected waveform, the serial parse inside the serial
//                     kernels' frame (serial_frame(), drx_lane_stream.h).  Correct, not tuned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"

namespace drx {

constexpr int kSelSeg = 16;  // words per lane and block
constexpr int kSelOv = 2;    // words of the next segment kept below a lane's column (a code has <= 25 bits)
constexpr uint32_t kSelSegBits = kSelSeg * 32u;
constexpr uint32_t kSelBlockWords = 64u * kSelSeg;
constexpr uint32_t kSelGuessBits = 160;  // bits in front of a segment's end from which the first guess is parsed
// rows in REVERSE word order plus one unused row on top and two below (k_decode_long's layout: with the bit position kept
// negated, Q = -pos, the row pair (Q >> 5, Q >> 5 + 1) holds the 32-bit window on and off a word boundary; a lane that has
// left its segment keeps reading at its last position, up to 49 bits past it)
constexpr uint32_t kSelRows = kSelSeg + kSelOv + 3;

// value of lane `src` (uniform) in every lane
__device__ __forceinline__ uint32_t lane_read(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }

__global__ __launch_bounds__(64) void k_decode_select(Geom G, const uint32_t *__restrict__ in,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words,
                                                      const uint64_t *__restrict__ sel, uint64_t n_sel, DevStatus *st,
                                                      int16_t *__restrict__ out, uint64_t stride) {
    constexpr uint32_t NT = 64;
    __shared__ uint32_t col[kSelRows * NT];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = G.k;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream (k_gather_scan's rule)
    if (st->err) return;

    for (uint64_t e = blockIdx.x; e < n_sel; e += gridDim.x) {
        const uint64_t g = sel[e];
        if (g >= G.total_waves) continue;  // (the host checked the list; never index the tables with anything else)
        const WaveRef r = locate(G, g);
        const uint32_t *src = in + wave_off[g] + 1;
        const uint32_t n = wave_words[g];
        int16_t *y = out + e * stride;
        const uint32_t len = r.len;
        uint32_t blk_word = 0;  // first word of the block
        uint32_t carry_in = 0;  // bit of lane 0's segment at which the next code starts
        uint32_t done = 0;      // samples written
        uint32_t acc_base = 0;  // running sum before the block (mod 2^16)
        uint64_t end_bits = 0;  // where the code of the last sample ended, in bits of the payload

        // parses this lane's segment from bit `start`; a code is taken when it STARTS inside the segment and inside the
        // stream.  emit: add to the running sum `acc` and store sample number idx, idx + 1, ...; last_end: where the code
        // of sample len - 1 ended (a bit of this segment), if this lane took it
        auto parse = [&](bool enable, uint32_t start, uint32_t avail_bits, auto emit_tag, uint32_t idx, uint32_t acc,
                         uint32_t &end, uint32_t &cnt, uint32_t &sum, uint32_t &last_end) __attribute__((always_inline)) {
            constexpr bool EMIT = decltype(emit_tag)::value;
            uint32_t c = 0, sacc = EMIT ? acc : 0u;
            uint32_t Q = 0u - start;  // minus the bit position
            const uint32_t lim = avail_bits < kSelSegBits ? avail_bits : kSelSegBits;
            const int32_t nlim = enable ? -(int32_t)lim : 1;  // a code is taken while -Q < lim, i.e. Q > -lim
            // EMIT: two samples per store where they fill an aligned dword; a row may start at either half of one
            const uint32_t par4 = (uint32_t)(((uintptr_t)y >> 1) & 1u);
            uint32_t held = 0, held_i = 0;  // the sample waiting for its partner
            bool holding = false;
            const uint32_t row0 = lds_addr(col) + ((kSelRows - 2u) * NT + tid) * 4u;  // this lane's row of word 0
            while (__any((int32_t)Q > nlim)) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {  // one vote per four codes
                    const bool act = (int32_t)Q > nlim;
                    typedef const uint32_t __attribute__((address_space(3))) lds_cu32;
                    const lds_cu32 *wp = (const lds_cu32 *)(uintptr_t)(row0 + (uint32_t)(((int32_t)Q >> 5) * (int32_t)(NT * 4u)));
                    const uint32_t lo = wp[0], hi = wp[NT];
                    const uint32_t win = __builtin_amdgcn_alignbit(hi, lo, Q);
                    const uint32_t q = ffbh(win);  // all-zero window (padding): the hardware's -1 is as good as any
                    const uint32_t kk = (win < (1u << 24)) ? 16u : k;
                    const uint32_t nu = ~(q + kk);  // minus the code length
                    const uint32_t z = (q << kk) + __builtin_amdgcn_ubfe(win, nu, kk);
                    const uint32_t d = (z >> 1) ^ (0u - (z & 1u));
                    const uint32_t s2 = sacc + d;
                    if (EMIT) {
                        if (act && idx + c < len) {
                            const uint32_t i = idx + c;
                            if (i + 1u == len) last_end = 0u - (Q + nu);
                            if (((i + par4) & 1u) == 0u) {  // low half of an aligned dword: wait for the next sample
                                held = s2 & 0xffffu;
                                held_i = i;
                                holding = true;
                            } else if (holding) {
                                *reinterpret_cast<uint32_t *>(y + i - 1u) = held | (s2 << 16);
                                holding = false;
                            } else {
                                y[i] = (int16_t)(uint16_t)s2;  // the lane's first sample sits in a high half
                            }
                        }
                    }
                    sacc = act ? s2 : sacc;
                    Q = act ? Q + nu : Q;
                    c += act ? 1u : 0u;
                }
            }
            if (EMIT && holding) y[held_i] = (int16_t)(uint16_t)held;  // the lane's last sample had no partner
            end = 0u - Q;
            cnt = c;
            sum = sacc;
        };

        while (done < len && blk_word < n) {
            // the block's words, transposed into per-lane columns; the first kSelOv words of segment s + 1 repeat below column s.
            // All loads first, at an index clamped into the payload (blk_word < n), so that they are in flight together: a
            // load per guarded branch waits for each in turn, sixteen memory latencies per block
            uint32_t wv16[kSelSeg];
#pragma unroll
            for (int rr = 0; rr < kSelSeg; ++rr) {
                const uint32_t at = blk_word + tid + NT * (uint32_t)rr;
                wv16[rr] = src[at < n ? at : n - 1u];
            }
#pragma unroll
            for (int rr = 0; rr < kSelSeg; ++rr) {
                const uint32_t j = tid + NT * (uint32_t)rr;
                const uint32_t wvl = (blk_word + j < n) ? wv16[rr] : 0u;
                const uint32_t sgm = j / kSelSeg, i = j % kSelSeg;
                col[(kSelRows - 2u - i) * NT + sgm] = wvl;
                if (i < (uint32_t)kSelOv && sgm >= 1u) col[(kSelRows - 2u - ((uint32_t)kSelSeg + i)) * NT + sgm - 1u] = wvl;
            }
            if (tid < (uint32_t)kSelOv) {
                const uint32_t wi = blk_word + kSelBlockWords + tid;
                col[(kSelRows - 2u - ((uint32_t)kSelSeg + tid)) * NT + NT - 1u] = (wi < n) ? src[wi] : 0u;
            }
            wave_sync();
            const uint32_t seg_word = blk_word + tid * kSelSeg;
            const uint32_t avail_bits = seg_word < n ? ((n - seg_word) > (1u << 26) ? 0xffffffffu : (n - seg_word) * 32u) : 0u;

            // first guess: only where the segment's last code ends is wanted, and a parse re-synchronises within a few
            // codes, so the guess starts kSelGuessBits before the segment's end (lane 0 knows its start)
            uint32_t start = tid == 0 ? carry_in : kSelSegBits - kSelGuessBits, end, cnt, sum, unused = 0;
            parse(true, start, avail_bits, std::false_type{}, 0u, 0u, end, cnt, sum, unused);
            for (uint32_t it = 0; it < NT; ++it) {
                // where the predecessor's last code ended, as a bit of MY segment (kSelSegBits = "nothing left for me")
                const uint32_t pe = (uint32_t)__shfl_up((int)end, 1);
                const uint32_t ns = tid == 0 ? carry_in : (pe >= kSelSegBits ? pe - kSelSegBits : kSelSegBits);
                const bool changed = ns != start;
                if (!__any(changed)) break;
                start = ns;
                uint32_t e2, c2, s2;
                parse(changed, start, avail_bits, std::false_type{}, 0u, 0u, e2, c2, s2, unused);
                if (changed) { end = e2; cnt = c2; sum = s2; }
            }
            // prefix sums over the wavefront: samples before my segment, sum of deltas before my segment
            const uint32_t incl_c = wave_incl_scan_dpp(cnt), incl_s = wave_incl_scan_dpp(sum);
            const uint32_t tot_c = lane_read(incl_c, 63), tot_s = lane_read(incl_s, 63), end_last = lane_read(end, 63);
            uint32_t e3, c3, s3, last_end = 0xffffffffu;
            parse(true, start, avail_bits, std::true_type{}, done + incl_c - cnt, acc_base + incl_s - sum, e3, c3, s3, last_end);
            // (one lane at most took the waveform's last sample)
            const uint64_t took = __ballot(last_end != 0xffffffffu);
            if (took) {
                const int w = (int)__builtin_ctzll(took);
                end_bits = ((uint64_t)blk_word + (uint32_t)w * kSelSeg) * 32u + lane_read(last_end, w);
            }
            done = (tot_c > len - done) ? len : done + tot_c;
            acc_base += tot_s;
            carry_in = end_last >= kSelSegBits ? end_last - kSelSegBits : 0u;
            blk_word += kSelBlockWords;
            wave_sync();  // (the next block's words replace this one's)
        }
        // the stream ended before the waveform did, or its codes do not end in its last payload word
        // (n_i = ceil(bits / 32), src/deltaRice.c:237-241)
        if (tid == 0 && len && (done < len || ((end_bits + 31u) >> 5) != n)) atomicOr(&st->err, kErrCorrupt);
    }
}

// General prediction filters: serial_frame() (drx_lane_stream.h) over the selection as its list -- lane e of the launch takes
// waveform sel[e] (the host checked the list; never index the tables with anything else) and writes row e by 2-byte stores.
__global__ __launch_bounds__(64) void k_select_serial(Geom G, const uint32_t *__restrict__ in,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words,
                                                      const uint64_t *__restrict__ sel, uint64_t n_sel, DevStatus *st,
                                                      int16_t *__restrict__ out, uint64_t stride) {
    int16_t *const y = out + ((uint64_t)blockIdx.x * 64u + threadIdx.x) * stride;
    serial_frame(
        G, in, wave_off, wave_words, 0u, sel, n_sel, st, [](uint64_t, const WaveRef &r) { return r.len; },
        [&](uint32_t i, int16_t v) __attribute__((always_inline)) { y[i] = v; }, [](uint64_t, const WaveRef &) {});
}

// A wavefront per entry up to kSelMaxGrid wavefronts (a selection of one launches one), which then stride over the list.
constexpr uint64_t kSelMaxGrid = 1u << 20;

hipError_t launch_decode_select(const StreamCall &c, const uint64_t *d_sel, uint64_t n_sel, int16_t *d_out, uint64_t stride) {
    if (!n_sel) return hipSuccess;
    const Geom &G = *c.G;
    if (G.n_taps == 0)
        k_decode_select<<<(unsigned)std::min<uint64_t>(n_sel, kSelMaxGrid), 64, 0, c.s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, d_sel, n_sel,
                                                                                      c.d_status, d_out, stride);
    else
        k_select_serial<<<blocks_for(n_sel, 64), 64, 0, c.s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, d_sel, n_sel, c.d_status, d_out, stride);
    return hipGetLastError();
}

}  // namespace drx
