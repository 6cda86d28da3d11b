// drx_window.hip -- a window of every waveform, at per-waveform offsets, straight from the encoded stream (drx_decode_window):
// waveform g is parsed as drx_decode parses it, from its first code to the last code of its window and no further, and the
// `width` samples from a_g = start[g] + offset on go to row g of the output (`pad` where the window leaves the waveform).
// The batch is not decoded to memory: a lane reads the head of its payload and writes its own row.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_decode_window(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   k_decode_window         delta filter: one LANE per waveform, 64 waveforms per wavefront.  The stream side is k_wave_stats'
//                           (drx_stats.hip): a per-lane word-major reversed LDS ring refilled in whole 128-byte lines, each
//                           requested once, one piece in flight; a 64-bit window gives two codes per ring access; escape and
//                           ordinary codes share one extraction.  This file has its own copy of that parse, as drx_transcode.hip
//                           has: here a lane ENDS EARLY, behind sample e_g = min(a_g + width, len_g), and requests no piece
//                           once it is through -- a wavefront runs wave_max(e_g) samples, so a head window fetches the head of
//                           every payload.  The ring (16 896 bytes) is all the LDS there is: the stores need no staging.
//   k_decode_window_serial  every other prediction filter: one lane per waveform, the serial loop of k_wave_stats_serial with
//                           the filter's history in an LDS column, stopping at the window's end.  Correct, not tuned.
//
// Few long waveforms (the nEDM / NOPTREX shapes: a few thousand waveforms of 10^5 - 10^6 samples) go through the same
// lane-per-waveform kernels.  That is correct and slow, 50-60 ns per sample and lane whatever else runs, with most of the
// chip idle: the open step drx_decode_select documents.  A wavefront or workgroup per long waveform is not built here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"

namespace drx {

// Samples [s, e) of the waveform go to row elements [pf, pf + e - s); pad fills [0, pf) and [pf + e - s, width).  A window
// that holds no sample of the waveform is s = e = 0, pf = width: the lane parses nothing.
struct Win {
    uint32_t s, e, pf;
};
__device__ __forceinline__ Win window_of(const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset, uint32_t width,
                                         uint64_t g, uint32_t len) {
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

// row elements [from, to) = pad: dword stores between a 2-byte store at either end where the address asks for one
__device__ __forceinline__ void fill_pad(int16_t *row, uint32_t from, uint32_t to, uint32_t pad2) {
    if (from >= to) return;
    if ((((uintptr_t)row >> 1) + from) & 1u) row[from++] = (int16_t)pad2;
    for (; from + 2u <= to; from += 2u) *(uint32_t *)(row + from) = pad2;
    if (from < to) row[from] = (int16_t)pad2;
}

// Lanes map as in k_wave_stats: g = 64 * wavefront + lane (a wavefront's lanes may lie in two chunks, the short last waveform
// of a chunk is a lane like any other), or rag_order's {chunk, group of 64 waveforms} entries for a ragged plan that has them.
// wf_base: first wavefront of this launch (launch_decode_window() slices a batch whose wavefronts one launch cannot carry).
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
// Verdict.  A lane whose range reaches its waveform's last sample makes k_wave_stats' end-of-payload check.  Any other lane
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
    constexpr int RW = 64;      // ring words per lane
    constexpr int LW = 32;      // words per stream piece: one 128-byte line
    constexpr int GS = 16;      // samples per group (a refill test per group)
    constexpr int T = 64;       // samples per round (a piece is committed and the next requested per round)
    constexpr int LOG_RW = 6;
    constexpr int NV = LW / 4;  // 16-byte loads per piece
    constexpr uint32_t WMASK = (1u << 27) - 1u;
    constexpr uint32_t NEED_AT = GS + 2;  // must refill below this many words (16 codes of 25 bits: 12.5 words; a pair reads three)
    static_assert(T % GS == 0 && RW - LW >= GS + 2, "round length / ring slack");
    // row r: word w with RW - (w mod RW) == r; row 0 mirrors row RW and row -1 mirrors row RW - 1 (a pair reads
    // three consecutive words: rows r + 1, r, r - 1).  A lane reads and writes its own column only.
    __shared__ uint32_t ring_all[(RW + 2) * 64];
    uint32_t *const ring = ring_all + 64;

    const int lane = lane_id();
    const uint32_t k = G.k;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
    const uint64_t wf = wf_base + blockIdx.x;
    uint64_t g;
    bool active;
    uint32_t len = 0, n = 0;
    uint64_t S = 1;
    if (!G.uniform && G.rag_order) {
        if (wf >= G.rag_groups) return;
        const uint2 e = G.rag_order[wf];  // {chunk, group of 64 waveforms inside it}
        const ChunkDesc d = G.chunks[e.x];
        const uint32_t idx = e.y * 64u + (uint32_t)lane;
        active = idx < d.n_waves;
        g = d.wave_base + idx;
        if (active) len = (idx + 1 == d.n_waves) ? (d.n_samples - idx * d.wave_len) : d.wave_len;
    } else {
        g = wf * 64u + (uint32_t)lane;
        active = g < G.total_waves;
        if (active) len = locate(G, g).len;
    }
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

    const uint64_t A = (S & ~(uint64_t)(RW - 1)) - (uint64_t)RW;  // s0 in [RW, 2 RW)
    const uint32_t s0 = (uint32_t)(S - A);
    // the words the lane may ask for: its payload's, and no more than e codes of 25 bits take; none where it parses nothing
    const uint32_t n_max = max_payload_words(e);
    const uint32_t endw = e ? s0 + (n < n_max ? n : n_max) : 0u;
    uint32_t flw = s0 & ~(uint32_t)(LW - 1);
    const bool in_vec_ok = ((uintptr_t)in & 15u) == 0;
    uint32_t *myring = ring + lane;
    uint32_t i = 0;  // first sample of the current group

    // a piece lies inside [0, in_words) or is read word by word, zero beyond: no load leaves the caller's stream
    auto load_piece = [&](uint4 (&v)[NV]) {
        const uint64_t a = A + flw;
        if (in_vec_ok && a + (uint32_t)LW <= in_words) {
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = *reinterpret_cast<const uint4 *>(in + a + 4 * j);
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                v[j].x = (a + 4 * j + 0 < in_words) ? in[a + 4 * j + 0] : 0u;
                v[j].y = (a + 4 * j + 1 < in_words) ? in[a + 4 * j + 1] : 0u;
                v[j].z = (a + 4 * j + 2 < in_words) ? in[a + 4 * j + 2] : 0u;
                v[j].w = (a + 4 * j + 3 < in_words) ? in[a + 4 * j + 3] : 0u;
            }
        }
    };
    auto store_piece = [&](const uint4 (&v)[NV]) {
        const uint32_t r0 = (uint32_t)RW - (flw & (uint32_t)(RW - 1));
        uint32_t *dst = myring + r0 * 64u;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            dst[-(4 * j + 0) * 64] = v[j].x; dst[-(4 * j + 1) * 64] = v[j].y;
            dst[-(4 * j + 2) * 64] = v[j].z; dst[-(4 * j + 3) * 64] = v[j].w;
        }
        if (r0 == (uint32_t)RW) {
            myring[0] = v[0].x;
            myring[-64] = v[0].y;
        }
        flw += (uint32_t)LW;
    };

    uint32_t Q = 0u - 32u * s0;  // minus the bit position (relative to A)
    // Q_need: position (in Q units, Q decreases) at which this lane must have its next piece; 0x7fffffff away from Q means
    // "never" (stream exhausted, or the lane is through).  cw = (~Q) >> 5, so cw >= c  <=>  Q <= ~(32 c)
    uint32_t Q_need;
    auto more = [&]() __attribute__((always_inline)) { return flw < endw && i < e; };  // words to come, and a use for them
    auto set_limits = [&]() __attribute__((always_inline)) {
        Q_need = more() ? ~(32u * (flw - NEED_AT + 1u)) : Q - 0x7fffffffu;
    };
    auto sync_refill = [&]() __attribute__((always_inline)) {  // serve every lane that is (nearly) dry, waiting for the data
        for (;;) {
            const uint32_t avail = (flw - ((~Q) >> 5)) & WMASK;
            const bool m = more();
            if (!__any(m && avail < NEED_AT)) break;
            if (m && avail <= (uint32_t)(RW - LW)) {
                uint4 v[NV];
                load_piece(v);
                store_piece(v);
            }
            wave_sync();
        }
    };

    {   // start-up: the piece that holds word s0 and as many more as fit
        uint4 v[NV];
        for (int j = 0; j < RW / LW; ++j) {
            if (__ballot(flw < endw && flw + (uint32_t)LW <= s0 + (uint32_t)RW) == 0) break;
            if (flw < endw && flw + (uint32_t)LW <= s0 + (uint32_t)RW) {
                load_piece(v);
                store_piece(v);
            }
        }
        wave_sync();
    }

    // ONE piece per lane is in flight (k_wave_stats): requested at a round's end as soon as the lane holds none and has groups
    // to come, committed at the first round end (or refill test) at which it fits, avail <= RW - LW.  Every line of a stream is
    // requested once, by one lane.  A piece still in flight when its lane is through is dropped.
    uint4 pv[NV];
    bool pneed = false;
    auto commit_if_fits = [&]() __attribute__((always_inline)) {  // the rows a piece overwrites must have been consumed
        const uint32_t avail = (flw - ((~Q) >> 5)) & WMASK;
        if (pneed && avail <= (uint32_t)(RW - LW)) {
            store_piece(pv);
            pneed = false;
        }
    };
    auto group_refill = [&]() __attribute__((always_inline)) {
        if (__any((int32_t)(Q - Q_need) <= 0)) {  // one signed compare per test (positions are mod 2^32)
            commit_if_fits();  // (a lane short of words has room for its piece: NEED_AT <= RW - LW)
            wave_sync();
            sync_refill();  // loads only where a lane is still short: it held no piece, or eats more than one per round
            set_limits();
        }
    };

    const uint32_t steps = wave_max_u32(e);
    int32_t acc = 0;     // running sum of the deltas: the sample in its low 16 bits
    uint32_t carry = 0;  // the last pair of the group before
    bool over = false;   // the position passed the words the lane fetched
    set_limits();
    for (; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (i + (uint32_t)GS <= e) {
            // ---- the unmasked group: eight pairs.  Two samples per ring access: a 64-bit window (three words) always holds
            // two codes (2 x 25 bits), so the second sample's window is one v_alignbit away from the first one's length
            uint32_t pr[GS / 2];  // the group's samples, two to a register (the earlier one in the low half)
#pragma unroll
            for (int u = 0; u < GS; u += 2) {
                const uint32_t rw = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)LOG_RW);
                const uint32_t *wp = myring + rw * 64u;
                const uint32_t lo = wp[0], hi = wp[64], lo2 = wp[-64];
                const uint32_t winA = __builtin_amdgcn_alignbit(hi, lo, Q);
                const uint32_t winB = __builtin_amdgcn_alignbit(lo, lo2, Q);
                const uint32_t q1 = ffbh(winA);
                const uint32_t kk1 = (winA < (1u << 24)) ? 16u : k;
                const uint32_t nu1 = ~(q1 + kk1);  // minus the code length
                const uint32_t win2 = __builtin_amdgcn_alignbit(winA, winB, nu1);
                const uint32_t q2 = ffbh(win2);
                const uint32_t kk2 = (win2 < (1u << 24)) ? 16u : k;
                const uint32_t nu2 = ~(q2 + kk2);
                // v_bfe_u32 and v_alignbit_b32 read 5 bits of their offset / shift: ~t == 31 - t (mod 32) serves both
                asm("v_add3_u32 %0, %1, %2, %3" : "=v"(Q) : "v"(Q), "v"(nu1), "v"(nu2));
                const uint32_t z1 = (q1 << kk1) + __builtin_amdgcn_ubfe(winA, nu1, kk1);  // escape: 8 << 16 stays above bit 15
                const uint32_t z2 = (q2 << kk2) + __builtin_amdgcn_ubfe(win2, nu2, kk2);
                acc += (int32_t)(z1 >> 1) ^ -(int32_t)(z1 & 1u);
                const uint32_t a1 = (uint32_t)acc;
                acc += (int32_t)(z2 >> 1) ^ -(int32_t)(z2 & 1u);
                pr[u / 2] = __builtin_amdgcn_perm((uint32_t)acc, a1, 0x05040100u);  // low halves of the two running sums
            }
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
                    const uint32_t rw = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)LOG_RW);
                    const uint32_t *wp = myring + rw * 64u;
                    const uint32_t lo = wp[0], hi = wp[64];
                    const uint32_t win = __builtin_amdgcn_alignbit(hi, lo, Q);
                    const uint32_t q = ffbh(win);  // win == 0 only past the end of a corrupt stream
                    const uint32_t kk = (win < (1u << 24)) ? 16u : k;
                    const uint32_t used = q + kk + 1u;
                    const uint32_t z = (q << kk) + __builtin_amdgcn_ubfe(win, 32u - used, kk);
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    Q -= used;
                    if (idx >= s) rs[idx] = (int16_t)(uint16_t)acc;
                }
            }
        }
        over |= ((flw - ((~Q) >> 5)) & WMASK) > (uint32_t)RW;
        if ((i & (uint32_t)(T - 1)) == (uint32_t)(T - GS)) {  // a round's end
            wave_sync();
            commit_if_fits();
            wave_sync();
            set_limits();
            if (!pneed) {
                pneed = flw < endw && i + (uint32_t)GS < e;  // no lane requests a piece once it is through
                if (pneed) load_piece(pv);
            }
        }
    }
    if (!e) return;
    // bits = -Q - 32 s0 (Q counts from A), positions are kept mod 2^32
    const uint32_t used_words = (((0u - Q) - 32u * s0 + 31u) >> 5) & WMASK;
    bool bad;
    if (e == len) {
        // A valid waveform's codes end inside its last payload word, n_i = ceil(bits / 32) (src/deltaRice.c:237-241), and every
        // word of it has been through the ring by then (k_wave_stats)
        bad = used_words != (n & WMASK) || flw < endw;
    } else {
        // the window's codes lay inside the payload: the exact end position from its distance to flw (at most a ring)
        const uint32_t d = (flw - (s0 + used_words)) & WMASK;
        const int32_t sd = (int32_t)(d << 5) >> 5;
        bad = over || (uint64_t)flw - (uint64_t)(int64_t)sd > (uint64_t)s0 + n;
    }
    if (bad) atomicOr(&st->err, kErrCorrupt);
}

// General prediction filters: a lane per waveform, the loop of k_wave_stats_serial (global loads); the last 64 outputs of every
// lane in an LDS column (taps <= DRX_MAX_TAPS = 64).  2-byte stores.
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
    const uint32_t k = G.k;
    uint64_t win = 0;
    uint32_t have = 0;
    uint64_t wi = 0;
    int32_t acc = 0;
    for (uint32_t i = 0; i < w.e; ++i) {
        if (have <= 32u) {
            const uint32_t v = wi < n ? s[wi] : 0u;
            ++wi;
            win |= (uint64_t)v << (32u - have);
            have += 32u;
        }
        uint32_t q = (uint32_t)__clzll((long long)win);
        q = q > 8u ? 8u : q;
        const uint32_t pl = (q == 8u) ? 16u : k;
        const uint64_t t = win << (q + 1u);
        const uint32_t rem = pl ? (uint32_t)(t >> (64u - pl)) : 0u;
        const uint32_t z = (q == 8u) ? rem : ((q << k) + rem);
        const int32_t d = (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);  // un-zig-zag (:172-177)
        if (G.n_taps == 0) {
            acc += d;  // running sum (:80-89)
        } else {
            // general inverse (:92-101): y[i] = (int16)((int16)(d[i] - sum_{j>=1} taps[j] y[i-j]) / taps[0])
            uint32_t a = (uint32_t)(int32_t)(int16_t)d;
            for (uint32_t j = 1; j < G.n_taps && j <= i; ++j) a -= (uint32_t)(int32_t)hist[(i - j) & 63u][lane] * (uint32_t)G.taps[j];
            acc = (int32_t)(int16_t)(uint16_t)a / G.taps[0];
            hist[i & 63u][lane] = (int16_t)acc;
        }
        if (i >= w.s) rs[i] = (int16_t)acc;  // the sample drx_decode writes
        const uint32_t used = q + 1u + pl;
        win <<= used;
        have -= used;
    }
    const uint64_t words = (32ull * wi - have + 31u) >> 5;  // the payload words the codes took
    if (w.e == r.len ? words != n : words > n) atomicOr(&st->err, kErrCorrupt);
}

// A launch carries fewer than 2^32 threads: at most this many wavefronts of 64 lanes go into one, a larger batch into several
constexpr uint64_t kWindowMaxGrid = 1ull << 25;

hipError_t launch_decode_window(const Geom &G, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                uint64_t *d_wave_off, uint32_t *d_wave_words, bool tables_ready, void *d_pw,
                                const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width, int16_t pad,
                                DevStatus *d_status, int16_t *d_out, uint64_t out_stride, hipEvent_t *ev, hipStream_t s) {
    if (G.total_waves == 0) return hipSuccess;
    mark(ev, 0, s);
    // ---- the walk (drx_walk.hip), as launch_wave_stats() runs it
    if (!tables_ready) {
        const WalkRoute R = route_walk(G, false, d_pw != nullptr);
        if (R.chunk_wide || R.blocks) {
            const hipError_t e = walk_scratch_reset(G, d_pw, s);
            if (e != hipSuccess) return e;
            if (R.chunk_wide) launch_walk_chunk_wide(G, d_in, in_words, d_chunk_word_off, d_wave_off, d_wave_words, d_status, d_pw, R.by_chains, s);
            if (R.blocks) launch_walk_blocks(G, d_in, in_words, d_chunk_word_off, d_wave_off, d_wave_words, d_status, d_pw, s);
        } else {
            launch_walk_serial(G, d_in, in_words, d_chunk_word_off, d_wave_off, d_wave_words, d_status, s);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    mark(ev, 1, s);
    // ---- the kernel: a wavefront per 64 waveforms
    const bool serial = G.n_taps != 0;
    const uint64_t n_wf = (!serial && !G.uniform && G.rag_order) ? (uint64_t)G.rag_groups : (G.total_waves + 63u) / 64u;
    const uint32_t pad2 = (uint32_t)(uint16_t)pad * 0x10001u;
    for (uint64_t base = 0; base < n_wf; base += kWindowMaxGrid) {
        const unsigned nb = (unsigned)std::min<uint64_t>(n_wf - base, kWindowMaxGrid);
        if (serial)
            k_decode_window_serial<<<nb, 64, 0, s>>>(G, d_in, d_wave_off, d_wave_words, base, d_start, start_stride, offset, width, pad2,
                                                     d_status, d_out, out_stride);
        else
            k_decode_window<<<nb, 64, 0, s>>>(G, d_in, in_words, d_wave_off, d_wave_words, base, d_start, start_stride, offset, width,
                                              pad2, d_status, d_out, out_stride);
    }
    mark(ev, 2, s);
    mark(ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
