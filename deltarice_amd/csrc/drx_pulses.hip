// drx_pulses.hip -- every pulse of every waveform straight from the encoded stream (drx_find_pulses): threshold discrimination.
// Waveform g is parsed as drx_decode parses it; its samples are compared with a per-waveform threshold t_g, every maximal run of
// consecutive samples over it that is at least min_width long is a pulse, and the first max_pulses of them go out as records of
// DRX_PULSE_COLS int64 (start, width, peak, where the peak sits, integral) beside the count of all of them.  The batch is read
// once and no sample goes to memory.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_find_pulses(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   k_find_pulses         delta filter: one LANE per waveform, 64 waveforms per wavefront.  The stream side is k_wave_stats'
//                         (drx_stats.hip): a per-lane word-major reversed LDS ring refilled in whole 128-byte lines, each
//                         requested once, one piece in flight; a 64-bit window gives two codes per ring access; escape and
//                         ordinary codes share one extraction; the same end-of-payload check.  This file has its own copy of
//                         that parse, as drx_window.hip and drx_transcode.hip have.  New is what happens to a group's 16
//                         samples: a small state machine per lane instead of eight running reductions, behind a fast reject.
//                         The ring (16 896 bytes) is all the LDS there is.
//   k_find_pulses_serial  every other prediction filter: one lane per waveform, the serial loop of k_wave_stats_serial with
//                         the filter's history in an LDS column and the same state machine.  Correct, not tuned.
//
// Few long waveforms (the nEDM / NOPTREX shapes, the reference's default of one waveform per chunk) go through the same
// lane-per-waveform kernels.  That is correct and slow, 50-60 ns per sample and lane whatever else runs, with most of the chip
// idle.  A block form behind drx_blocks_body.inc, as drx_wave_stats has one, is not built here: a run spans block borders, so
// the blocks' open runs would have to be stitched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"

namespace drx {

typedef short s16x2 __attribute__((ext_vector_type(2)));

// One polarity.  A sample y enters the state machine as v = y ^ flip, flip = 0 for positive polarity and -1 for negative:
// ~y = -1 - y reverses the order of the int16 values without leaving them, so "y < t" is "v > -1 - t" and the minimum of a run
// is the complement of the maximum of its v.  The lane's threshold tv is clamped so that it compares as an int32 with any
// int16: positive polarity t to [-32769, 32767] (at the top nothing is over, at the bottom everything), negative polarity t to
// [-32768, 32768] and then tv = -1 - t, the same range.  The sum d_thr + thr saturates at the int64 ends.
__device__ __forceinline__ int32_t lane_threshold(const int64_t *__restrict__ thr_tab, uint64_t thr_stride, int64_t thr, bool neg,
                                                  uint64_t g) {
    int64_t t = thr;
    if (thr_tab) {
        const int64_t v = thr_tab[g * thr_stride];
        if (__builtin_add_overflow(v, thr, &t)) t = v < 0 ? INT64_MIN : INT64_MAX;
    }
    if (neg) {
        t = t < -32768 ? -32768 : (t > 32768 ? 32768 : t);
        return (int32_t)(-1 - t);
    }
    return (int32_t)(t < -32769 ? -32769 : (t > 32767 ? 32767 : t));
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

// Lanes map as in k_wave_stats: g = 64 * wavefront + lane (a wavefront's lanes may lie in two chunks, the short last waveform
// of a chunk is a lane like any other), or rag_order's {chunk, group of 64 waveforms} entries for a ragged plan that has them.
// wf_base: first wavefront of this launch (launch_find_pulses() slices a batch whose wavefronts one launch cannot carry).
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
    PulseLane P;
    P.tv = 32767;
    P.min_width = min_width;
    P.max_pulses = max_pulses;
    P.flip = neg ? -1 : 0;
    P.slots = out;
    P.open = false;
    P.s = P.apk = 0;
    P.peak = 0;
    P.sum = 0;
    P.count = 0;
    if (active) {
        S = wave_off[g] + 1u;
        n = wave_words[g];
        P.tv = lane_threshold(thr_tab, thr_stride, thr, neg != 0u, g);
        P.slots = out + g * (uint64_t)max_pulses * (uint64_t)DRX_PULSE_COLS;  // (never followed where max_pulses == 0)
    }
    const uint32_t pm = neg ? 0xffffffffu : 0u;  // flip of a pair

    const uint64_t A = (S & ~(uint64_t)(RW - 1)) - (uint64_t)RW;  // s0 in [RW, 2 RW)
    const uint32_t s0 = (uint32_t)(S - A);
    const uint32_t endw = s0 + n;
    uint32_t flw = s0 & ~(uint32_t)(LW - 1);
    const bool in_vec_ok = ((uintptr_t)in & 15u) == 0;
    uint32_t *myring = ring + lane;

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
    // "never" (stream exhausted).  cw = (~Q) >> 5, so cw >= c  <=>  Q <= ~(32 c)
    uint32_t Q_need;
    auto set_limits = [&]() __attribute__((always_inline)) {
        const bool more = flw < endw;
        Q_need = more ? ~(32u * (flw - NEED_AT + 1u)) : Q - 0x7fffffffu;
    };
    auto sync_refill = [&]() __attribute__((always_inline)) {  // serve every lane that is (nearly) dry, waiting for the data
        for (;;) {
            const uint32_t avail = (flw - ((~Q) >> 5)) & WMASK;
            const bool more = flw < endw;
            if (!__any(more && avail < NEED_AT)) break;
            if (more && avail <= (uint32_t)(RW - LW)) {
                uint4 v[NV];
                load_piece(v);
                store_piece(v);
            }
            wave_sync();
        }
    };

    {   // start-up: the piece that holds word s0 and as many more as fit
        uint4 v[NV];
        for (int i = 0; i < RW / LW; ++i) {
            if (__ballot(flw < endw && flw + (uint32_t)LW <= s0 + (uint32_t)RW) == 0) break;
            if (flw < endw && flw + (uint32_t)LW <= s0 + (uint32_t)RW) {
                load_piece(v);
                store_piece(v);
            }
        }
        wave_sync();
    }

    // ONE piece per lane is in flight (k_wave_stats): requested at a round's end as soon as the lane holds none, committed at
    // the first round end (or refill test) at which it fits, avail <= RW - LW; until then it stays in its registers.  Every
    // line of a stream is requested once, by one lane.  A piece still in flight when its lane is through is dropped: it lay
    // inside the lane's own stream.
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

    const uint32_t steps = wave_max_u32(len);
    int32_t acc = 0;  // running sum of the deltas: the sample in its low 16 bits
    set_limits();
    for (uint32_t i = 0; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (i + (uint32_t)GS <= len) {
            // ---- the unmasked group: eight pairs.  Two samples per ring access: a 64-bit window (three words) always holds
            // two codes (2 x 25 bits), so the second sample's window is one v_alignbit away from the first one's length
            uint32_t pr[GS / 2];  // the group's v, two to a register (the earlier one in the low half)
#pragma unroll
            for (int u = 0; u < GS; u += 2) {
                const uint32_t row = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)LOG_RW);
                const uint32_t *wp = myring + row * 64u;
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
                pr[u / 2] = __builtin_amdgcn_perm((uint32_t)acc, a1, 0x05040100u) ^ pm;  // low halves of the two running sums
            }
            s16x2 gm = __builtin_bit_cast(s16x2, pr[0]);
#pragma unroll
            for (int j = 1; j < GS / 2; ++j) gm = __builtin_elementwise_max(gm, __builtin_bit_cast(s16x2, pr[j]));
            const int32_t gmax = gm.x > gm.y ? (int32_t)gm.x : (int32_t)gm.y;
            if (P.open || gmax > P.tv) {
                // the registers rotate: pr[0] is the pair in turn
#pragma unroll 1
                for (uint32_t u = 0; u < (uint32_t)GS; u += 2u) {
                    const uint32_t p = pr[0];
#pragma unroll
                    for (int j = 0; j < GS / 2 - 1; ++j) pr[j] = pr[j + 1];
                    P.step((int32_t)(int16_t)(uint16_t)p, i + u);
                    P.step((int32_t)p >> 16, i + u + 1u);
                }
            }
        } else if (i < len) {
            // ---- the masked group: the lane's waveform ends inside it.  One sample per ring access.
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)GS; ++u) {
                const uint32_t idx = i + u;
                if (idx < len) {
                    const uint32_t row = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)LOG_RW);
                    const uint32_t *wp = myring + row * 64u;
                    const uint32_t lo = wp[0], hi = wp[64];
                    const uint32_t win = __builtin_amdgcn_alignbit(hi, lo, Q);
                    const uint32_t q = ffbh(win);  // win == 0 only past the end of a corrupt stream
                    const uint32_t kk = (win < (1u << 24)) ? 16u : k;
                    const uint32_t used = q + kk + 1u;
                    const uint32_t z = (q << kk) + __builtin_amdgcn_ubfe(win, 32u - used, kk);
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    Q -= used;
                    P.step((int32_t)(int16_t)(uint16_t)((uint32_t)acc ^ pm), idx);
                }
            }
        }
        if ((i & (uint32_t)(T - 1)) == (uint32_t)(T - GS)) {  // a round's end
            wave_sync();
            commit_if_fits();
            wave_sync();
            set_limits();
            if (!pneed) {
                pneed = flw < endw;
                if (pneed) load_piece(pv);
            }
        }
    }
    if (!active) return;
    if (P.open) P.close(len);  // a run still open at the last sample ends there
    // A valid waveform's codes end inside its last payload word, n_i = ceil(bits / 32) (src/deltaRice.c:237-241), and every
    // word of it has been through the ring by then; bits = -Q - 32 s0 (Q counts from A), positions are kept mod 2^32.  A
    // payload that ends before its samples do, or whose codes do not end in its last word, fails one of the two (k_wave_stats).
    if (len && (((((0u - Q) - 32u * s0 + 31u) >> 5) & WMASK) != (n & WMASK) || flw < endw)) atomicOr(&st->err, kErrCorrupt);
    count_out[g] = P.count;
}

// General prediction filters: a lane per waveform, the loop of k_wave_stats_serial (global loads); the last 64 outputs of every
// lane in an LDS column (taps <= DRX_MAX_TAPS = 64).
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
    const uint32_t k = G.k;
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
    uint64_t win = 0;
    uint32_t have = 0, wi = 0;
    int32_t acc = 0;
    for (uint32_t i = 0; i < r.len; ++i) {
        if (have <= 32u) {
            const uint32_t w = wi < n ? s[wi] : 0u;
            ++wi;
            win |= (uint64_t)w << (32u - have);
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
        P.step((int32_t)(int16_t)acc ^ fm, i);  // the sample drx_decode writes, flipped for negative polarity
        const uint32_t used = q + 1u + pl;
        win <<= used;
        have -= used;
    }
    if (P.open) P.close(r.len);
    const uint64_t bits = 32ull * wi - have;
    if (r.len && ((bits + 31u) >> 5) != n) atomicOr(&st->err, kErrCorrupt);
    count_out[g] = P.count;
}

// A launch carries fewer than 2^32 threads: at most this many wavefronts of 64 lanes go into one, a larger batch into several
constexpr uint64_t kPulsesMaxGrid = 1ull << 25;

hipError_t launch_find_pulses(const Geom &G, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              uint64_t *d_wave_off, uint32_t *d_wave_words, bool tables_ready, void *d_pw, const int64_t *d_thr,
                              uint64_t thr_stride, int64_t thr, bool neg, uint32_t min_width, uint32_t max_pulses,
                              DevStatus *d_status, uint32_t *d_count, int64_t *d_out, hipEvent_t *ev, hipStream_t s) {
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
    // ---- the zero slots: the whole output, once (the lanes then store the records alone)
    if (max_pulses) {
        const hipError_t e = hipMemsetAsync(d_out, 0, (size_t)(G.total_waves * (uint64_t)max_pulses * DRX_PULSE_COLS * sizeof(int64_t)), s);
        if (e != hipSuccess) return e;
    }
    // ---- the kernel: a wavefront per 64 waveforms
    const bool serial = G.n_taps != 0;
    const uint64_t n_wf = (!serial && !G.uniform && G.rag_order) ? (uint64_t)G.rag_groups : (G.total_waves + 63u) / 64u;
    for (uint64_t base = 0; base < n_wf; base += kPulsesMaxGrid) {
        const unsigned nb = (unsigned)std::min<uint64_t>(n_wf - base, kPulsesMaxGrid);
        if (serial)
            k_find_pulses_serial<<<nb, 64, 0, s>>>(G, d_in, d_wave_off, d_wave_words, base, d_thr, thr_stride, thr, neg ? 1u : 0u, min_width,
                                                   max_pulses, d_status, d_count, d_out);
        else
            k_find_pulses<<<nb, 64, 0, s>>>(G, d_in, in_words, d_wave_off, d_wave_words, base, d_thr, thr_stride, thr, neg ? 1u : 0u,
                                            min_width, max_pulses, d_status, d_count, d_out);
    }
    mark(ev, 2, s);
    mark(ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
