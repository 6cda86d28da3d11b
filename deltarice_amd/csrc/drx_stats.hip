// drx_stats.hip -- per-waveform statistics straight from the encoded stream (drx_wave_stats): every waveform is parsed as
// drx_decode parses it, and reduced to eight int64 values (DRX_STAT_* of include/deltarice_hip.h) instead of being written out.
// The batch is read once (the stream) and 64 bytes per waveform are written; no sample goes to memory.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_wave_stats(): the walks of drx_walk.hip, or the side-band's tables).
//
//   k_wave_stats         delta filter: one LANE per waveform, 64 waveforms per wavefront.  The stream side is k_decode_lanes'
//                        (drx_decode_kernels.hip): a per-lane word-major reversed LDS ring refilled in
//                        whole 128-byte lines, each requested once; a 64-bit window gives two codes per ring access; escape
//                        and ordinary codes share one extraction.  What the decoder needs for its STORES is absent: no
//                        transposition buffer, no start delay, no edge rounds, no write-out -- a lane starts at its first
//                        sample and stops behind its last, and the ring (16 896 bytes) is all the LDS there is.
//   k_wave_stats_serial  every other prediction filter: one lane per waveform, the serial loop of k_select_serial
//                        (drx_select.hip) with the filter's history in an LDS column.  Correct, not tuned.
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

namespace drx {

typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_pair(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ uint32_t as_word(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
constexpr int32_t kNarrow = 16383;  // sixteen squares of samples within +-kNarrow sum to less than 2^32
static_assert(16ll * kNarrow * kNarrow < (1ll << 32), "a narrow group's sum of squares fits 32 bits");

// a lane's row: eight int64, by 16-byte stores where the caller's buffer allows them (a row is 64 bytes, so every row of a
// 16-byte aligned buffer is), by 8-byte stores otherwise (the ABI asks 8-byte alignment of d_out)
__device__ __forceinline__ void store_row(int64_t *__restrict__ out, uint64_t g, bool vec, const int64_t (&v)[DRX_STAT_COLS]) {
    int64_t *row = out + g * (uint64_t)DRX_STAT_COLS;
    if (vec) {
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        typedef u32x4v __attribute__((address_space(1))) g_uint4;
        g_uint4 *dst = (g_uint4 *)row;
#pragma unroll
        for (int j = 0; j < DRX_STAT_COLS / 2; ++j)
            dst[j] = (u32x4v){(uint32_t)v[2 * j], (uint32_t)((uint64_t)v[2 * j] >> 32), (uint32_t)v[2 * j + 1], (uint32_t)((uint64_t)v[2 * j + 1] >> 32)};
    } else {
#pragma unroll
        for (int j = 0; j < DRX_STAT_COLS; ++j) row[j] = v[j];
    }
}

// Lanes map plainly, g = 64 * wavefront + lane (chunks need no alignment to wavefronts: a wavefront's lanes may lie in two
// chunks, and the short last waveform of a chunk is a lane like any other); a ragged plan that has rag_order takes its
// {chunk, group of 64 waveforms} entries instead, longest WaveformLength first (a lane takes ~60 ns per sample, so the
// wavefronts of the longest waveforms must not start last).  wf_base: first wavefront of this launch (launch_wave_stats()
// slices a batch whose wavefronts one launch cannot carry).
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
    if (active) {
        S = wave_off[g] + 1u;
        n = wave_words[g];
    }

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

    // ONE piece per lane is in flight, as in the decoder: requested at a round's end as soon as the lane holds none, committed
    // at the first round end (or refill test) at which it fits, avail <= RW - LW; until then it stays in its registers.  Every
    // line of a stream is requested once, by one lane, by the NV loads of one round.  A piece still in flight when its lane
    // is through is dropped: it lay inside the lane's own stream.
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
            // ---- the unmasked group: eight pairs.  Two samples per ring access: a 64-bit window (three words) always holds
            // two codes (2 x 25 bits), so the second sample's window is one v_alignbit away from the first one's length
            uint32_t pr[GS / 2];  // the group's samples, two to a register (the earlier one in the low half)
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
                pr[u / 2] = __builtin_amdgcn_perm((uint32_t)acc, a1, 0x05040100u);  // low halves of the two running sums
            }
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
    if (h == len) { hsum = sum; hsq = sq; }  // the window holds the whole waveform
    // A valid waveform's codes end inside its last payload word, n_i = ceil(bits / 32) (src/deltaRice.c:237-241), and every
    // word of it has been through the ring by then; bits = -Q - 32 s0 (Q counts from A), positions are kept mod 2^32.  A
    // payload that ends before its samples do, or whose codes do not end in its last word, fails one of the two.
    if (len && (((((0u - Q) - 32u * s0 + 31u) >> 5) & WMASK) != (n & WMASK) || flw < endw)) atomicOr(&st->err, kErrCorrupt);
    const int64_t v[DRX_STAT_COLS] = {(int64_t)mn, (int64_t)amn, (int64_t)mx, (int64_t)amx, sum, (int64_t)sq, hsum, (int64_t)hsq};
    store_row(out, g, ((uintptr_t)out & 15u) == 0, v);
}

// General prediction filters: a lane per waveform, the loop of k_select_serial (global loads); the last 64 outputs of every
// lane in an LDS column (taps <= DRX_MAX_TAPS = 64).
// list != nullptr: the waveforms list[0 .. *n_list) instead of all of them (behind the block form, drx_stats_blocks.hip: the
// list and its length are written on the device by the kernel in front; the launch is sized for the whole batch).
__global__ __launch_bounds__(64) void k_wave_stats_serial(Geom G, const uint32_t *__restrict__ in,
                                                          const uint64_t *__restrict__ wave_off,
                                                          const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                          uint32_t head_len, DevStatus *st, int64_t *__restrict__ out,
                                                          const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    const uint32_t lane = threadIdx.x;
    uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;  // (as k_wave_stats)
    if (list) {
        if (g >= (uint64_t)*n_list) return;
        g = list[g];
    }
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    const uint32_t *s = in + wave_off[g] + 1;
    const uint32_t n = wave_words[g];
    const uint32_t k = G.k;
    const uint32_t h = head_len < r.len ? head_len : r.len;
    uint64_t win = 0;
    uint32_t have = 0, wi = 0;
    int32_t acc = 0;
    int32_t mn = 0x7fffffff, mx = -0x7fffffff - 1;
    uint32_t amn = 0, amx = 0;
    int64_t sum = 0, hsum = 0;
    uint64_t sq = 0, hsq = 0;
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
        if (i == h) { hsum = sum; hsq = sq; }
        const int32_t y = (int32_t)(int16_t)acc;  // the sample drx_decode writes
        sum += y;
        sq += (uint64_t)(uint32_t)(y * y);
        if (y < mn) { mn = y; amn = i; }
        if (y > mx) { mx = y; amx = i; }
        const uint32_t used = q + 1u + pl;
        win <<= used;
        have -= used;
    }
    if (h == r.len) { hsum = sum; hsq = sq; }
    const uint64_t bits = 32ull * wi - have;
    if (r.len && ((bits + 31u) >> 5) != n) atomicOr(&st->err, kErrCorrupt);
    const int64_t v[DRX_STAT_COLS] = {(int64_t)mn, (int64_t)amn, (int64_t)mx, (int64_t)amx, sum, (int64_t)sq, hsum, (int64_t)hsq};
    store_row(out, g, ((uintptr_t)out & 15u) == 0, v);
}

// A launch carries fewer than 2^32 threads: at most this many wavefronts of 64 lanes go into one, a larger batch into several
constexpr uint64_t kStatsMaxGrid = 1ull << 25;

hipError_t launch_wave_stats(const Geom &G, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             uint64_t *d_wave_off, uint32_t *d_wave_words, bool tables_ready, void *d_pw, void *d_blk, void *d_sacc,
                             uint32_t head_len, DevStatus *d_status, int64_t *d_out, hipEvent_t *ev, hipStream_t s, uint32_t *form_out) {
    const bool blocks = d_sacc != nullptr && stats_blocks_batch(G, d_blk);
    if (form_out) *form_out = blocks ? (DRX_STATS_FORM_BLOCKS | ((G.dbg & DRX_DBG_STATS_ALL_FALLBACK) ? DRX_STATS_FORM_FALLBACK_ALL : 0u)) : DRX_STATS_FORM_LANES;
    if (G.total_waves == 0) return hipSuccess;
    mark(ev, 0, s);
    // ---- the walk (drx_walk.hip), all of it on this stream: nothing here is worth a fork
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
    // ---- few long waveforms: a workgroup per block of a waveform's stream, then a lane per waveform that form lists (the
    // launch is sized from here, at most a lane per waveform of the batch; the list's length is read on the device)
    if (blocks) {
        const uint32_t *listed = nullptr, *n_listed = nullptr;
        const hipError_t e = launch_stats_blocks(G, d_in, in_words, d_wave_off, d_wave_words, d_blk, d_sacc, head_len, d_status, d_out, &listed, &n_listed, s);
        if (e != hipSuccess) return e;
        k_wave_stats_serial<<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, d_in, d_wave_off, d_wave_words, 0, head_len, d_status, d_out, listed, n_listed);
        mark(ev, 2, s);
        mark(ev, 3, s);
        return hipGetLastError();
    }
    // ---- the kernel: a wavefront per 64 waveforms
    const bool serial = G.n_taps != 0;
    const uint64_t n_wf = (!serial && !G.uniform && G.rag_order) ? (uint64_t)G.rag_groups : (G.total_waves + 63u) / 64u;
    for (uint64_t base = 0; base < n_wf; base += kStatsMaxGrid) {
        const unsigned nb = (unsigned)std::min<uint64_t>(n_wf - base, kStatsMaxGrid);
        if (serial)
            k_wave_stats_serial<<<nb, 64, 0, s>>>(G, d_in, d_wave_off, d_wave_words, base, head_len, d_status, d_out, nullptr, nullptr);
        else
            k_wave_stats<<<nb, 64, 0, s>>>(G, d_in, in_words, d_wave_off, d_wave_words, base, head_len, d_status, d_out);
    }
    mark(ev, 2, s);
    mark(ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
