// drx_stack.hip -- the sum of selected, aligned waveforms straight from the encoded stream (drx_wave_stack): position j of the
// result, 0 <= j < width, receives sample a_g + j of every selected waveform g that has one, a_g a per-waveform origin, and row
// j holds three int64 (DRX_STACK_* of include/deltarice_hip.h: how many, their sum, the sum of their squares).  The first stream
// call that reduces ACROSS waveforms: the batch is read once (the stream, no further than every window's end) and 24 bytes per
// position are written; no sample goes to memory and there is no temporary beside the rows.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of these launches
// (launch_wave_stack(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   k_stack_rows_zero    the rows, row by row (they may be strided): (0, 0, 0)
//   k_stack_count        COUNT depends on geometry, origins and selection alone, never on the stream, so it is computed apart
//                        from the parse: a lane per waveform adds +1 at its window's first position and -1 behind its last to
//                        the COUNT column (a wavefront adds once per distinct end, not once per lane), and
//                        under a selection appends the waveforms that add something to a list (the plan's scratch, first call), and
//   k_stack_count_scan   one workgroup turns the column of differences into counts in place.
//   k_wave_stack<T>      delta filter: one LANE per waveform over the shared reader's early-ending form (drx_lane_reader.inc
//                        with DRX_LANE_EARLY, as k_decode_window), in PERSISTENT workgroups of four wavefronts that own one
//                        accumulator in LDS for a tile of T positions (int32 sum, uint64 sum of squares: 12 bytes a position),
//                        walk many groups of 64 waveforms and flush once.  Under a selection the lanes take the LISTED waveforms,
//                        64 to a wavefront: a wavefront runs as long as its longest lane, so the 54 lanes in 60 of a 10 %
//                        selection that idle beside a waveform nobody selected would cost what the whole batch costs.
//   k_wave_stack_serial  every other prediction filter: serial_frame() (drx_lane_stream.h), 64-bit atomics straight to the
//                        rows for every sample of a window.  Correct, not tuned: its atomic traffic is 16 bytes per sample.
//
// The accumulator.  Four wavefronts add into it with LDS atomics and nothing orders them until the flush.  The int32 sum is
// exact while at most 65 535 waveforms went into it (65 535 x 32 768 < 2^31): a workgroup flushes after kStackFlushEvery = 255
// rounds of its 256 lanes, 65 280 waveforms, and at its end.  The flush adds every position that received something to its row
// with two 64-bit integer atomics, consecutive lanes at consecutive positions; with 256 or 512 resident workgroups that is
// 29 or 8 MB of atomic traffic for the two tile sizes however many waveforms there are.  Integer adds: the same rows in any order.
//
// Two forms per group of 16 samples, chosen PER WAVEFRONT by a wave-uniform test of the geometry (never of the stream): the
// rows do not depend on which one runs.  In both the lanes leave their group -- eight packed pairs, zero outside the window --
// in 2 KB of LDS per wavefront and other lanes take it from there.  A per-lane LDS add per sample is not built in: with equal
// origins it is a 64-way same-address conflict on every sample, and with windows at the waveforms' maxima its 32 atomic
// instructions a group would be issued for the five lanes in 64 that are inside their windows at any one time.
//   equal     every lane that parses maps sample index to position alike (d_start == NULL, or equal origins: the whole-waveform
//             stack).  Lane (pair p, slice q) reads pair p of the eight lanes of slice q, reduces them in registers (v_dot2: the
//             squares two at a time in 32 bits, then 64), and adds its two positions to the accumulator: 8-way conflicts on
//             four adds a lane and group.
//   distinct  the lanes' positions differ.  Only the lanes that add something from this group store, in columns compacted by
//             their rank; the position of their sample i travels to the lane of that rank by one ds_permute.  The wavefront
//             then takes the (column, pair) items eight columns a step -- four LDS atomic adds a step with all 64 lanes busy,
//             one step where up to eight lanes are inside their windows, eight where all are.
//
// Tiles.  T = 512 positions (two workgroups, eight wavefronts per CU: 81 920 bytes each) where width <= 512, T = 7168 (one
// workgroup per CU, 161 792 bytes) otherwise; wider results run as more tiles across workgroups, each parsing a waveform no
// further than the smaller of its window's end and the tile's end.
//
// A width far beyond every window's reach is allowed (up to 2^32 - 1) and costs what its rows cost: the host does not know the
// origins, so every tile is launched -- its workgroups find no window and flush nothing -- and the one workgroup of
// k_stack_count_scan walks all `width` cells, 1024 a step; at the ABI's limit that is seconds.  Not clamped.
//
// The context option "stack_workgroups" (0: the resident grid) caps the workgroups of a tile, so that few waveforms drive a
// workgroup through many rounds: the tests reach the periodic flush with it.
//
// Few long waveforms (the reference's default of one waveform per chunk) are correct this way and slow: a lane per waveform,
// 50-60 ns per sample and lane, once per tile of 7168 positions.  A block form is the follow-up.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_window_rows.h"

namespace drx {

constexpr int kStackWaves = 4;                 // wavefronts of a workgroup
constexpr int kStackTileNarrow = 512;          // positions of a tile: two workgroups per CU ...
constexpr int kStackTileWide = 7168;           // ... or one
constexpr uint32_t kStackFlushEvery = 255;     // rounds of 64 * kStackWaves waveforms between two flushes
constexpr uint32_t kStackStageWords = 8 * 64;  // the equal form's transposition: eight packed pairs of 64 lanes
static_assert((uint64_t)kStackFlushEvery * 64u * kStackWaves <= 65535u, "the int32 partial sum stays exact");
static_assert(DRX_STACK_COUNT == 0 && DRX_STACK_SUM == 1 && DRX_STACK_SUMSQ == 2 && DRX_STACK_COLS == 3, "the row's order");

// The window of waveform g in samples and in positions: samples [w.s, w.e) go to positions [w.pf, w.pf + w.e - w.s).  A
// waveform that is not selected has none (s = e = 0).  (Win, window_start(), window_at(): drx_window_rows.h)
__device__ __forceinline__ Win stack_window(const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset, uint32_t width,
                                            const uint8_t *__restrict__ select, uint64_t g, uint32_t len) {
    if (select && !select[g]) return Win{0u, 0u, width};
    return window_at(window_start(start ? start[g * start_stride] : 0, offset), width, len);
}

__global__ __launch_bounds__(256) void k_stack_rows_zero(uint32_t width, int64_t *__restrict__ out, uint64_t out_stride) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= width) return;
    int64_t *row = out + j * out_stride;
    row[DRX_STACK_COUNT] = 0;
    row[DRX_STACK_SUM] = 0;
    row[DRX_STACK_SUMSQ] = 0;
}

// COUNT as a difference array in the rows' own column: no scratch.  Plain lane mapping (the order does not matter here).
__global__ __launch_bounds__(64) void k_stack_count(Geom G, uint64_t wf_base, const int64_t *__restrict__ start, uint64_t start_stride,
                                                    int64_t offset, uint32_t width, const uint8_t *__restrict__ select,
                                                    unsigned long long *__restrict__ list, int64_t *__restrict__ out,
                                                    uint64_t out_stride) {
    const int lane = lane_id();
    const uint64_t g = (wf_base + blockIdx.x) * 64u + (uint32_t)lane;
    uint32_t lo = 0, n = 0;
    if (g < G.total_waves) {
        const Win w = stack_window(start, start_stride, offset, width, select, g, locate(G, g).len);
        lo = w.pf;
        n = w.e - w.s;
    }
    // One add per wavefront and distinct end, not one per lane: windows at the waveforms' maxima begin at position 0 in nearly
    // every lane, and a million adds to one address take 13 ms
    auto add_by_value = [&](uint64_t at, bool has, unsigned long long sign) {
        uint64_t left = __ballot(has);
        while (left) {  // (uniform)
            const int first = __ffsll((unsigned long long)left) - 1;
            const uint64_t at0 = (uint64_t)__shfl((long long)at, first);
            const uint64_t same = __ballot(has && at == at0);
            if (lane == first)
                atomicAdd((unsigned long long *)(out + at0 * out_stride + DRX_STACK_COUNT), sign * (unsigned long long)__popcll((unsigned long long)same));
            left &= ~same;
            has = has && at != at0;
        }
    };
    const uint64_t hi = (uint64_t)lo + n;  // (<= width)
    // under a selection: the waveforms that add something, for the lanes of k_wave_stack (u64 n_listed | u64 listed[]: stack_list_bytes(); in no particular order)
    const uint64_t has_any = __ballot(n != 0u);
    if (list && has_any) {
        const int first = __ffsll((unsigned long long)has_any) - 1;
        unsigned long long base = 0;
        if (lane == first) base = atomicAdd(list, (unsigned long long)__popcll((unsigned long long)has_any));
        base = (unsigned long long)__shfl((long long)base, first);
        if (n != 0u) list[1u + base + __builtin_amdgcn_mbcnt_hi((uint32_t)(has_any >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)has_any, 0u))] = g;
    }
    add_by_value(lo, n != 0u, 1ull);
    add_by_value(hi, n != 0u && hi < width, ~0ull);
}

// ... and its inclusive scan in place: one workgroup, 1024 positions a step, the carry in a register of every lane
__global__ __launch_bounds__(1024) void k_stack_count_scan(uint32_t width, int64_t *__restrict__ out, uint64_t out_stride) {
    __shared__ int64_t wsum[16];
    const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
    int64_t carry = 0;
    for (uint64_t base = 0; base < width; base += 1024u) {
        const uint64_t p = base + threadIdx.x;
        int64_t *cell = out + p * out_stride + DRX_STACK_COUNT;
        int64_t v = p < width ? *cell : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) wsum[wv] = v;
        __syncthreads();
        int64_t pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int64_t t = wsum[w];
            tot += t;
            if (w < wv) pre += t;
        }
        if (p < width) *cell = carry + pre + v;
        carry += tot;
        __syncthreads();
    }
}

// Workgroup b of tile t is block t * P + b; it takes the wavefronts b * 4 + wave, + 4 P, ... of the batch's n_wf (lane_wave():
// rag_order's groups for a ragged plan that has them, longest first).  Tile t covers positions [(tile_base + t) * T, + T).
//
// A group is 16 samples.  A lane whose group lies inside its parse range, i + 16 <= e, runs the UNMASKED group: eight pairs of
// samples in eight registers.  The group in which the range ends runs the masked form, a sample per ring access.
//
// Verdict: k_decode_window's.  A lane whose range reaches its waveform's last sample makes the reader's end-of-payload check;
// any other lane asks only that its codes lay inside its payload.  No address depends on the stream: positions come from the
// geometry, the origins and the selection.
template <int T>
__global__ __launch_bounds__(64 * kStackWaves) void k_wave_stack(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                                const uint64_t *__restrict__ wave_off,
                                                                const uint32_t *__restrict__ wave_words, uint64_t n_wf,
                                                                uint64_t tile_base, uint32_t P, const int64_t *__restrict__ start,
                                                                uint64_t start_stride, int64_t offset, uint32_t width,
                                                                const unsigned long long *__restrict__ list, DevStatus *st,
                                                                int64_t *__restrict__ out, uint64_t out_stride) {
    constexpr int GS = kGS;
    __shared__ unsigned long long acc_sq[T];
    __shared__ int32_t acc_sum[T];
    __shared__ uint32_t ring_wg[kStackWaves][kInRingWords];
    __shared__ __attribute__((aligned(16))) uint32_t stage_wg[kStackWaves][kStackStageWords];
    const int lane = lane_id();
    const int wv = wave_id();
    const uint32_t k = G.k;
    const uint32_t tile = blockIdx.x / P, b = blockIdx.x - tile * P;
    const uint64_t t0 = (tile_base + tile) * (uint64_t)T, t1 = t0 + (uint64_t)T;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream.  One read for
    // the workgroup, so that its wavefronts leave together
    if (threadIdx.x == 0) stage_wg[0][0] = st->err;
    for (uint32_t j = threadIdx.x; j < (uint32_t)T; j += 64u * kStackWaves) {
        acc_sum[j] = 0;
        acc_sq[j] = 0;
    }
    __syncthreads();
    const uint32_t seen = stage_wg[0][0];
    __syncthreads();
    if (seen) return;
    uint32_t *const ring = ring_wg[wv] + 64;
    uint32_t *const stage = stage_wg[wv];

    // the positions that received something go to their rows: consecutive lanes, consecutive positions
    auto flush = [&]() {
        for (uint32_t j = threadIdx.x; j < (uint32_t)T; j += 64u * kStackWaves) {
            const uint64_t p = t0 + j;
            if (p >= width) break;
            const unsigned long long q = acc_sq[j];
            if (q) {  // (no square, no sample but zeros)
                int64_t *row = out + p * out_stride;
                atomicAdd((unsigned long long *)(row + DRX_STACK_SUM), (unsigned long long)(int64_t)acc_sum[j]);
                atomicAdd((unsigned long long *)(row + DRX_STACK_SUMSQ), q);
                acc_sum[j] = 0;
                acc_sq[j] = 0;
            }
        }
    };

    // under a selection the lanes take the listed waveforms, 64 to a wavefront: no lane idles beside a waveform nobody selected
    const uint64_t n_listed = list ? list[0] : 0u;
    if (list) n_wf = (n_listed + 63u) / 64u;
    uint32_t rounds = 0;
    for (uint64_t wf0 = (uint64_t)b * kStackWaves; wf0 < n_wf; wf0 += (uint64_t)P * kStackWaves) {  // (uniform in the workgroup)
        const uint64_t wf = wf0 + (uint32_t)wv;
        LaneWave lw = {};
        bool have = wf < n_wf;
        if (have && list) {
            const uint64_t at = wf * 64u + (uint32_t)lane;
            lw.active = at < n_listed;
            if (lw.active) {
                lw.g = list[1u + at];
                lw.len = locate(G, lw.g).len;
            }
        } else if (have) {
            have = lane_wave(G, wf, lane, lw);
        }
        // the lane parses samples [0, e) and adds [s, e): its window's part inside this tile.  Sample idx is position idx + jb
        // of the tile (mod 2^32)
        uint32_t s = 0, e = 0, jb = 0;
        if (have && lw.active) {
            const Win w = stack_window(start, start_stride, offset, width, nullptr, lw.g, lw.len);  // (a selection comes as the list)
            const uint64_t p_lo = w.pf, p_hi = (uint64_t)w.pf + (w.e - w.s);
            const uint64_t lo = p_lo > t0 ? p_lo : t0, hi = p_hi < t1 ? p_hi : t1;
            if (lo < hi) {
                s = w.s + (uint32_t)(lo - p_lo);
                e = w.s + (uint32_t)(hi - p_lo);
                jb = (uint32_t)(lo - t0) - s;
            }
        }
        const uint64_t live = __ballot(e != 0u);
        if (live) {  // (a wavefront whose lanes all lie outside the tile, or have no window, reads nothing)
            const uint32_t len = lw.len;
            const uint64_t g = lw.g;
            uint32_t n = 0;
            uint64_t S = 1;
            if (e) {
                S = wave_off[g] + 1u;
                n = wave_words[g];
            }
            // the form: equal where every lane that parses maps sample index to position alike
            const uint32_t jb0 = (uint32_t)__shfl((int)jb, __ffsll((unsigned long long)live) - 1);
            const bool equal = __all(e == 0u || jb == jb0);
#define DRX_LANE_EARLY
#include "drx_lane_reader.inc"
#undef DRX_LANE_EARLY

            const uint32_t steps = wave_max_u32(e);
            int32_t acc = 0;    // running sum of the deltas: the sample in its low 16 bits
            bool over = false;  // the position passed the words the lane fetched
            set_limits();
            for (; i < steps; i += (uint32_t)GS) {
                group_refill();
                // Who adds something from this group is the geometry's answer.  The lanes leave their eight packed pairs (zero
                // outside the window) in the wavefront's transposition buffer, a column each: in the equal form every lane its
                // own, in the distinct form only the lanes that add something, compacted by rank and rotated by eight per
                // pair (the loads then meet two lanes per bank, not eight)
                const bool mine = i + (uint32_t)GS > s && i < e;
                const uint64_t act = __ballot(mine);
                const bool take = act != 0;  // (uniform)
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
                const uint32_t col = equal ? (uint32_t)lane : rank, rot = equal ? 0u : 8u;
                if (i + (uint32_t)GS <= e) {
                    // ---- the unmasked group: eight pairs, two samples per ring access
                    LANE_GROUP_PAIRS(acc, pr, 0u)
                    if (equal ? take : mine) {
#pragma unroll
                        for (int j = 0; j < GS / 2; ++j) {
                            const uint32_t m = (i + 2u * (uint32_t)j >= s ? 0xffffu : 0u) | (i + 2u * (uint32_t)j + 1u >= s ? 0xffff0000u : 0u);
                            stage[j * 64 + ((col + rot * (uint32_t)j) & 63u)] = pr[j] & m;
                        }
                    }
                } else if (i < e) {
                    // ---- the masked group: the lane's parse range ends inside it.  One sample per ring access.
#pragma unroll 1
                    for (uint32_t j = 0; j < (uint32_t)GS / 2u; ++j) {
                        const uint32_t idx = i + 2u * j;
                        uint32_t pk = 0;
                        if (idx < e) {
                            LANE_ONE(z)
                            acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                            if (idx >= s) pk = (uint32_t)acc & 0xffffu;
                        }
                        if (idx + 1u < e) {
                            LANE_ONE(z)
                            acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                            if (idx + 1u >= s) pk |= (uint32_t)acc << 16;
                        }
                        stage[j * 64u + ((col + rot * j) & 63u)] = pk;
                    }
                } else if (equal && take) {
#pragma unroll
                    for (int j = 0; j < GS / 2; ++j) stage[j * 64 + lane] = 0u;
                }
                if (take) {
                    wave_sync();
                    if (equal) {
                        // ---- across the lanes: lane (pair p, slice q) takes pair p of lanes 8 q .. 8 q + 7
                        const uint32_t *src = stage + (lane & 7) * 64 + (lane >> 3) * 8;
                        uint32_t v[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) v[t] = src[t];
                        int32_t s_ev = 0, s_od = 0;
                        unsigned long long q_ev = 0, q_od = 0;
#pragma unroll
                        for (int t = 0; t < 8; t += 2) {
                            const s16x2 a = as_pair(v[t]), c = as_pair(v[t + 1]);
                            const s16x2 a_ev = as_pair(v[t] & 0xffffu), c_ev = as_pair(v[t + 1] & 0xffffu);
                            const s16x2 a_od = as_pair(v[t] & 0xffff0000u), c_od = as_pair(v[t + 1] & 0xffff0000u);
                            s_ev = __builtin_amdgcn_sdot2(c, (s16x2){1, 0}, __builtin_amdgcn_sdot2(a, (s16x2){1, 0}, s_ev, false), false);
                            s_od = __builtin_amdgcn_sdot2(c, (s16x2){0, 1}, __builtin_amdgcn_sdot2(a, (s16x2){0, 1}, s_od, false), false);
                            // two squares of at most 2^30: 32 bits hold them
                            q_ev += (uint32_t)__builtin_amdgcn_sdot2(c_ev, c_ev, __builtin_amdgcn_sdot2(a_ev, a_ev, 0, false), false);
                            q_od += (uint32_t)__builtin_amdgcn_sdot2(c_od, c_od, __builtin_amdgcn_sdot2(a_od, a_od, 0, false), false);
                        }
                        const uint32_t p0 = i + 2u * (uint32_t)(lane & 7) + jb0;  // the even sample's position (mod 2^32)
                        if (q_ev && p0 < (uint32_t)T) {
                            atomicAdd(&acc_sum[p0], s_ev);
                            atomicAdd(&acc_sq[p0], q_ev);
                        }
                        if (q_od && p0 + 1u < (uint32_t)T) {
                            atomicAdd(&acc_sum[p0 + 1u], s_od);
                            atomicAdd(&acc_sq[p0 + 1u], q_od);
                        }
                    } else {
                        // ---- a work list of (column, pair): eight columns a step, all 64 lanes busy whatever the number of
                        // lanes inside their windows.  Every lane's position of sample i goes to the lane of its rank by one
                        // permutation (the lanes that add nothing behind those that do)
                        const uint32_t n_act = (uint32_t)__popcll((unsigned long long)act);
                        const uint32_t to = mine ? rank : n_act + ((uint32_t)lane - rank);
                        const uint32_t base_of = (uint32_t)__builtin_amdgcn_ds_permute((int)(to << 2), (int)(i + jb));
                        const uint32_t j = (uint32_t)lane >> 3;
                        for (uint32_t k0 = 0; k0 < n_act; k0 += 8u) {
                            const uint32_t kk = k0 + ((uint32_t)lane & 7u);
                            const uint32_t p0 = (uint32_t)__shfl((int)base_of, (int)kk) + 2u * j;  // the even sample's position (mod 2^32)
                            const uint32_t v = stage[j * 64u + ((kk + 8u * j) & 63u)];
                            const int32_t y_ev = (int32_t)(int16_t)(uint16_t)v, y_od = (int32_t)v >> 16;
                            if (kk < n_act) {
                                if (y_ev && p0 < (uint32_t)T) {
                                    atomicAdd(&acc_sum[p0], y_ev);
                                    atomicAdd(&acc_sq[p0], (unsigned long long)(uint32_t)(y_ev * y_ev));
                                }
                                if (y_od && p0 + 1u < (uint32_t)T) {
                                    atomicAdd(&acc_sum[p0 + 1u], y_od);
                                    atomicAdd(&acc_sq[p0 + 1u], (unsigned long long)(uint32_t)(y_od * y_od));
                                }
                            }
                        }
                    }
                    wave_sync();  // (the next group's stores come behind these loads)
                }
                over |= ((flw - ((~Q) >> 5)) & kWMask) > (uint32_t)kRW;
                round_end(i);
            }
            if (e) {
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
        }
        if (++rounds == kStackFlushEvery) {
            __syncthreads();
            flush();
            __syncthreads();
            rounds = 0;
        }
    }
    __syncthreads();
    flush();
}

// General prediction filters: serial_frame() (drx_lane_stream.h); every sample of a window goes to its row by two 64-bit atomics
__global__ __launch_bounds__(64) void k_wave_stack_serial(Geom G, const uint32_t *__restrict__ in, const uint64_t *__restrict__ wave_off,
                                                          const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                          const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset,
                                                          uint32_t width, const uint8_t *__restrict__ select, DevStatus *st,
                                                          int64_t *__restrict__ out, uint64_t out_stride) {
    Win w = {0u, 0u, width};
    serial_frame(
        G, in, wave_off, wave_words, wf_base, (const uint32_t *)nullptr, 0u, st,
        [&](uint64_t g, const WaveRef &r) __attribute__((always_inline)) {
            w = stack_window(start, start_stride, offset, width, select, g, r.len);
            return w.e;
        },
        [&](uint32_t i, int16_t y16) __attribute__((always_inline)) {
            if (i < w.s) return;
            int64_t *row = out + (uint64_t)(w.pf + (i - w.s)) * out_stride;
            const int32_t y = y16;
            atomicAdd((unsigned long long *)(row + DRX_STACK_SUM), (unsigned long long)(int64_t)y);
            atomicAdd((unsigned long long *)(row + DRX_STACK_SUMSQ), (unsigned long long)(uint32_t)(y * y));
        },
        [&](uint64_t, const WaveRef &) __attribute__((always_inline)) {});
}

template <int T>
static void launch_stack_tiles(const StreamCall &c, uint64_t n_wf, unsigned per_cu, const int64_t *d_start, uint64_t start_stride,
                               int64_t offset, uint32_t width, const unsigned long long *d_list, uint32_t max_wgs, int64_t *d_out,
                               uint64_t out_stride) {
    const Geom &G = *c.G;
    const uint64_t wgs = (n_wf + kStackWaves - 1u) / kStackWaves, resident = 256u * per_cu;
    uint32_t P = (uint32_t)(wgs < resident ? wgs : resident);
    if (max_wgs && P > max_wgs) P = max_wgs;  // (the context option "stack_workgroups": fewer workgroups, more rounds each)
    const uint64_t tiles = ((uint64_t)width + (uint64_t)T - 1u) / (uint64_t)T;
    const uint64_t per_launch = (1ull << 23) / P;  // (a launch carries fewer than 2^32 threads)
    for (uint64_t tb = 0; tb < tiles; tb += per_launch) {
        const uint64_t nt = tiles - tb < per_launch ? tiles - tb : per_launch;
        k_wave_stack<T><<<(unsigned)(nt * P), 64 * kStackWaves, 0, c.s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, n_wf, tb, P, d_start,
                                                                        start_stride, offset, width, d_list, c.d_status, d_out, out_stride);
    }
}

hipError_t launch_wave_stack(const StreamCall &c, void *d_list_, uint32_t max_wgs, const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width,
                             const uint8_t *d_select, int64_t *d_out, uint64_t out_stride) {
    // (the list serves the delta filter's kernel under a selection)
    unsigned long long *d_list = (d_select && c.G->n_taps == 0) ? (unsigned long long *)d_list_ : nullptr;
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    // ---- the walk (drx_walk.hip): launch_batch_walk()
    const hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    // ---- the rows, and COUNT from the geometry alone
    k_stack_rows_zero<<<blocks_for(width, 256), 256, 0, s>>>(width, d_out, out_stride);
    if (G.total_waves) {
        if (d_list) {
            const hipError_t em = hipMemsetAsync(d_list, 0, sizeof(unsigned long long), s);
            if (em != hipSuccess) return em;
        }
        for_wavefront_slices(G, false, [&](uint64_t base, unsigned nb) {
            k_stack_count<<<nb, 64, 0, s>>>(G, base, d_start, start_stride, offset, width, d_select, d_list, d_out, out_stride);
        });
        k_stack_count_scan<<<1, 1024, 0, s>>>(width, d_out, out_stride);
        // ---- the sums: persistent workgroups over tiles of positions, or a lane per waveform
        if (G.n_taps != 0) {
            for_wavefront_slices(G, false, [&](uint64_t base, unsigned nb) {
                k_wave_stack_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, d_start, start_stride, offset, width, d_select,
                                                      c.d_status, d_out, out_stride);
            });
        } else {
            const uint64_t n_wf = (!G.uniform && G.rag_order) ? (uint64_t)G.rag_groups : (G.total_waves + 63u) / 64u;
            if (width <= (uint32_t)kStackTileNarrow)
                launch_stack_tiles<kStackTileNarrow>(c, n_wf, 2u, d_start, start_stride, offset, width, d_list, max_wgs, d_out, out_stride);
            else
                launch_stack_tiles<kStackTileWide>(c, n_wf, 1u, d_start, start_stride, offset, width, d_list, max_wgs, d_out, out_stride);
        }
    }
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
