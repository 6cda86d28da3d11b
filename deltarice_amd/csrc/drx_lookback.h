// drx_lookback.h -- the decoupled look-back of the kernels that scan across workgroups (not installed): k_encode_fused,
// k_encode_pieces, the block-form body (drx_blocks_body.inc) and k_iir_tiles.  DESIGN.md, "The decoupled look-back".
//
// One 64-bit entry per workgroup, block, tile or waveform, zeroed by the launcher.  The owner of an entry first publishes
// kScanAgg | its own value, later kScanPrefix | the fold of everything from the site's first entry up to its own; a zero
// entry is not there yet (the word is its own flag: 2 status bits on top of the value).  Between the two stores ONE
// wavefront of the owner walks its predecessors, nearest first, folding aggregates until it meets a prefix.  Indices are
// drawn from a ticket counter, so every lower entry belongs to a running (or finished) workgroup: with zeroed state the
// walk always ends.  The site says what a value is and how a window of them folds; everything else is here, once.
#ifndef DRX_LOOKBACK_H
#define DRX_LOOKBACK_H

#include "drx_device.h"

namespace drx {

constexpr uint64_t kScanAgg = 1ull << 62, kScanPrefix = 2ull << 62, kScanValMask = (1ull << 62) - 1ull;

// Entries per poll: two per lane.  The frontier of known prefixes advances one window per hop (a hop = an agent-scope store
// becoming visible + an agent-scope load, 3-5 us under the encoder's own streaming loads: a predecessor's prefix is published
// one round trip after its aggregate), so the window bounds the rate of a whole kernel: 128 entries carried ~25 workgroups
// per microsecond, just what k_encode_fused's 1M waveforms in 6 ms need (round 3: without the look-back the kernel took 4.5 ms
// instead of 6.0; one entry per waveform and 64 per poll capped it at ~64 waveforms per round trip, ~9 ms).
constexpr int kLookbackWin = 128;
constexpr uint32_t kLookbackSpins = 1u << 22;  // polls of one walk before it gives up with kErrInternal
static_assert(kIirWin == (uint32_t)kLookbackWin, "drx_iir.hip's P^j table and its per-window factor P^kIirWin are one window of this walk");

// The window rule.  p[j] / z[j]: the ballots "status == 2" (prefix) / "status == 0" (not there yet) of the entries at
// distance 64 j + lane from the nearest one (distance 0).  fp: distance of the nearest prefix, kLookbackWin = none in this
// window.  hole: an entry nearer than fp is not there yet -- the window cannot be folded.  An entry counts when its distance
// is <= fp (lookback_counts): the aggregates in front of the prefix and the prefix itself.
struct LookbackWindow {
    int fp;
    bool hole;
};
__host__ __device__ __forceinline__ LookbackWindow lookback_window(uint64_t p0, uint64_t z0, uint64_t p1, uint64_t z1) {
    const int fp = p0 ? __builtin_ctzll(p0) : (p1 ? 64 + __builtin_ctzll(p1) : kLookbackWin);
    const uint64_t near0 = fp >= 64 ? ~0ull : ((1ull << fp) - 1ull);
    const uint64_t near1 = fp >= 128 ? ~0ull : (fp > 64 ? ((1ull << (fp - 64)) - 1ull) : 0ull);
    return LookbackWindow{fp, ((z0 & near0) | (z1 & near1)) != 0ull};
}
__host__ __device__ __forceinline__ bool lookback_counts(int fp, int j, int lane) { return 64 * j + lane <= fp; }

__device__ __forceinline__ void scan_publish(uint64_t *state, int64_t idx, uint64_t tagged, int lane) {
    if (lane == 0) __hip_atomic_store(state + idx, tagged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The walk of entries [first, idx), by one wavefront.  fold(s0, s1, in0, in1) is called once per completed window, nearest
// window first: the lane's two raw entries (status bits included), at distances lane and 64 + lane from the window's nearest
// entry, and whether each counts.  An entry in front of `first` reads as an empty prefix and ends the walk (idx == first: no
// load at all, one fold of that empty prefix).
template <int GATE_SLEEP, class Fold>
__device__ __forceinline__ void lookback_walk(const uint64_t *state, int64_t idx, int64_t first, int lane, DevStatus *st, Fold &&fold) {
    int64_t base = idx - 1;
    uint32_t spins = 0;
    // Wait for the NEAREST predecessor alone first: one 8-byte load per poll instead of a whole window from every waiting
    // workgroup.  Workgroups finish roughly in ticket order, so when idx - 1 has published, the window behind it has too;
    // and ~500 workgroups polling 128 entries each were a fabric load of their own beside the encoder's streaming reads
    // (agent-scope loads are served by the memory side, not by L2; k_encode_fused: 5.86 -> 5.43 ms, profiles/r03_notes.md).
    // At the spin bound the gate leaves silently: the window loop below finds the same hole and is the one place that reports.
    while (base >= first) {
        uint64_t v = 0;
        if (lane == 0) v = __hip_atomic_load(state + base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 62)) != 0) break;
        __builtin_amdgcn_s_sleep(GATE_SLEEP);
        if (++spins > kLookbackSpins) break;
    }
    for (;;) {
        const int64_t i0 = base - lane, i1 = base - 64 - lane;
        uint64_t s0v = kScanPrefix, s1v = kScanPrefix;  // in front of `first`: an empty prefix
        if (i0 >= first) s0v = __hip_atomic_load(state + i0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (i1 >= first) s1v = __hip_atomic_load(state + i1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t st0 = (uint32_t)(s0v >> 62), st1 = (uint32_t)(s1v >> 62);
        const LookbackWindow w = lookback_window(__ballot(st0 == 2u), __ballot(st0 == 0u), __ballot(st1 == 2u), __ballot(st1 == 0u));
        if (w.hole) {  // a nearer predecessor has not published yet
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kLookbackSpins) {  // cannot happen with zeroed state (ticket holders' predecessors run); never hang the GPU
                if (lane == 0) atomicOr(&st->err, kErrInternal);
                break;
            }
            continue;
        }
        fold(s0v, s1v, lookback_counts(w.fp, 0, lane), lookback_counts(w.fp, 1, lane));
        if (w.fp < kLookbackWin) break;
        base -= kLookbackWin;
    }
}

// What the owner of entry idx does: the site's first entry publishes its prefix (its own value) at once; any other
// publishes its aggregate, walks, then publishes prefix(), the site's fold of what the walk found and its own value.
template <int GATE_SLEEP, class Fold, class Prefix>
__device__ __forceinline__ void lookback_scan(uint64_t *state, int64_t idx, int64_t first, uint64_t mine, int lane, DevStatus *st,
                                              Fold &&fold, Prefix &&prefix) {
    if (idx == first) {
        scan_publish(state, idx, kScanPrefix | mine, lane);
    } else {
        scan_publish(state, idx, kScanAgg | mine, lane);
        lookback_walk<GATE_SLEEP>(state, idx, first, lane, st, fold);
        scan_publish(state, idx, kScanPrefix | prefix(), lane);
    }
}

// The plain fold: values are counts (62 bits), a window folds to their sum.  lookback_sum: the sum over [first, idx);
// lookback_scan_sum: the same as the owner of entry idx with the value `mine`.
struct LookbackSum {
    uint64_t sum = 0;
    __device__ __forceinline__ void operator()(uint64_t s0, uint64_t s1, bool in0, bool in1) {
        sum += wave_sum_u64((in0 ? (s0 & kScanValMask) : 0ull) + (in1 ? (s1 & kScanValMask) : 0ull));
    }
};
template <int GATE_SLEEP>
__device__ __forceinline__ uint64_t lookback_sum(const uint64_t *state, int64_t idx, int64_t first, int lane, DevStatus *st) {
    LookbackSum f;
    lookback_walk<GATE_SLEEP>(state, idx, first, lane, st, f);
    return f.sum;
}
template <int GATE_SLEEP>
__device__ __forceinline__ uint64_t lookback_scan_sum(uint64_t *state, int64_t idx, int64_t first, uint64_t mine, int lane, DevStatus *st) {
    LookbackSum f;
    lookback_scan<GATE_SLEEP>(state, idx, first, mine, lane, st, f, [&] { return f.sum + mine; });
    return f.sum;
}

}  // namespace drx
#endif
