// drx_pulse_runs.h -- runs of over-threshold samples, summarised per stretch of a waveform so that stretches can be worked on
// apart and put together afterwards (not installed).  Plain C++: a host compiler takes this file without HIP
// (tests/pulse_runs_host.cpp), and the same text serves three levels -- the lanes of a block and the blocks of a waveform in
// drx_pulses_blocks.hip, and that host test.
//
// Polarity is drx_pulses.hip's: a sample y enters as v = y ^ flip (flip = 0 / -1), it is over when v > tv, tv the waveform's
// clamped threshold (pulse_threshold()).  A run's sum is the sum of its v, its peak a KEY that orders by v and then by the
// earliest index, (v << 32) | (0x7fffffff - index) under max, as k_stats_blocks' maximum does; pulse_record() turns both back.
//
// PulseSeg summarises a stretch of n consecutive samples:
//   lead_*   the run that touches the stretch's first sample: width, peak key, sum (lead_w = 0: the first sample is not over)
//   trail_*  the run that touches its last sample: start (an index in the waveform), width, peak key, sum (trail_w = 0: none)
//   inner    the pulses -- runs of at least min_width -- that lie wholly inside, both ends closed inside the stretch
// Every sample is over exactly when lead_w == n (pulse_seg_all_over()); the one run is then both the leading and the trailing
// one.  A run that is absent has width 0, start 0, key kPulseNoKey and sum 0, so that joins need no case for it, and the
// empty stretch (all of that, n = 0) is pulse_combine()'s identity on both sides.
#ifndef DRX_PULSE_RUNS_H
#define DRX_PULSE_RUNS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DRX_PULSE_HD __host__ __device__ __forceinline__
#else
#define DRX_PULSE_HD inline
#endif

namespace drx {

constexpr int64_t kPulseNoKey = INT64_MIN;
constexpr int kPulseRecCols = 5;  // start, width, peak, where the peak sits, integral: DRX_PULSE_* of include/deltarice_hip.h

// The threshold a waveform's samples are compared with, as drx_find_pulses defines it: tab_v + thr saturating at the int64
// ends (has_tab false: thr alone), clamped so that it compares as an int32 with any int16 -- positive polarity to
// [-32769, 32767] (at the top nothing is over, at the bottom everything), negative polarity to [-32768, 32768] and then
// tv = -1 - t, the same range.
DRX_PULSE_HD int32_t pulse_threshold(bool has_tab, int64_t tab_v, int64_t thr, bool neg) {
    int64_t t = thr;
    if (has_tab && __builtin_add_overflow(tab_v, thr, &t)) t = tab_v < 0 ? INT64_MIN : INT64_MAX;
    if (neg) {
        t = t < -32768 ? -32768 : (t > 32768 ? 32768 : t);
        return (int32_t)(-1 - t);
    }
    return (int32_t)(t < -32769 ? -32769 : (t > 32767 ? 32767 : t));
}

DRX_PULSE_HD int64_t pulse_key(int32_t v, uint32_t idx) { return (int64_t)(((uint64_t)(uint32_t)v << 32) | (uint64_t)(0x7fffffffu - idx)); }
DRX_PULSE_HD int32_t pulse_key_value(int64_t key) { return (int32_t)(uint32_t)((uint64_t)key >> 32); }
DRX_PULSE_HD uint32_t pulse_key_index(int64_t key) { return 0x7fffffffu - (uint32_t)(uint64_t)key; }

// a run as drx_find_pulses reports it: y = v ^ flip, and for negative polarity y = -1 - v summed over w samples
DRX_PULSE_HD void pulse_record(int64_t *rec, uint32_t s, uint32_t w, int64_t key, int64_t sum, bool neg) {
    rec[0] = (int64_t)s;
    rec[1] = (int64_t)w;
    rec[2] = (int64_t)pulse_key_value(key) ^ (neg ? (int64_t)-1 : (int64_t)0);
    rec[3] = (int64_t)pulse_key_index(key);
    rec[4] = neg ? -sum - (int64_t)w : sum;
}

struct PulseSeg {
    uint32_t n, inner;
    uint32_t lead_w, trail_w, trail_s;
    int64_t lead_key, lead_sum, trail_key, trail_sum;
};
DRX_PULSE_HD PulseSeg pulse_seg_empty() { return PulseSeg{0u, 0u, 0u, 0u, 0u, kPulseNoKey, 0, kPulseNoKey, 0}; }
DRX_PULSE_HD bool pulse_seg_all_over(const PulseSeg &S) { return S.n != 0u && S.lead_w == S.n; }

// a summary as kPulseSegWords uint64: what a block publishes per block slot (drx_pulses_blocks.hip) and what the wavefronts of
// a block exchange through LDS
constexpr int kPulseSegWords = 7;
DRX_PULSE_HD void pulse_seg_pack(const PulseSeg &S, uint64_t *w) {
    w[0] = (uint64_t)S.n | ((uint64_t)S.inner << 32);
    w[1] = (uint64_t)S.lead_w | ((uint64_t)S.trail_w << 32);
    w[2] = (uint64_t)S.trail_s;
    w[3] = (uint64_t)S.lead_key;
    w[4] = (uint64_t)S.lead_sum;
    w[5] = (uint64_t)S.trail_key;
    w[6] = (uint64_t)S.trail_sum;
}
DRX_PULSE_HD PulseSeg pulse_seg_unpack(const uint64_t *w) {
    return PulseSeg{(uint32_t)w[0], (uint32_t)(w[0] >> 32), (uint32_t)w[1], (uint32_t)(w[1] >> 32), (uint32_t)w[2],
                    (int64_t)w[3], (int64_t)w[4], (int64_t)w[5], (int64_t)w[6]};
}

// ---- a stretch from its samples: pulse_seg_step() for each in order (idx: its index in the waveform), then pulse_seg_finish()
DRX_PULSE_HD void pulse_seg_close(PulseSeg &S, uint32_t min_width) {  // the open run ends in front of sample n of the stretch
    if (S.trail_w == S.n) {  // it began at the stretch's first sample
        S.lead_w = S.trail_w;
        S.lead_key = S.trail_key;
        S.lead_sum = S.trail_sum;
    } else if (S.trail_w >= min_width) {
        ++S.inner;
    }
    S.trail_w = 0u;
    S.trail_s = 0u;
    S.trail_key = kPulseNoKey;
    S.trail_sum = 0;
}
DRX_PULSE_HD void pulse_seg_step(PulseSeg &S, int32_t v, int32_t tv, uint32_t idx, uint32_t min_width) {
    if (v > tv) {
        if (S.trail_w == 0u) S.trail_s = idx;
        const int64_t key = pulse_key(v, idx);
        S.trail_key = key > S.trail_key ? key : S.trail_key;  // (an equal v further on has the smaller key: the first place stays)
        S.trail_sum += (int64_t)v;
        ++S.trail_w;
    } else if (S.trail_w != 0u) {
        pulse_seg_close(S, min_width);
    }
    ++S.n;
}
DRX_PULSE_HD void pulse_seg_finish(PulseSeg &S) {
    if (S.n != 0u && S.trail_w == S.n) {  // every sample is over: the one run leads as well
        S.lead_w = S.trail_w;
        S.lead_key = S.trail_key;
        S.lead_sum = S.trail_sum;
    }
}

// ---- A then B, adjacent stretches of one waveform.  A's trailing run and B's leading run are one run J.  Where A is all over,
// J leads the result; where B is, J trails it; where neither is, J closes inside the result and counts as an inner pulse if it
// is wide enough.  Associative (J of (A B) C and of A (B C) are the same runs), and the empty stretch is the identity.  Written
// component by component: a select between two structs is compiled as a select between their addresses.
DRX_PULSE_HD PulseSeg pulse_combine(const PulseSeg &A, const PulseSeg &B, uint32_t min_width) {
    const bool a_all = A.lead_w == A.n, b_all = B.lead_w == B.n;  // (the empty stretch counts as all over: it cuts no run)
    const uint32_t jw = A.trail_w + B.lead_w;
    const uint32_t js = A.trail_w ? A.trail_s : B.trail_s;  // (used where B is all over: B.trail_s is B's first sample)
    const int64_t jkey = A.trail_key > B.lead_key ? A.trail_key : B.lead_key;
    const int64_t jsum = A.trail_sum + B.lead_sum;
    PulseSeg R;
    R.n = A.n + B.n;
    R.inner = A.inner + B.inner + ((!a_all && !b_all && jw >= min_width) ? 1u : 0u);
    R.lead_w = a_all ? jw : A.lead_w;
    R.lead_key = a_all ? jkey : A.lead_key;
    R.lead_sum = a_all ? jsum : A.lead_sum;
    R.trail_w = b_all ? jw : B.trail_w;
    R.trail_s = b_all ? js : B.trail_s;
    R.trail_key = b_all ? jkey : B.trail_key;
    R.trail_sum = b_all ? jsum : B.trail_sum;
    return R;
}

// ---- the second pass over a stretch that is part of a BLOCK (samples [blk_first, ...) of the waveform): seeded with P, the
// summary of the block's samples in front of the stretch, it hands every pulse that closes inside the stretch to
// store(number, start, width, key, sum), numbered from 0 inside the block in the order of their starts.  The run that touches
// the block's first sample is no pulse of the block (it may go on in the block before): it goes into the block's summary,
// as the run still open at the block's last sample does -- which never closes here.
struct PulseEmit {
    bool open;
    uint32_t s, number;
    int64_t key, sum;
};
DRX_PULSE_HD PulseEmit pulse_emit_seed(const PulseSeg &P) { return PulseEmit{P.trail_w != 0u, P.trail_s, P.inner, P.trail_key, P.trail_sum}; }
template <class Store>
DRX_PULSE_HD void pulse_emit_step(PulseEmit &E, int32_t v, int32_t tv, uint32_t idx, uint32_t blk_first, uint32_t min_width, Store &&store) {
    if (v > tv) {
        if (!E.open) {
            E.open = true;
            E.s = idx;
            E.key = kPulseNoKey;
            E.sum = 0;
        }
        const int64_t key = pulse_key(v, idx);
        E.key = key > E.key ? key : E.key;
        E.sum += (int64_t)v;
    } else if (E.open) {
        if (E.s != blk_first && idx - E.s >= min_width) {
            store(E.number, E.s, idx - E.s, E.key, E.sum);
            ++E.number;
        }
        E.open = false;
    }
}

// ---- A waveform from the summaries of its blocks, in order (seg_of(b), b < n_blocks; together they cover the waveform from
// sample 0 to its last).  A carried open run is joined to the next block's leading run; a run that closes is a pulse if it is at
// least min_width wide; the run still open behind the last block ends with the waveform.  Pulses are numbered by their start:
// number p < max_pulses goes to output slot p, either put together here -- emit(p, start, width, key, sum) -- or one of the
// block's own, which the block staged under its block-relative number r if r < cap -- copy(b, r, p).  *count: all pulses.
// base(b, first): block b's own pulses are numbers first, first + 1, ... of the waveform (told of every block that is not all
// over).  Returns false if a block did not stage a record that is needed (more than cap of its pulses are among the waveform's
// first max_pulses): the count and every slot written are still exact, some slots are missing -- those of block b are slots
// first + r, r >= cap, which a block that is run again knowing `first` can write itself.
template <class SegOf, class Emit, class Copy, class Base>
DRX_PULSE_HD bool pulse_stitch(uint32_t n_blocks, uint32_t min_width, uint32_t max_pulses, uint32_t cap, SegOf &&seg_of, Emit &&emit,
                               Copy &&copy, Base &&base, uint32_t *count) {
    uint32_t cw = 0, cs = 0, pos = 0, cnt = 0;  // the carried run (width, start), samples so far, pulses so far
    int64_t ckey = kPulseNoKey, csum = 0;
    bool complete = true;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const PulseSeg S = seg_of(b);
        const uint32_t jw = cw + S.lead_w, js = cw ? cs : pos;
        const int64_t jkey = ckey > S.lead_key ? ckey : S.lead_key, jsum = csum + S.lead_sum;
        if (S.lead_w == S.n) {  // all over (or empty): the run goes on
            cw = jw; cs = js; ckey = jkey; csum = jsum;
        } else {
            if (jw >= min_width) {
                if (cnt < max_pulses) emit(cnt, js, jw, jkey, jsum);
                ++cnt;
            }
            base(b, cnt);
            const uint32_t room = max_pulses > cnt ? max_pulses - cnt : 0u;
            uint32_t need = S.inner < room ? S.inner : room;
            if (need > cap) { complete = false; need = cap; }
            for (uint32_t r = 0; r < need; ++r) copy(b, r, cnt + r);
            cnt += S.inner;
            cw = S.trail_w; cs = S.trail_s; ckey = S.trail_key; csum = S.trail_sum;
        }
        pos += S.n;
    }
    if (cw != 0u && cw >= min_width) {
        if (cnt < max_pulses) emit(cnt, cs, cw, ckey, csum);
        ++cnt;
    }
    *count = cnt;
    return complete;
}

}  // namespace drx
#endif
