// drx_windows_lane_body.inc -- the body of the delta filter's lane-per-waveform kernel of drx_decode_windows, included INSIDE the
// definitions of k_decode_windows and k_decode_windows_list (drx_windows.hip) behind their arguments: text, not a function, as
// drx_pulses_lane_body.inc is for the pulse kernels.  The including kernel provides LIST, and `list` / `n_list` (nullptr where
// LIST is false).
    constexpr int GS = kGS;
    __shared__ uint32_t ring_all[kInRingWords];
    const int lane = lane_id();
    const uint32_t k = G.k;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
    LANE_WAVE_G_ACTIVE_LEN(G, wf_base + blockIdx.x, lane)
    if constexpr (LIST) {  // lane j of the launch takes waveform list[j], j < *n_list (the mapping above is then not used)
        const uint64_t j_ = wf * 64u + (uint32_t)lane;
        active = j_ < (uint64_t)*n_list;
        g = active ? (uint64_t)list[j_] : 0u;
        len = active ? locate(G, g).len : 0u;
    }
    uint32_t n = 0;
    uint64_t S = 1;
    uint32_t nlive = 0, e = 0;  // the lane parses samples [0, e): e_g, the largest end of its live windows
    bool sorted = true;
    if (active) e = windows_prologue(wl, g, len, nlive, sorted);
    if (e) {
        S = wave_off[g] + 1u;
        n = wave_words[g];
    } else {
        nlive = 0;
    }
    // Window p as the cursor sees it: samples [s_, e_) of the waveform, sample idx at rs_[idx].  The ends are clamped so that both
    // are non-decreasing in the window's start: a window in front of the waveform is [0, 0), one behind it [len, len); a slot
    // behind the last live one is [2^32 - 1, 2^32 - 1), which no group reaches.
    auto span = [&](uint32_t p, uint32_t &s_, uint32_t &e_, int16_t *&rs_) __attribute__((always_inline)) {
        s_ = e_ = 0xffffffffu;
        rs_ = wl.out;
        if (p >= nlive) return;
        const int64_t a = wl.at(g, p);
        const Win w = window_at(a, wl.width, len);
        s_ = w.s;
        e_ = w.e;
        if (a >= (int64_t)len) s_ = e_ = len;
        rs_ = wl.row(g, p) + ((int64_t)w.pf - (int64_t)w.s);
    };
    // the cursor of a sorted list: window `cur` is the first whose end lies behind the samples done, [cs, ce) and its row stay in
    // registers, and so does the start of the window behind it
    uint32_t cur = 0, cs, ce, ns;
    int16_t *crs;
    span(0u, cs, ce, crs);
    auto next_start = [&]() __attribute__((always_inline)) {
        uint32_t t_;
        int16_t *r_;
        span(cur + 1u, ns, t_, r_);
    };
    next_start();
    auto advance = [&](uint32_t done) __attribute__((always_inline)) {  // samples [0, done) are through
        while (cur < nlive && ce <= done) {
            ++cur;
            span(cur, cs, ce, crs);
            next_start();
        }
    };
    if (sorted) advance(0u);
    uint32_t *const ring = ring_all + 64;
#define DRX_LANE_EARLY
#include "drx_lane_reader.inc"
#undef DRX_LANE_EARLY

    const uint32_t steps = wave_max_u32(e);
    int32_t acc = 0;    // running sum of the deltas: the sample in its low 16 bits
    bool over = false;  // the position passed the words the lane fetched
    set_limits();
    for (; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (i + (uint32_t)GS <= e) {
            // ---- the unmasked group: eight pairs, two samples per ring access
            LANE_GROUP_PAIRS(acc, pr, 0u)  // the group's samples, two to a register (the earlier one in the low half)
            // a sorted list: one compare says that the group touches no window.  An unsorted one: every live window, every group.
            if (!sorted || i + (uint32_t)GS > cs) {
                uint32_t q = sorted ? cur : 0u, s_ = cs, e_ = ce;
                int16_t *rs_ = crs;
                if (!sorted) span(0u, s_, e_, rs_);
                for (;;) {
                    if (i >= s_ && i + (uint32_t)GS <= e_ && (((uintptr_t)rs_ >> 1) & 1u) == 0u) {
                        // the group lies inside the window and its first destination is a dword's: eight dword stores
                        uint32_t *d = (uint32_t *)(rs_ + i);
#pragma unroll
                        for (int j = 0; j < GS / 2; ++j) d[j] = pr[j];
                    } else if (i + (uint32_t)GS > s_ && i < e_) {
#pragma unroll
                        for (int u = 0; u < GS; ++u) {
                            const uint32_t v = (u & 1) ? pr[u / 2] >> 16 : pr[u / 2];
                            if (i + (uint32_t)u >= s_ && i + (uint32_t)u < e_) rs_[i + (uint32_t)u] = (int16_t)v;
                        }
                    }
                    if (sorted && q == cur && ns >= i + (uint32_t)GS) break;  // (the common case: no window behind this one begins here)
                    if (++q >= nlive) break;
                    span(q, s_, e_, rs_);
                    if (sorted && s_ >= i + (uint32_t)GS) break;
                }
                if (sorted) advance(i + (uint32_t)GS);
            }
        } else if (i < e) {
            // ---- the masked group: the lane's parse range ends inside it.  One sample per ring access, 2-byte stores, a plain
            // loop over the windows from the cursor on (an unsorted list: all of them).
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)GS; ++u) {
                const uint32_t idx = i + u;
                if (idx < e) {
                    LANE_ONE(z)
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    for (uint32_t q = sorted ? cur : 0u; q < nlive; ++q) {
                        uint32_t s_, e_;
                        int16_t *rs_;
                        span(q, s_, e_, rs_);
                        if (sorted && s_ > idx) break;
                        if (idx >= s_ && idx < e_) rs_[idx] = (int16_t)(uint16_t)acc;
                    }
                }
            }
        }
        over |= ((flw - ((~Q) >> 5)) & kWMask) > (uint32_t)kRW;
        round_end(i);
    }
    if (!e) return;
    // the verdict is k_decode_window's (drx_window.hip), applied at e_g
    const uint32_t used_words = LANE_USED_WORDS();
    bool bad;
    if (e == len) {
        bad = LANE_MISSES_LAST_WORD_AT(used_words);
    } else {
        // the windows' codes lay inside the payload: the exact end position from its distance to flw (at most a ring)
        const uint32_t d = (flw - (s0 + used_words)) & kWMask;
        const int32_t sd = (int32_t)(d << 5) >> 5;
        bad = over || (uint64_t)flw - (uint64_t)(int64_t)sd > (uint64_t)s0 + n;
    }
    if (bad) atomicOr(&st->err, kErrCorrupt);
