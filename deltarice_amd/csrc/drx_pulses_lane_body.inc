// drx_pulses_lane_body.inc -- the body of the delta filter's lane-per-waveform pulse kernel, included INSIDE the definitions of
// k_find_pulses and k_find_pulses_list (drx_pulses.hip) behind their arguments: text, not a function, so that k_find_pulses keeps
// the instructions it had (as drx_lane_reader.inc and drx_blocks_body.inc do for their kernels).  The including kernel provides
// LIST, and `list` / `n_list` (nullptr where LIST is false).
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
    uint32_t *const ring = ring_all + 64;
#include "drx_lane_reader.inc"

    const uint32_t steps = wave_max_u32(len);
    int32_t acc = 0;  // running sum of the deltas: the sample in its low 16 bits
    set_limits();
    for (uint32_t i = 0; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (i + (uint32_t)GS <= len) {
            // ---- the unmasked group: eight pairs, two samples per ring access
            LANE_GROUP_PAIRS(acc, pr, pm)  // the group's v, two to a register (the earlier one in the low half)
            s16x2 gm = as_pair(pr[0]);
#pragma unroll
            for (int j = 1; j < GS / 2; ++j) gm = __builtin_elementwise_max(gm, as_pair(pr[j]));
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
                    LANE_ONE(z)
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    P.step((int32_t)(int16_t)(uint16_t)((uint32_t)acc ^ pm), idx);
                }
            }
        }
        round_end(i);
    }
    if (!active) return;
    if (P.open) P.close(len);  // a run still open at the last sample ends there
    if (len && LANE_MISSES_LAST_WORD()) atomicOr(&st->err, kErrCorrupt);
    count_out[g] = P.count;
