// drx_lane_reader.inc -- one lane's reader of its waveform's payload, included in the BODY of the kernels that read an encoded
// batch a lane per waveform (k_wave_stats, k_decode_window, k_find_pulses, parse_lane() of drx_transcode.hip; constants and the
// lane mapping: drx_lane_stream.h).  The stream side is k_decode_lanes' (drx_decode_kernels.hip, DESIGN.md section 4.2): a
// per-lane word-major reversed LDS ring refilled in whole 128-byte lines, each requested once; a 64-bit window gives two codes
// per ring access; escape and ordinary codes share one extraction.  What that decoder needs for its STORES is absent: no
// transposition buffer, no start delay, no edge rounds -- a lane starts at its first sample and stops behind its last.
//
// An included text and not a struct of inlined members: the struct form compiled the three kernels to other schedules, which
// were measured 1-2 % slower (profiles/lane_stream_refactor_ab.txt); this form compiles to the instructions each kernel had
// with a copy of its own (as drx_blocks_body.inc does for the block kernels).
//
// In scope where it is included: ring (the wavefront's ring_all + 64, ring_all[kInRingWords] in LDS), lane, in, in_words, k,
// S (the payload's first word) and n (its words; S = 1, n = 0: a lane without a waveform).  It leaves behind
//   set_limits()                 once, in front of the loop over groups of kGS samples, i = 0, kGS, ...
//   group_refill()               in front of every group
//   LANE_PAIR(z1, z2)            two zig-zag values per ring access (an escape leaves 8 << 16 above its bit 15) ...
//   LANE_GROUP_PAIRS(acc, pr, f) ... eight of those: an unmasked group's samples, packed into pr[kGS / 2] ...
//   LANE_ONE(z)                  ... or the masked form's one
//   round_end(i)                 behind every group
//   LANE_MISSES_LAST_WORD()      the verdict of a lane that parsed its whole waveform
// DRX_LANE_EARLY defined (k_decode_window): the lane parses samples [0, e) and no further, e in scope as well; the loop variable
// is the i declared here.  The lane asks for no more words than e codes of 25 bits take and requests no piece once it is
// through.  (The verdict of a lane that stops in front of its waveform's end is that kernel's own.)

const uint64_t A = (S & ~(uint64_t)(kRW - 1)) - (uint64_t)kRW;  // s0 in [kRW, 2 kRW)
const uint32_t s0 = (uint32_t)(S - A);
#ifdef DRX_LANE_EARLY
// the words the lane may ask for: its payload's, and no more than e codes of 25 bits take; none where it parses nothing
const uint32_t n_max = max_payload_words(e);
const uint32_t endw = e ? s0 + (n < n_max ? n : n_max) : 0u;
#else
const uint32_t endw = s0 + n;
#endif
uint32_t flw = s0 & ~(uint32_t)(kLW - 1);
const bool in_vec_ok = ((uintptr_t)in & 15u) == 0;
uint32_t *myring = ring + lane;
#ifdef DRX_LANE_EARLY
uint32_t i = 0;  // first sample of the current group
#endif

// a piece lies inside [0, in_words) or is read word by word, zero beyond: no load leaves the caller's stream
auto load_piece = [&](uint4 (&v)[kNV]) {
    const uint64_t a = A + flw;
    if (in_vec_ok && a + (uint32_t)kLW <= in_words) {
#pragma unroll
        for (int j = 0; j < kNV; ++j) v[j] = *reinterpret_cast<const uint4 *>(in + a + 4 * j);
    } else {
#pragma unroll
        for (int j = 0; j < kNV; ++j) {
            v[j].x = (a + 4 * j + 0 < in_words) ? in[a + 4 * j + 0] : 0u;
            v[j].y = (a + 4 * j + 1 < in_words) ? in[a + 4 * j + 1] : 0u;
            v[j].z = (a + 4 * j + 2 < in_words) ? in[a + 4 * j + 2] : 0u;
            v[j].w = (a + 4 * j + 3 < in_words) ? in[a + 4 * j + 3] : 0u;
        }
    }
};
auto store_piece = [&](const uint4 (&v)[kNV]) {
    const uint32_t r0 = (uint32_t)kRW - (flw & (uint32_t)(kRW - 1));
    uint32_t *dst = myring + r0 * 64u;
#pragma unroll
    for (int j = 0; j < kNV; ++j) {
        dst[-(4 * j + 0) * 64] = v[j].x; dst[-(4 * j + 1) * 64] = v[j].y;
        dst[-(4 * j + 2) * 64] = v[j].z; dst[-(4 * j + 3) * 64] = v[j].w;
    }
    if (r0 == (uint32_t)kRW) {
        myring[0] = v[0].x;
        myring[-64] = v[0].y;
    }
    flw += (uint32_t)kLW;
};

uint32_t Q = 0u - 32u * s0;  // minus the bit position (relative to A)
// Q_need: position (in Q units, Q decreases) at which this lane must have its next piece; 0x7fffffff away from Q means
// "never" (stream exhausted, or an early-ending lane is through).  cw = (~Q) >> 5, so cw >= c  <=>  Q <= ~(32 c)
uint32_t Q_need;
#ifdef DRX_LANE_EARLY
auto more = [&]() __attribute__((always_inline)) { return flw < endw && i < e; };  // words to come, and a use for them
#else
auto more = [&]() __attribute__((always_inline)) { return flw < endw; };  // words to come
#endif
auto set_limits = [&]() __attribute__((always_inline)) {
    Q_need = more() ? ~(32u * (flw - kNeedAt + 1u)) : Q - 0x7fffffffu;
};
auto sync_refill = [&]() __attribute__((always_inline)) {  // serve every lane that is (nearly) dry, waiting for the data
    for (;;) {
        const uint32_t avail = (flw - ((~Q) >> 5)) & kWMask;
        const bool m = more();
        if (!__any(m && avail < kNeedAt)) break;
        if (m && avail <= (uint32_t)(kRW - kLW)) {
            uint4 v[kNV];
            load_piece(v);
            store_piece(v);
        }
        wave_sync();
    }
};

{   // start-up: the piece that holds word s0 and as many more as fit
    uint4 v[kNV];
    for (int j = 0; j < kRW / kLW; ++j) {
        if (__ballot(flw < endw && flw + (uint32_t)kLW <= s0 + (uint32_t)kRW) == 0) break;
        if (flw < endw && flw + (uint32_t)kLW <= s0 + (uint32_t)kRW) {
            load_piece(v);
            store_piece(v);
        }
    }
    wave_sync();
}

// ONE piece per lane is in flight, as in k_decode_lanes: requested at a round's end as soon as the lane holds none, committed
// at the first round end (or refill test) at which it fits, avail <= kRW - kLW; until then it stays in its registers.  Every
// line of a stream is requested once, by one lane, by the kNV loads of one round.  A piece still in flight when its lane
// is through is dropped: it lay inside the lane's own stream.
uint4 pv[kNV];
bool pneed = false;
auto commit_if_fits = [&]() __attribute__((always_inline)) {  // the rows a piece overwrites must have been consumed
    const uint32_t avail = (flw - ((~Q) >> 5)) & kWMask;
    if (pneed && avail <= (uint32_t)(kRW - kLW)) {
        store_piece(pv);
        pneed = false;
    }
};
auto group_refill = [&]() __attribute__((always_inline)) {
    if (__any((int32_t)(Q - Q_need) <= 0)) {  // one signed compare per test (positions are mod 2^32)
        commit_if_fits();  // (a lane short of words has room for its piece: kNeedAt <= kRW - kLW)
        wave_sync();
        sync_refill();  // loads only where a lane is still short: it held no piece, or eats more than one per round
        set_limits();
    }
};

// behind group i: at a round's end the piece in flight is committed where it fits and the next one requested
auto round_end = [&](uint32_t at) __attribute__((always_inline)) {
    if ((at & (uint32_t)(kT - 1)) == (uint32_t)(kT - kGS)) {
        wave_sync();
        commit_if_fits();
        wave_sync();
        set_limits();
        if (!pneed) {
#ifdef DRX_LANE_EARLY
            pneed = flw < endw && at + (uint32_t)kGS < e;  // no lane requests a piece once it is through
#else
            pneed = flw < endw;
#endif
            if (pneed) load_piece(pv);
        }
    }
};
// Two codes per ring access: a 64-bit window (three words) always holds two codes (2 x 25 bits), so the second code's window
// is one v_alignbit away from the first one's length.  v_bfe_u32 and v_alignbit_b32 read 5 bits of their offset / shift:
// ~t == 31 - t (mod 32) serves both.
#define LANE_PAIR(z1, z2)                                                                  \
    uint32_t z1, z2;                                                                       \
    {                                                                                      \
        const uint32_t row_ = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)kLogRW);              \
        const uint32_t *wp_ = myring + row_ * 64u;                                         \
        const uint32_t lo_ = wp_[0], hi_ = wp_[64], lo2_ = wp_[-64];                       \
        const uint32_t winA_ = __builtin_amdgcn_alignbit(hi_, lo_, Q);                     \
        const uint32_t winB_ = __builtin_amdgcn_alignbit(lo_, lo2_, Q);                    \
        const uint32_t q1_ = ffbh(winA_);                                                  \
        const uint32_t kk1_ = (winA_ < (1u << 24)) ? 16u : k;                              \
        const uint32_t nu1_ = ~(q1_ + kk1_); /* minus the code length */                   \
        const uint32_t win2_ = __builtin_amdgcn_alignbit(winA_, winB_, nu1_);              \
        const uint32_t q2_ = ffbh(win2_);                                                  \
        const uint32_t kk2_ = (win2_ < (1u << 24)) ? 16u : k;                              \
        const uint32_t nu2_ = ~(q2_ + kk2_);                                               \
        asm("v_add3_u32 %0, %1, %2, %3" : "=v"(Q) : "v"(Q), "v"(nu1_), "v"(nu2_));         \
        z1 = (q1_ << kk1_) + __builtin_amdgcn_ubfe(winA_, nu1_, kk1_);                     \
        z2 = (q2_ << kk2_) + __builtin_amdgcn_ubfe(win2_, nu2_, kk2_);                     \
    }
// The unmasked group of the kernels that keep samples: eight pairs, two samples per ring access.  acc: the lane's running sum
// of the deltas (int32_t, the sample in its low 16 bits).  Declares pr[kGS / 2]: the group's samples two to a register, the
// earlier one in the low half, every register ^ flip (0u: the samples as they are).
#define LANE_GROUP_PAIRS(acc, pr, flip)                                                                                          \
    uint32_t pr[kGS / 2];                                                                                                        \
    _Pragma("unroll") for (int u_ = 0; u_ < kGS; u_ += 2) {                                                                      \
        LANE_PAIR(z1_, z2_)                                                                                                      \
        acc += (int32_t)(z1_ >> 1) ^ -(int32_t)(z1_ & 1u);                                                                       \
        const uint32_t a1_ = (uint32_t)acc;                                                                                      \
        acc += (int32_t)(z2_ >> 1) ^ -(int32_t)(z2_ & 1u);                                                                       \
        pr[u_ / 2] = __builtin_amdgcn_perm((uint32_t)acc, a1_, 0x05040100u) ^ (flip); /* low halves of the two running sums */   \
    }
// the masked form: one code per ring access (win == 0 only past the end of a corrupt stream)
#define LANE_ONE(z)                                                                        \
    uint32_t z;                                                                            \
    {                                                                                      \
        const uint32_t row_ = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)kLogRW);              \
        const uint32_t *wp_ = myring + row_ * 64u;                                         \
        const uint32_t lo_ = wp_[0], hi_ = wp_[64];                                        \
        const uint32_t win_ = __builtin_amdgcn_alignbit(hi_, lo_, Q);                      \
        const uint32_t q_ = ffbh(win_);                                                    \
        const uint32_t kk_ = (win_ < (1u << 24)) ? 16u : k;                                \
        const uint32_t used_ = q_ + kk_ + 1u;                                              \
        z = (q_ << kk_) + __builtin_amdgcn_ubfe(win_, 32u - used_, kk_);                   \
        Q -= used_;                                                                        \
    }
// payload words the codes so far took: bits = -Q - 32 s0 (Q counts from A), positions are kept mod 2^32
#define LANE_USED_WORDS() ((((0u - Q) - 32u * s0 + 31u) >> 5) & kWMask)
// A valid waveform's codes end inside its last payload word, n_i = ceil(bits / 32) (src/deltaRice.c:237-241), and every word
// of it has been through the ring by then.  A payload that ends before its samples do, or whose codes do not end in its last
// word, fails one of the two.
#define LANE_MISSES_LAST_WORD_AT(used_words) ((used_words) != (n & kWMask) || flw < endw)
#define LANE_MISSES_LAST_WORD() LANE_MISSES_LAST_WORD_AT(LANE_USED_WORDS())
