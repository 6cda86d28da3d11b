// drx_blocks_body.inc -- the body of a kernel that gives a workgroup a block of a waveform's stream, included INSIDE the kernel's
// definition (k_decode_blocks, drx_blocks.hip; k_stats_blocks, drx_stats_blocks.hip; k_pulses_blocks, drx_pulses_blocks.hip;
// k_windows_blocks, drx_windows_blocks.hip; k_trc_blocks, drx_transcode_blocks.hip; k_bins_blocks, drx_bins_blocks.hip)
// behind its arguments: text, not a function, because k_decode_blocks is sensitive to how its arguments reach it (an inlined
// function with the same body was compiled to other code: other spills, another schedule).  The including kernel provides NT,
// RESID, SW, FUSE, STATS, PULSES, WINDOWS, TRANSCODE, BINS, the arguments of k_decode_blocks by name, `sa` (BlkStatsArgs), `pa`
// (BlkPulseArgs), `wa` (BlkWindowArgs), `ta` (BlkTrcArgs) and `ba` (BlkBinsArgs).
    static_assert(!FUSE || RESID, "the fused inverse filter works on residuals");
    using BG = BlkGeom<NT, SW>;
    constexpr int kBlkSegW = SW;
    constexpr uint32_t kBlkLaneCap = BG::kLaneCap, kBlkLaneStride = BG::kLaneStride, kCap2 = BG::kLaneCap / 2u;
    constexpr uint32_t K = BG::kLdsWords + 2u;  // word w of the image sits at W[K + 1 - w]; K = 2 (mod 4): 16-byte quads
    constexpr uint32_t C = 32u * K;
    constexpr int NW = NT / 64;
    constexpr uint32_t kSegBits = 32u * kBlkSegW;
    // one LDS object, the image first: its three-word windows are read with immediate offsets from address 0
    constexpr uint32_t kWSize = BG::kLdsWords + 4u, kObufWords = BG::kStageWords;  // (kOutCap + 8 samples fit: NT >= 8)
    __shared__ __attribute__((aligned(16))) uint32_t lds[kWSize + kObufWords + NT + 2 * NW + 4 + 8 + 4 + 3 * NW];  // (+ s_unit, s_pred, s_next, s_vote[3], ..., FUSE: s_F[NW][3])
    uint32_t *const W = lds;
    uint32_t *const stage = lds + kWSize;                        // phase 1: lane-major, kBlkLaneStride dwords per lane
    uint16_t *const obuf = reinterpret_cast<uint16_t *>(stage);  // phase 2: the block's samples in output order
    uint32_t *const s_e = lds + kWSize + kObufWords;
    uint32_t(*const s_tot)[NW] = reinterpret_cast<uint32_t(*)[NW]>(s_e + NT);
    uint64_t *const s_b = reinterpret_cast<uint64_t *>(s_e + NT + 2 * NW);  // (kWSize, kObufWords, NT, 2 NW: all even)
    uint32_t &s_unit = s_e[NT + 2 * NW + 4], &s_pred = s_e[NT + 2 * NW + 5];
    uint32_t(*const s_F)[3] = reinterpret_cast<uint32_t(*)[3]>(s_e + NT + 2 * NW + 16);  // FUSE: a wavefront's zero-state response
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id(), wv = (int)(tid >> 6);
    uint32_t k = G.k;
    asm volatile("" : "+v"(k));  // in a VGPR for good: the parse selects between k and 16 per code, and re-materialised it per pair
    // TRANSCODE: the pack launch -- a block's start comes from its slot of the table, no block waits for another (drx_blocks.h)
    [[maybe_unused]] bool t_pack = false;
    if constexpr (TRANSCODE) t_pack = ta.pack != 0u;
    // A ticket is a RUN of run_len consecutive blocks of one waveform, dealt run-major: run 0 of every waveform, then run 1
    // of every waveform, ...  Inside a run only its first block talks to other workgroups (where the predecessor's
    // stream ended, the look-back for samples and sum in front of it); the others start exactly where the block before
    // them ended, with counts carried in registers.  The host makes runs longer than one block only when there are more
    // waveforms than workgroups: two runs of ONE waveform in flight together serialise (the later one's look-back waits
    // for the earlier one's last block).  The image of the next block -- of this run or of the next ticket's -- travels
    // while the current block's samples are put in order and written out, and the next ticket is drawn a run ahead.
    // In-kernel stamps of the first version (a ticket per block, waveform-major: 768 blocks of ONE 14 M-sample waveform
    // in flight, every one polling twelve windows of aggregates) had 11 % of a workgroup's time in the parse and 77 % in
    // four waits: ticket, image, predecessor's end, look-back (profiles/r02_notes.md).
    // the waveforms of THIS launch: all of the batch, or (ragged batches) those of one length class -- tickets are dealt
    // run-major over them, and a class whose waveforms differ by less than 2x in length wastes few tickets on empty runs
    uint32_t n_waves32_ = wave_list ? n_list : (uint32_t)G.total_waves;
    if constexpr (PULSES) { if (pa.n_redo) n_waves32_ = *pa.n_redo; }  // (a list whose length is known on the device alone)
    const uint32_t n_waves32 = n_waves32_;
    const uint32_t max_runs = (info[0] + run_len - 1u) / run_len;
    const uint64_t total_units64 = (uint64_t)max_runs * n_waves32;
    const uint32_t total_units = total_units64 > 0xffffffffull ? 0xffffffffu : (uint32_t)total_units64;
    typedef uint16_t __attribute__((address_space(1))) g_u16;
    typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
    typedef u32x4v __attribute__((address_space(1))) g_uint4;
    constexpr int NQ = (int)((BG::kLdsWords / 4u + NT - 1u) / NT);  // 16-byte pieces of an image per thread

    // tickets: every lower ticket is held by a running (or finished) workgroup, so waiting for a predecessor cannot
    // deadlock whatever the dispatch order; the grid is sized to be resident
    uint32_t &s_next = s_e[NT + 2 * NW + 6];
    uint32_t &s_front = s_e[NT + 2 * NW + 7];   // settle(): the lowest lane that started again last round and how far its end moved
    uint32_t &s_defer = s_e[NT + 2 * NW + 11];  // this block does not publish its end before its start is verified
    uint32_t *const s_vote = s_e + NT + 2 * NW + 8;  // [3], in rotation, so that a vote needs one barrier
    uint32_t vote_no = 0;
    // true in every thread if `v` holds in any thread of the workgroup.  Vote i uses word i mod 3; thread 0 clears the word
    // of vote i + 1 on its way into vote i: every thread has passed the barrier of vote i - 1 by then, so none still
    // reads the word of vote i - 2 (the same word), and the word of vote i - 1, which slow threads may still read, is another.
    auto wg_any = [&](bool v) __attribute__((always_inline)) {
        uint32_t *w = s_vote + vote_no % 3u;
        if (__any(v) && lane == 0) __hip_atomic_fetch_or(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (tid == 0) s_vote[(vote_no + 1u) % 3u] = 0u;
        blk_barrier();
        ++vote_no;
        return *w != 0u;
    };
    if (tid == 0) { s_unit = atomicAdd(ticket, 1u); s_vote[0] = 0u; s_vote[1] = 0u; s_vote[2] = 0u; }
    __syncthreads();
    uint32_t unit = s_unit;
    __syncthreads();
    // where a ticket's run lies: waveform, first block, payload
    struct RunRef { uint64_t g, pay_lo; uint32_t n, blk_lo, blk_hi; };
    auto run_of = [&](uint32_t u) __attribute__((always_inline)) {
        RunRef q;
        const uint32_t run = u / n_waves32;
        const uint32_t j = u - run * n_waves32;
        q.g = wave_list ? wave_list[j] : j;
        q.pay_lo = wave_off[q.g] + 1u;
        q.n = wave_words[q.g];
        const uint32_t n_blocks = (q.n + BG::kWords - 1u) / BG::kWords;
        q.blk_lo = run * run_len;
        q.blk_hi = (q.blk_lo + run_len < n_blocks) ? q.blk_lo + run_len : n_blocks;  // (blk_lo >= n_blocks: an empty run)
        if constexpr (TRANSCODE) { if (t_pack && !ta.keep[q.g]) q.blk_hi = q.blk_lo; }  // (a listed waveform: the lane kernel packs it)
        return q;
    };
    // image of block b: words [b kWords - kBlkPre, (b + 1) kWords + kBlkTail) of the payload, from a 16-byte boundary
    auto image_base = [&](uint64_t pay_lo, uint32_t b) { return ((int64_t)(pay_lo + (uint64_t)b * BG::kWords) - (int64_t)kBlkPre) & ~(int64_t)3; };
    // The fetch is unconditional 16-byte loads from a clamped address and nothing else: a load inside a branch is waited
    // for at the end of that branch, which would put the whole round trip back in front of the parse.  What the clamp
    // and the payload's end invalidate is sorted out when the registers are written to LDS.  (in_words >= 64 here: the
    // host gives this decoder waveforms of 2048 samples and more.)
    const int64_t a_max = (int64_t)in_words - 4;
    auto fetch_image = [&](const RunRef &q, uint32_t b, uint4 (&v)[NQ]) __attribute__((always_inline)) {
        const int64_t al = image_base(q.pay_lo, b);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int64_t a = al + 4 * (int64_t)(tid + (uint32_t)i * NT);
            const int64_t ac = a < 0 ? 0 : (a > a_max ? a_max : a);
            v[i] = *reinterpret_cast<const uint4 *>(in + ac);
        }
    };
    auto store_image = [&](const RunRef &q, uint32_t b, const uint4 (&v)[NQ]) __attribute__((always_inline)) {
        const int64_t al = image_base(q.pay_lo, b);
        const int64_t pay_hi = (int64_t)(q.pay_lo + q.n);  // nothing behind the payload is read as stream
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const uint32_t qd = tid + (uint32_t)i * NT;
            const int64_t a = al + 4 * (int64_t)qd;
            if (qd >= BG::kLdsWords / 4u) continue;
            uint4 w = v[i];
            if (a < 0 || a > a_max) {  // the clamp moved this piece: word by word (the first and the last piece of a batch)
                auto ld = [&](int64_t j) { return (j >= 0 && j < (int64_t)in_words) ? in[j] : 0u; };
                w = make_uint4(ld(a), ld(a + 1), ld(a + 2), ld(a + 3));
            }
            w.x = (a + 0 < pay_hi) ? w.x : 0u;
            w.y = (a + 1 < pay_hi) ? w.y : 0u;
            w.z = (a + 2 < pay_hi) ? w.z : 0u;
            w.w = (a + 3 < pay_hi) ? w.w : 0u;
            // words 4q .. 4q+3 at W[K - 4q - 2 .. K - 4q + 1]: one 16-byte store (K - 4q - 2 = kLdsWords - 4q)
            *reinterpret_cast<uint4 *>(W + (BG::kLdsWords - 4u * qd)) = make_uint4(w.w, w.z, w.y, w.x);
        }
    };
    // ---- FUSE: the inverse filter over the samples [a0, a0 + nsamp) of the staging buffer, in place ----
    V3 xs{0u, 0u, 0u};  // the state in front of the next sample of the waveform (y[i-1], y[i-2], y[i-3]); thread 0's is the one that counts
    auto iir_lds = [&](uint32_t a0, uint32_t nsamp) __attribute__((always_inline)) {
        constexpr uint32_t M = kBlkLaneCap, NP = M / 2u;  // samples / dwords per lane
        static_assert(NP % 2u == 0u, "a lane's share is moved in 8-byte pieces");
        if (nsamp == 0u) return;
        const uint32_t c1 = itab[kRunTabC], c2 = itab[kRunTabC + 1], c3 = itab[kRunTabC + 2], sg = itab[kRunTabC + 3];
        uint32_t *const mine = reinterpret_cast<uint32_t *>(obuf) + tid * NP;
        // the recurrence over my run from state s, two dwords (four samples) of LDS at a time -- the run is read once per pass
        // rather than held in 38 registers across the scan (that form needed 214 registers: two workgroups per CU instead of
        // three).  Thread 0's first a0 entries lie in front of the block's first sample: no step there.  EMIT: the samples
        // replace the residuals.
        uint32_t last2 = 0, last1 = 0;  // EMIT: the run's last two dwords (the last lane may have to go on behind its share)
        auto run = [&](V3 s0, auto emit_tag) __attribute__((always_inline)) {
            constexpr bool EMIT = decltype(emit_tag)::value;
            uint32_t sx = s0.x, sy = s0.y, sz = s0.z;
            // one dword = two samples; SKIP: the dword may lie in front of the block's first sample (thread 0's first four)
            // (component by component: a select between two structs is compiled as a select between their ADDRESSES, and the
            // states went through scratch memory)
            auto pair = [&](uint32_t dj, uint32_t j, auto skip_tag) __attribute__((always_inline)) {
                constexpr bool SKIP = decltype(skip_tag)::value;
                const uint32_t lo = dj & 0xffffu, hi = dj >> 16;
                uint32_t a = __umul24(lo, sg) + __umul24(c1, sx) + __umul24(c2, sy) + __umul24(c3, sz);
                if (SKIP) {
                    const bool skip = tid == 0u && 2u * j < a0;
                    const uint32_t nx = skip ? sx : a, ny = skip ? sy : sx, nz = skip ? sz : sy;
                    a = skip ? lo : a;
                    sx = nx; sy = ny; sz = nz;
                } else {
                    sz = sy; sy = sx; sx = a;
                }
                uint32_t b = __umul24(hi, sg) + __umul24(c1, sx) + __umul24(c2, sy) + __umul24(c3, sz);
                if (SKIP) {
                    const bool skip = tid == 0u && 2u * j + 1u < a0;
                    const uint32_t nx = skip ? sx : b, ny = skip ? sy : sx, nz = skip ? sz : sy;
                    b = skip ? hi : b;
                    sx = nx; sy = ny; sz = nz;
                } else {
                    sz = sy; sy = sx; sx = b;
                }
                return __builtin_amdgcn_perm(b, a, 0x05040100u);
            };
            uint2 w = *reinterpret_cast<const uint2 *>(mine);
#pragma unroll
            for (uint32_t j0 = 0; j0 < 4u; j0 += 2u) {  // the first eight samples
                const uint2 wn = *reinterpret_cast<const uint2 *>(mine + j0 + 2u);
                const uint32_t o0 = pair(w.x, j0, std::true_type{}), o1 = pair(w.y, j0 + 1u, std::true_type{});
                if (EMIT) *reinterpret_cast<uint2 *>(mine + j0) = make_uint2(o0, o1);
                w = wn;
            }
            // the rest, the next piece in flight while one is worked on; NOT unrolled further: all 19 loads of a fully unrolled
            // loop were hoisted to its top (180 registers: two workgroups per CU instead of three)
#pragma unroll 2
            for (uint32_t j0 = 4u; j0 < NP; j0 += 2u) {
                const uint32_t jn = j0 + 2u < NP ? j0 + 2u : j0;
                const uint2 wn = *reinterpret_cast<const uint2 *>(mine + jn);
                const uint32_t o0 = pair(w.x, j0, std::false_type{}), o1 = pair(w.y, j0 + 1u, std::false_type{});
                if (EMIT) {
                    *reinterpret_cast<uint2 *>(mine + j0) = make_uint2(o0, o1);
                    last2 = o0; last1 = o1;
                }
                w = wn;
            }
            return V3{sx, sy, sz};
        };
        // pass 1, then the scan: inside the wavefront, then over the wavefronts
        V3 F = lo16(run(V3{tid == 0u ? xs.x : 0u, tid == 0u ? xs.y : 0u, tid == 0u ? xs.z : 0u}, std::false_type{}));
#pragma unroll
        for (int dd = 0; dd < 6; ++dd) {
            const M3 P = load_m3(itab + kRunTabPL + 9 * dd);  // A^(M 2^dd)
            const V3 up = shfl_up_v3(F, 1 << dd);
            if (lane >= (1 << dd)) F = lo16(add(F, mul(P, up)));
        }
        V3 E = shfl_up_v3(F, 1);  // the state in front of my run as far as my wavefront knows
        if (lane == 0) E = V3{0u, 0u, 0u};
        if (lane == 63) { s_F[wv][0] = F.x; s_F[wv][1] = F.y; s_F[wv][2] = F.z; }
        blk_barrier();
        V3 XW{0u, 0u, 0u};  // ... and in front of my wavefront
        if (NW > 1) {
            const M3 PW = load_m3(itab + kRunTabPL + 9 * 6);  // A^(64 M)
            for (int w = 0; w < wv; ++w) XW = lo16(add(mul(PW, XW), V3{s_F[w][0], s_F[w][1], s_F[w][2]}));
        }
        V3 S = E;  // (thread 0: the state in front of the block, as in pass 1)
        if (tid == 0u) { S.x = xs.x; S.y = xs.y; S.z = xs.z; }
        if (NW > 1 && wv > 0) S = lo16(add(mul(load_m3(itab + kRunTabPLANE + 9 * lane), XW), E));
        // pass 2: the samples
        (void)run(S, std::true_type{});
        // (up to seven samples lie behind the last lane's share when the block's first sample is not 16-byte aligned and the
        // buffer is full: the last lane goes on, one sample at a time)
        if (tid == NT - 1u && a0 + nsamp > NT * M) {
            V3 s{last1 >> 16, last1 & 0xffffu, last2 >> 16};
            for (uint32_t i = NT * M; i < a0 + nsamp; ++i) {
                const uint32_t v = (__umul24((uint32_t)obuf[i], sg) + __umul24(c1, s.x) + __umul24(c2, s.y) + __umul24(c3, s.z)) & 0xffffu;
                obuf[i] = (uint16_t)v;
                s = V3{v, s.x, s.y};
            }
        }
        blk_barrier();
        // the state behind these samples: the last three of them (fewer: what was in front moves down)
        if (tid == 0u) {
            const uint16_t *e = obuf + (a0 + nsamp);
            if (nsamp >= 3u) xs = V3{e[-1], e[-2], e[-3]};
            else if (nsamp == 2u) xs = V3{e[-1], e[-2], xs.x};
            else xs = V3{e[-1], xs.x, xs.y};
        }
    };
    if (unit >= total_units) return;
    RunRef cur = run_of(unit);
    uint4 img[NQ];
    if (cur.blk_lo < cur.blk_hi) fetch_image(cur, cur.blk_lo, img);
    for (;;) {
        // the next ticket, drawn a run ahead.  Inline asm: a returning atomic the compiler sees inside `if (tid == 0)` is
        // waited for at the end of that branch; this one is waited for where its value is used.  The address travels in a
        // VGPR pair (`off` form): the hardware interlocks VGPR operands, whereas an SGPR base restored from a spill by
        // v_readlane in the instruction in front needs five wait states that nothing pads inside an asm statement (round 2:
        // an experimental form of this kernel faulted on address 0 that way).  tools/check_asm_hazards.py, run by `make hip`
        // on the gfx950 disassembly, checks both that rule and that nothing touches next_ticket before the s_waitcnt below.
        uint32_t next_ticket = 0;
        if (tid == 0)
            asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(next_ticket) : "v"((uint64_t)(uintptr_t)ticket), "v"(1u) : "memory");
        const uint64_t g = cur.g, pay_lo = cur.pay_lo;
        const uint32_t n = cur.n, blk_lo = cur.blk_lo, blk_hi = cur.blk_hi;
        const WaveRef r = locate(G, g);
        const uint32_t len = r.len;
        int16_t *y = out + r.sample_off;
        const uint32_t n_blocks = (n + BG::kWords - 1u) / BG::kWords;
        [[maybe_unused]] int32_t p_tv = 0;  // PULSES: the waveform's clamped threshold, v > p_tv is over
        if constexpr (PULSES) p_tv = pulse_threshold(pa.thr_tab != nullptr, pa.thr_tab ? pa.thr_tab[g * pa.thr_stride] : 0, pa.thr, pa.neg != 0u);
        RunRef nxt = cur;
        uint32_t next_unit = 0xffffffffu;
        if (blk_lo >= blk_hi) {  // an empty run (a waveform with fewer blocks than the longest): only the hand-over
            if (tid == 0) {
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(next_ticket)::"memory");
                s_next = next_ticket;
            }
            blk_barrier();
            next_unit = s_next;
            blk_barrier();
            if (next_unit < total_units) { nxt = run_of(next_unit); if (nxt.blk_lo < nxt.blk_hi) fetch_image(nxt, nxt.blk_lo, img); }
        }
        uint64_t run_base_c = 0;   // samples in front of the current block (known from the run's second block on)
        uint32_t run_acc = 0;      // the running sum there
        uint32_t carry_rel = 0;    // where the previous block's last code ended, in bits behind that block
        for (uint32_t blk = blk_lo; blk < blk_hi; ++blk) {
            const bool first_of_run = blk == blk_lo;
            const uint32_t sidx = (uint32_t)g * slots_per_wave + blk;  // this block's look-back entry and end word
            const uint32_t w0 = blk * BG::kWords;
            const uint32_t avail = (n - w0 < BG::kWords) ? n - w0 : BG::kWords;
            const uint32_t s_i0 = (uint32_t)((int64_t)(pay_lo + w0) - image_base(pay_lo, blk));  // image index of the block's first word
            store_image(cur, blk, img);
            if (tid == 0) s_defer = 0u;
            blk_barrier();

            // ---- phase 1: where the codes of my segment start, how many there are, what they sum to ----
            const uint32_t B0 = 32u * s_i0, bend = B0 + 32u * avail;
            const uint32_t bj = B0 + kSegBits * tid;
            const bool active = bj < bend;
            const uint32_t lim = (bj + kSegBits < bend) ? bj + kSegBits : bend;
            // lane 0 knows its start when the block is the waveform's first (bit 0) or follows one of this run
            [[maybe_unused]] uint32_t t_rel0 = 0u;  // TRANSCODE, pack: a run's first block starts where the sizes launch found its first code
            if constexpr (TRANSCODE) { if (t_pack && first_of_run) t_rel0 = ta.slots[(uint64_t)sidx * kTrcSlotWords + 3u]; }
            const bool exact0 = tid == 0 && (blk == 0 || !first_of_run || (TRANSCODE && t_pack));
            const uint32_t start0 = B0 + (first_of_run ? t_rel0 : carry_rel);
            uint32_t Qp = C - (exact0 ? start0 : (active ? bj - kBlkGuessBits : B0));
            uint32_t cnt = 0, sum = 0;
            blk_skip_pairs(W, k, active && !exact0, Qp, C - bj);
            if (!active) Qp = C - B0;
            uint32_t f = C - Qp;  // first code that starts in my segment
            uint32_t *const my_stage = stage + tid * kBlkLaneStride;
            // where the waveform's zero padding can be: its last payload word, if this block holds it
            const uint32_t qpad = (n - 1u >= w0 && n - 1u < w0 + BG::kWords) ? C - (B0 + 32u * (n - 1u - w0)) : 0u;
            if (qpad) blk_parse<kBlkCount, RESID, true>(W, k, active, Qp, C - lim, cnt, sum, 0u, nullptr, my_stage, qpad, kCap2);
            else blk_count_pairs<RESID>(W, k, active, Qp, C - lim, cnt, sum, my_stage, kCap2);
            if (!active) { cnt = 0; sum = 0; }
            uint32_t e = C - Qp;  // first code that starts behind it (or where the padding starts)

            // Every lane must start where its predecessor ended; lanes that do not, start again from there.
            // CREEP: in a stream of equal-length codes whose pattern reads as the same codes from another phase (a slope-1 ramp
            // is "1010" per sample) a parse never falls into step: lanes that guessed the same wrong phase agree with one
            // another, and once lane 0 is put right the correction moves ONE lane per round (243 rounds per block measured,
            // NOPTREX-shaped ramps 81 ms).  Its signature -- the lowest lane that starts again advances by exactly one per
            // round and its end moves by the same amount each time -- is looked for, and after three such rounds every lane
            // behind the front is shifted by that amount at once.  Only where to start again is guessed (at most four times per
            // call); what is accepted is still the chain of equalities.  Noise and quiet data never show the signature.
            auto settle = [&]() __attribute__((always_inline)) {
                uint32_t prev_front = 0xffffffffu, creep = 0, jumps = 0;
                if (tid == 0) s_front = 0xffffffffu;
                for (uint32_t it = 0; it <= 2u * (uint32_t)NT + 8u; ++it) {
                    s_e[tid] = e;
                    blk_barrier();
                    const uint32_t want = tid ? s_e[tid - 1u] : f;
                    bool changed = active && want != f;
                    uint32_t from = want;
                    const uint32_t front = s_front;  // (lane << 8) | (how far its end moved + 128), 0xffffffff: nobody started again
                    if (it > 0u) {
                        const bool step = front != 0xffffffffu && prev_front != 0xffffffffu && (front >> 8) == (prev_front >> 8) + 1u &&
                                          (front & 0xffu) == (prev_front & 0xffu) && (front & 0xffu) != 128u && (front & 0xffu) != 0u;
                        creep = step ? creep + 1u : 0u;
                        prev_front = front;
                        if (creep >= 2u && jumps < 4u) {
                            creep = 0;
                            ++jumps;
                            prev_front = 0xffffffffu;
                            const uint32_t to = f + (front & 0xffu) - 128u;
                            if (active && tid > (front >> 8) && (int32_t)(to - bj) >= 0 && to < lim) { from = to; changed = from != f; }
                        }
                    }
                    if (!wg_any(changed)) break;  // (also: every read of s_e and s_front is done before the next write)
                    if (tid == 0) s_front = 0xffffffffu;
                    blk_barrier();
                    const uint32_t e_old = e;
                    if (changed) { f = from; Qp = C - f; cnt = 0; sum = 0; }
                    blk_parse<kBlkCount, RESID>(W, k, changed, Qp, C - lim, cnt, sum, 0u, nullptr, my_stage, qpad, kCap2);
                    if (changed) {
                        e = C - Qp;
                        const int32_t d = (int32_t)(e - e_old);
                        const uint32_t dd = (d > -128 && d < 128) ? (uint32_t)(d + 128) : 0u;
                        __hip_atomic_fetch_min(&s_front, (tid << 8) | dd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            };
            // A block whose lane 0 only guessed its start and reads a pattern that another phase reads as the same codes does
            // not publish its end before its predecessor's has confirmed the guess: the end would move, and a successor that
            // started from it sends the whole waveform to the one-workgroup fallback (ramps: 25 x 14 M samples 824 ms).
            // (asked of lane 0, whose guess decides whether the block has to start again, and of the last lane, whose end is the one published)
            if (first_of_run && blk > 0u && cnt >= 8u && (tid == 0u || tid == (avail + (uint32_t)kBlkSegW - 1u) / (uint32_t)kBlkSegW - 1u)) {
                bool amb = false;
                const BlkPair p0 = blk_pair<false>(W, k, C - f);
                const uint32_t f2 = f + (0u - p0.nu1), P = 0u - p0.nu2;  // (nu = minus the code length; from the second code on)
                if (P != 0u && P < 26u && P * (cnt - 1u) == e - f2) {  // codes of one length ...
                    const uint32_t w0 = blk_window(W, C - f2);
                    if (w0 == blk_window(W, C - (f2 + P)) && w0 == blk_window(W, C - (f2 + 2u * P))) {  // ... of one pattern ...
                        for (uint32_t r = 1; r < P && !amb; ++r)  // ... that reads as a code of that length from another phase
                            amb = (0u - blk_pair<false>(W, k, C - (f2 + r)).nu1) == P;
                    }
                }
                if (amb) s_defer = 1u;
            }
            settle();
            const bool defer = s_defer != 0u;  // (read behind settle()'s barriers)
            const uint32_t last_active = (avail + (uint32_t)kBlkSegW - 1u) / (uint32_t)kBlkSegW - 1u;
            const uint32_t e_last0 = s_e[last_active];
            const bool last_of_run = blk + 1u == blk_hi;
            // the end of this run = the start of the next one, published as soon as it is known
            if (tid == 0 && last_of_run && !defer)
                __hip_atomic_store(ends + sidx, 0x80000000u | (e_last0 - bend), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (first_of_run && blk > 0 && !(TRANSCODE && t_pack)) {
                if (tid == 0) {
                    uint32_t v = 0, spins = 0;
                    for (;;) {
                        v = __hip_atomic_load(ends + sidx - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (v & 0x80000000u) break;
                        __builtin_amdgcn_s_sleep(2);
                        if (++spins > (1u << 24)) { atomicOr(&st->err, kErrInternal); break; }  // cannot happen; never hang
                    }
                    s_pred = v & 0xffffu;
                }
                blk_barrier();
                const uint32_t true_f0 = B0 + s_pred;
                const bool fix0 = tid == 0 && true_f0 != f;
                if (fix0) s_next = true_f0 - f;  // (how far lane 0 moves; s_next is not in use here)
                if (wg_any(fix0)) {
                    // a block that held its end back reads one pattern throughout: its lanes all guessed the phase lane 0 guessed,
                    // and move with it (a guess again: settle() below accepts nothing but the chain of equalities)
                    bool mv = fix0;
                    uint32_t to = true_f0;
                    if (defer && tid != 0u && active) {
                        const uint32_t t = f + s_next;
                        if ((int32_t)(t - bj) >= 0 && t < lim) { mv = true; to = t; }
                    }
                    if (mv) { f = to; Qp = C - f; cnt = 0; sum = 0; }
                    blk_parse<kBlkCount, RESID>(W, k, mv, Qp, C - lim, cnt, sum, 0u, nullptr, my_stage, qpad, kCap2);
                    if (mv) e = C - Qp;
                    settle();
                    // a one-block run has published its end already, and its successor has started from it: if that end
                    // moved, the successor's run is wrong
                    if (tid == 0 && last_of_run && !defer && s_e[last_active] != e_last0 && blk + 1u < n_blocks) atomicExch(fail + g, 1u);
                }
                if (tid == 0 && last_of_run && defer)
                    __hip_atomic_store(ends + sidx, 0x80000000u | (s_e[last_active] - bend), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const uint32_t e_end = s_e[last_active];  // (after a correction: the corrected end)

            // ---- samples and residual sum in front of my segment (workgroup scan) and in front of the block ----
            const uint32_t incl_c = wave_incl_scan_dpp(cnt), incl_s = wave_incl_scan_dpp(sum);
            if (lane == 63) { s_tot[0][wv] = incl_c; s_tot[1][wv] = incl_s; }
            if (tid == 0 && last_of_run) {  // (drawn at the start of the run: it has arrived)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(next_ticket)::"memory");
                s_next = next_ticket;
            }
            blk_barrier();
            uint32_t pre_c = 0, pre_s = 0, tot_c = 0, tot_s = 0;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const uint32_t tc = s_tot[0][i], ts = s_tot[1][i];
                if (i < wv) { pre_c += tc; pre_s += ts; }
                tot_c += tc;
                tot_s += ts;
            }
            if (wv == 0) {
                const uint64_t mine = ((uint64_t)tot_c << 16) | (uint64_t)(tot_s & 0xffffu);
                uint64_t ex_c = run_base_c, ex_s = run_acc;
                if (blk == 0) {
                    ex_c = 0;
                    ex_s = 0;
                } else if (TRANSCODE && t_pack) {
                    if (first_of_run) {  // (the sizes launch left it in the block's slot; a re-code needs no running sum)
                        if constexpr (TRANSCODE) ex_c = ta.slots[(uint64_t)sidx * kTrcSlotWords + 4u];
                        ex_s = 0;
                    }
                } else if (first_of_run) {
                    // lookback_walk (drx_lookback.h): entry sidx = {samples << 16 | 16-bit residual sum} of a block, scanned from
                    // block 0 of this waveform, the two fields summed apart
                    ex_c = 0;
                    ex_s = 0;
                    scan_publish(state, sidx, kScanAgg | mine, lane);
                    lookback_walk<kBlkGateSleep>(state, sidx, (int64_t)sidx - (int64_t)blk, lane, st, [&](uint64_t s0, uint64_t s1, bool in0, bool in1) {
                        const uint64_t v0 = in0 ? (s0 & kScanValMask) : 0ull, v1 = in1 ? (s1 & kScanValMask) : 0ull;
                        ex_c += wave_sum_u64((v0 >> 16) + (v1 >> 16));
                        ex_s += wave_sum_u64((v0 & 0xffffull) + (v1 & 0xffffull));
                    });
                }
                // everything in front of this block is known now: its successors find a prefix here
                scan_publish(state, sidx, kScanPrefix | ((((ex_c + tot_c) << 16) | ((ex_s + tot_s) & 0xffffull)) & kScanValMask), lane);
                if (lane == 0) { s_b[0] = ex_c; s_b[1] = ex_s; }
            }
            blk_barrier();
            const uint64_t base_c = s_b[0];
            const uint32_t acc_base = (uint32_t)s_b[1];
            run_base_c = base_c + tot_c;
            run_acc = acc_base + tot_s;
            carry_rel = e_end - bend;
            // The next block's image -- of this run or of the next ticket's -- travels while this one's samples are put in
            // order and written out.  (Issued earlier -- at the top of the block, or behind the count -- the loads were
            // measured no faster to arrive: the wait in front of the next block is for this block's output lines, whose
            // store loop the compiler cannot count, and retiring the loads by hand in front of those stores only moved the
            // wait there: profiles/r02_notes.md.)
            if (!last_of_run) {
                fetch_image(cur, blk + 1u, img);
            } else {
                next_unit = s_next;
                if (next_unit < total_units) { nxt = run_of(next_unit); if (nxt.blk_lo < nxt.blk_hi) fetch_image(nxt, nxt.blk_lo, img); }
            }
            // the waveform has `len` samples; a code decoded out of the zero padding behind the last one does not count
            const uint32_t blk_first = base_c < (uint64_t)len ? (uint32_t)base_c : len;
            const uint32_t blk_count = (tot_c < len - blk_first) ? tot_c : len - blk_first;
            const uint32_t rel0 = pre_c + incl_c - cnt;  // my first sample, relative to the block's first
            const uint32_t todo = rel0 >= blk_count ? 0u : ((cnt < blk_count - rel0) ? cnt : blk_count - rel0);
            // Verdicts, left to the kernel that runs after this one (a block behind a mis-started one counts garbage, and its
            // waveform is flagged for the fallback anyway): the waveform's last block must bring the count to exactly `len`
            // samples, and its last code must end in the last payload word: n_i = ceil(bits / 32) (src/deltaRice.c:237-241).
            if (tid == 0 && blk + 1u == n_blocks) {
                if (base_c + tot_c != (uint64_t)len || w0 + ((e_end - B0 + 31u) >> 5) != n) atomicExch(suspect + g, 1u);
            }

            // FUSE: the filter's state in front of this block -- zero at the waveform's start, thread 0's own inside a run, the
            // previous run's last block's across runs (long published where runs of one waveform are not in flight together)
            if (FUSE && first_of_run && tid == 0u) {
                xs = V3{0u, 0u, 0u};
                if (blk > 0u) {
                    uint64_t v = 0;
                    uint32_t spins = 0;
                    for (;;) {
                        v = __hip_atomic_load(xstate + sidx - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (v >> 63) break;
                        __builtin_amdgcn_s_sleep(2);
                        if (++spins > (1u << 24)) { atomicOr(&st->err, kErrInternal); break; }  // cannot happen; never hang
                    }
                    xs = V3{(uint32_t)v & 0xffffu, (uint32_t)(v >> 16) & 0xffffu, (uint32_t)(v >> 32) & 0xffffu};
                }
            }
            if constexpr (TRANSCODE) {
#include "drx_blocks_trc.inc"
            } else if constexpr (BINS) {
#include "drx_blocks_bins.inc"
            } else if constexpr (PULSES) {
                // ---- phase 2, pulses: every lane summarises the runs of over-threshold samples among its own samples
                // (drx_pulse_runs.h), a scan over the lanes with pulse_combine() tells each what lies in front of it inside
                // the block -- the run open there and how many of the block's pulses -- and a second pass over the same staged
                // values stores the pulses that close in the lane's samples to the block's staging slots, numbered inside the
                // block.  The runs that touch the block's first and last sample are nobody's pulse yet: they go out with the
                // block's summary, and k_pulses_stitch joins them across blocks behind this kernel.  A lane's samples are read
                // as the statistics form reads them: from the running sums phase 1 staged, or from a second parse.
                const uint32_t base16 = (acc_base + pre_s + incl_s - sum) & 0xffffu;  // the running sum in front of my first sample
                const uint32_t i0 = blk_first + rel0;                                 // its index in the waveform
                const uint32_t fl = pa.neg ? 0xffffu : 0u;
                const uint32_t mw = pa.min_width;
                const bool reparse = wg_any(cnt > kBlkLaneCap);
                auto samples = [&](auto &&take) __attribute__((always_inline)) {  // take(c, v): my sample c as v = y ^ flip
                    if (!reparse) {
                        for (uint32_t i = 0; 2u * i < todo; ++i) {
                            const uint32_t d = my_stage[i];
                            take(2u * i, (int32_t)(int16_t)(uint16_t)((base16 + (d & 0xffffu)) ^ fl));
                            if (2u * i + 1u < todo) take(2u * i + 1u, (int32_t)(int16_t)(uint16_t)((base16 + (d >> 16)) ^ fl));
                        }
                    } else {
                        uint32_t Qr = C - (todo ? f : B0), rs = 0;
                        for (uint32_t c = 0; c < todo; ++c) {
                            const BlkPair p = blk_pair<true>(W, k, Qr);
                            rs += unzigzag(p.z1);
                            Qr += p.nu1;
                            take(c, (int32_t)(int16_t)(uint16_t)((base16 + rs) ^ fl));
                        }
                    }
                };
                // the fast reject, a lane at a time: a packed maximum over its staged pairs says that none of its samples is over
                bool look = todo != 0u;
                if (!reparse && todo != 0u) {
                    typedef short s16x2 __attribute__((ext_vector_type(2)));
                    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
                    const u16x2 b2 = {(uint16_t)base16, (uint16_t)base16};
                    const uint32_t pm = fl | (fl << 16);
                    s16x2 gm = {-32768, -32768};
                    for (uint32_t i = 0; 2u * i < todo; ++i) {
                        uint32_t d = my_stage[i];
                        if (2u * i + 1u >= todo) d = __builtin_amdgcn_perm(d, d, 0x05040504u);  // (my last sample twice: the high half is not mine)
                        const uint32_t v2 = __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, d) + b2)) ^ pm;
                        gm = __builtin_elementwise_max(gm, __builtin_bit_cast(s16x2, v2));
                    }
                    look = (gm.x > gm.y ? (int32_t)gm.x : (int32_t)gm.y) > p_tv;
                }
                // pass 1: my summary
                PulseSeg S = pulse_seg_empty();
                if (look) {
                    samples([&](uint32_t c, int32_t v) __attribute__((always_inline)) { pulse_seg_step(S, v, p_tv, i0 + c, mw); });
                    pulse_seg_finish(S);
                } else {
                    S.n = todo;
                }
                uint64_t *const tab = pa.table + (uint64_t)sidx * kPulseTabWords;
                static_assert(kPulseSegWords <= (int)kPulseTabWords, "a block slot of the table holds a packed summary");
                const bool redo = pa.n_redo != nullptr;  // the second launch: nothing is published, the pulses go to the caller's slots
                const uint32_t first_no = redo ? (uint32_t)tab[kPulseSegWords] : 0u;  // (read only where the block holds a pulse: the stitch wrote it)
                auto publish = [&](const PulseSeg &T) __attribute__((always_inline)) { if (!redo) pulse_seg_pack(T, tab); };
                if (!wg_any((S.lead_w | S.trail_w | S.inner) != 0u)) {
                    // nothing over that matters in the whole block (runs shorter than min_width inside one lane leave no trace)
                    if (tid == 0u) {
                        PulseSeg T = pulse_seg_empty();
                        T.n = blk_count;
                        publish(T);
                    }
                } else {
                    // the scan: inside the wavefront by shuffles, across the wavefronts through s_e (its last reader is a barrier back)
                    // (every lane shuffles, then selects: a shuffle under a condition reads nothing from the lanes the condition leaves out)
                    auto up = [&](const PulseSeg &X, int d) __attribute__((always_inline)) {  // the summary `d` lanes down; the empty one below lane d
                        const bool have = lane >= d;
                        const uint32_t n_ = (uint32_t)__shfl_up((int)X.n, d), inner_ = (uint32_t)__shfl_up((int)X.inner, d);
                        const uint32_t lead_w_ = (uint32_t)__shfl_up((int)X.lead_w, d), trail_w_ = (uint32_t)__shfl_up((int)X.trail_w, d);
                        const uint32_t trail_s_ = (uint32_t)__shfl_up((int)X.trail_s, d);
                        const int64_t lead_key_ = (int64_t)__shfl_up((long long)X.lead_key, d), lead_sum_ = (int64_t)__shfl_up((long long)X.lead_sum, d);
                        const int64_t trail_key_ = (int64_t)__shfl_up((long long)X.trail_key, d), trail_sum_ = (int64_t)__shfl_up((long long)X.trail_sum, d);
                        PulseSeg U;
                        U.n = have ? n_ : 0u;
                        U.inner = have ? inner_ : 0u;
                        U.lead_w = have ? lead_w_ : 0u;
                        U.trail_w = have ? trail_w_ : 0u;
                        U.trail_s = have ? trail_s_ : 0u;
                        U.lead_key = have ? lead_key_ : kPulseNoKey;
                        U.lead_sum = have ? lead_sum_ : (int64_t)0;
                        U.trail_key = have ? trail_key_ : kPulseNoKey;
                        U.trail_sum = have ? trail_sum_ : (int64_t)0;
                        return U;
                    };
                    PulseSeg I = S;
#pragma unroll
                    for (int dd = 0; dd < 6; ++dd) I = pulse_combine(up(I, 1 << dd), I, mw);
                    const PulseSeg E = up(I, 1);  // what lies in front of me as far as my wavefront knows
                    uint64_t *const s_seg = reinterpret_cast<uint64_t *>(s_e);  // [NW][kPulseSegWords]: 56 NW bytes of s_e's 4 NT
                    if (lane == 63) pulse_seg_pack(I, s_seg + kPulseSegWords * wv);
                    blk_barrier();
                    auto wave_total = [&](int w) __attribute__((always_inline)) { return pulse_seg_unpack(s_seg + kPulseSegWords * w); };
                    PulseSeg P = pulse_seg_empty();  // ... and in front of my wavefront
                    for (int w = 0; w < wv; ++w) P = pulse_combine(P, wave_total(w), mw);
                    // the block's summary: the last thread has every wavefront in front of its own, and its own from LDS (of its
                    // own summary S only n, lead_w and inner are needed from here on: fewer registers across pass 2)
                    if (tid == (uint32_t)NT - 1u) publish(pulse_combine(P, wave_total(wv), mw));
                    P = pulse_combine(P, E, mw);
                    // pass 2: the pulses that close among my samples.  None does where every sample of mine is over, or where no
                    // run is open in front of me and my own summary holds none that closed
                    if (todo != 0u && S.lead_w != S.n && (P.trail_w | S.lead_w | S.inner) != 0u) {
                        PulseEmit em = pulse_emit_seed(P);
                        int64_t *const slots = redo ? pa.out + (g * (uint64_t)pa.max_pulses + first_no) * (uint64_t)kPulseRecCols
                                                    : pa.staging + (uint64_t)sidx * pa.cap * (uint64_t)kPulseRecCols;
                        const uint32_t room = redo ? (pa.max_pulses > first_no ? pa.max_pulses - first_no : 0u) : pa.cap;
                        samples([&](uint32_t c, int32_t v) __attribute__((always_inline)) {
                            pulse_emit_step(em, v, p_tv, i0 + c, blk_first, mw,
                                            [&](uint32_t r, uint32_t rs0, uint32_t rw, int64_t key, int64_t rsum) __attribute__((always_inline)) {
                                                if (r < room) pulse_record(slots + (uint64_t)r * kPulseRecCols, rs0, rw, key, rsum, pa.neg != 0u);
                                            });
                        });
                    }
                }
            } else if constexpr (STATS) {
                // ---- phase 2, statistics: every lane reduces its own samples, the block folds the result into the waveform's
                // accumulator.  Everything in front of a lane's first code is exact by now -- its index in the waveform, how many
                // of its codes are samples, the running sum in front of them -- and has to be: samples wrap modulo 2^16, so an
                // extreme taken on relative values and shifted afterwards is wrong.  Nothing is put in output order and no
                // sample leaves the workgroup.
                const uint32_t base16 = (acc_base + pre_s + incl_s - sum) & 0xffffu;  // the running sum in front of my first sample
                const uint32_t i0 = blk_first + rel0;                                 // its index in the waveform
                const uint32_t h = sa.head_len < len ? sa.head_len : len;             // the head window ends in front of sample h
                const uint32_t nh = h > i0 ? ((h - i0 < todo) ? h - i0 : todo) : 0u;  // my samples inside it
                int32_t mn = 0x7fffffff, mx = -0x7fffffff - 1;
                uint32_t amn = 0, amx = 0;
                int32_t s32 = 0, hs32 = 0;  // (a lane holds at most 32 kSegW codes: below 2^25 in magnitude)
                uint64_t sq = 0, hq = 0;
                auto take = [&](uint32_t c, uint32_t rel) __attribute__((always_inline)) {  // my sample c, `rel` behind the base
                    const int32_t v = (int32_t)(int16_t)(uint16_t)(base16 + rel);
                    if (c == nh) { hs32 = s32; hq = sq; }
                    s32 += v;
                    sq += (uint64_t)(uint32_t)(v * v);
                    if (v < mn) { mn = v; amn = c; }  // STRICTLY: the first occurrence stays
                    if (v > mx) { mx = v; amx = c; }
                };
                // the common case: every lane's running sums are complete in its share of the staging buffer, two to a dword
                if (!wg_any(cnt > kBlkLaneCap)) {
                    const uint32_t wmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(todo));
                    for (uint32_t i = 0; 2u * i < wmax; ++i) {
                        const uint32_t d = my_stage[i];
                        if (2u * i < todo) take(2u * i, d & 0xffffu);
                        if (2u * i + 1u < todo) take(2u * i + 1u, d >> 16);
                    }
                } else {
                    // some lane holds more codes than its share (long runs of tiny residuals): every lane parses its codes
                    // again from f, with values, a code at a time
                    uint32_t Qr = C - (todo ? f : B0), rs = 0;
                    for (uint32_t c = 0; c < todo; ++c) {
                        const BlkPair p = blk_pair<true>(W, k, Qr);
                        rs += unzigzag(p.z1);
                        Qr += p.nu1;
                        take(c, rs);
                    }
                }
                if (nh >= todo) { hs32 = s32; hq = sq; }
                // keys that order by value first and by the earliest index second (a waveform has fewer than 2^31 samples)
                int64_t kmin = todo ? (int64_t)(((uint64_t)(uint32_t)mn << 32) | (uint64_t)(i0 + amn)) : INT64_MAX;
                int64_t kmax = todo ? (int64_t)(((uint64_t)(uint32_t)mx << 32) | (uint64_t)(0x7fffffffu - (i0 + amx))) : INT64_MIN;
                uint64_t r_s = (uint64_t)(int64_t)s32, r_hs = (uint64_t)(int64_t)hs32;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const int64_t omin = (int64_t)__shfl_xor((long long)kmin, d), omax = (int64_t)__shfl_xor((long long)kmax, d);
                    kmin = omin < kmin ? omin : kmin;
                    kmax = omax > kmax ? omax : kmax;
                    r_s += (uint64_t)__shfl_xor((unsigned long long)r_s, d);
                    sq += (uint64_t)__shfl_xor((unsigned long long)sq, d);
                    r_hs += (uint64_t)__shfl_xor((unsigned long long)r_hs, d);
                    hq += (uint64_t)__shfl_xor((unsigned long long)hq, d);
                }
                // ... across the wavefronts through s_e (its last reader is two barriers back), then six atomics per block
                uint64_t *const s_red = reinterpret_cast<uint64_t *>(s_e);  // [NW][6]; 48 NW bytes of s_e's 4 NT
                if (lane == 0) {
                    uint64_t *r = s_red + 6 * wv;
                    r[0] = (uint64_t)kmin; r[1] = (uint64_t)kmax; r[2] = r_s; r[3] = sq; r[4] = r_hs; r[5] = hq;
                }
                blk_barrier();
                if (tid == 0 && blk_count != 0u) {
#pragma unroll
                    for (int w = 1; w < NW; ++w) {
                        const uint64_t *r = s_red + 6 * w;
                        kmin = (int64_t)r[0] < kmin ? (int64_t)r[0] : kmin;
                        kmax = (int64_t)r[1] > kmax ? (int64_t)r[1] : kmax;
                        r_s += r[2]; sq += r[3]; r_hs += r[4]; hq += r[5];
                    }
                    unsigned long long *a = sa.acc + 6u * g;
                    __hip_atomic_fetch_min(reinterpret_cast<long long *>(a), (long long)kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_max(reinterpret_cast<long long *>(a + 1), (long long)kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(a + 2, (unsigned long long)r_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(a + 3, (unsigned long long)sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(a + 4, (unsigned long long)r_hs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(a + 5, (unsigned long long)hq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                // ---- phase 2: the samples in output order, whole lines to HBM ----
                // WINDOWS: only where a live window of the waveform meets the block's samples [blk_first, blk_first + blk_count) --
                // the threads test the windows in parallel, the workgroup decides as one.  A block that no window meets puts nothing
                // in order and stores nothing.
                [[maybe_unused]] uint32_t w_live = 0;
                if constexpr (WINDOWS) {
                    w_live = wa.wl.live(g);
                    bool hit = false;
                    for (uint32_t q = tid; q < w_live; q += (uint32_t)NT) {
                        const Win w = window_at(wa.wl.at(g, q), wa.wl.width, len);
                        hit = hit || (w.e > blk_first && w.s < blk_first + blk_count);
                    }
                    if (!wg_any(hit)) {
                        blk_barrier();  // (as at the end of a block: W, the staging buffer and the s_* words are rewritten by the next)
                        continue;
                    }
                }
                // (WINDOWS: the staged samples go to rows of any alignment: staged from element 0)
                const uint32_t a0 = WINDOWS ? 0u : (uint32_t)((((uintptr_t)(y + blk_first)) >> 1) & 7u);  // kOutCap is a multiple of 8: the same every pass
                auto copy_out = [&](uint32_t R0) __attribute__((always_inline)) {  // staged samples [R0, R0 + kOutCap) of the block -> HBM
                    const uint32_t nsamp = (blk_count - R0 < BG::kOutCap) ? blk_count - R0 : BG::kOutCap;
                    if constexpr (WINDOWS) {
                        // ... -> the rows of the windows they lie in: sample x of the waveform sits at obuf[x - lo], and goes to element
                        // x - a of the row of every live window [a, a + width) that holds it.  The destinations come from the
                        // window and `len` alone: a block whose start is later corrected may write wrong values into its own
                        // waveform's rows (the waveform is then listed, and its rows written again), never outside them.
                        const uint32_t lo = blk_first + R0, hi = lo + nsamp;
                        for (uint32_t q = 0; q < w_live; ++q) {
                            const Win w = window_at(wa.wl.at(g, q), wa.wl.width, len);
                            const uint32_t is = w.s > lo ? w.s : lo, ie = w.e < hi ? w.e : hi;
                            if (is >= ie) continue;
                            g_u16 *const rs = (g_u16 *)(wa.wl.row(g, q) + ((int64_t)w.pf - (int64_t)w.s));  // sample x at rs[x]
                            for (uint32_t x = is + tid; x < ie; x += (uint32_t)NT) rs[x] = obuf[x - lo];
                        }
                        return;
                    }
                    g_u16 *gbase = (g_u16 *)(y + blk_first + R0) - a0;  // 16-byte aligned
                    // whole 16-byte pieces [p_lo, p_hi) without a test per piece; the up to seven samples in front of the first and
                    // behind the last one by sixteen lanes
                    const uint32_t end = a0 + nsamp, p_lo = (a0 + 7u) >> 3, p_hi = end >> 3;
                    auto piece = [&](uint32_t p) __attribute__((always_inline)) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(obuf + 8u * p);
                        *(g_uint4 *)(gbase + 8u * p) = (u32x4v){v.x, v.y, v.z, v.w};
                    };
                    uint32_t p = tid;  // (piece p by thread p mod NT: a wavefront's store instruction covers whole aligned lines)
                    if (p >= p_lo && p < p_hi) piece(p);
                    for (p += NT; p < p_hi; p += NT) piece(p);
                    if (tid < 16u) {
                        const uint32_t s = tid < 8u ? tid : 8u * p_hi + (tid - 8u);
                        const bool ok = tid < 8u ? (s >= a0 && s < 8u * p_lo && s < end) : (p_hi >= p_lo && s >= a0 && s < end);
                        if (ok) gbase[s] = obuf[s];
                    }
                };
                // the common case: every lane's codes are all samples of the waveform and fit its share of the staging buffer
                const bool lane_ok = cnt <= kBlkLaneCap && todo == cnt;
                if (!wg_any(!lane_ok)) {
                    constexpr int NR = (int)(kBlkLaneCap / 2u);
                    uint32_t rr[NR];
                    // (pairs beyond the wavefront's largest count are skipped by a scalar branch: 54 of the 76 slots are used on average)
                    const uint32_t wmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(cnt));
#pragma unroll
                    for (int i = 0; i < NR; ++i) {
                        rr[i] = 0;
                        if (2u * (uint32_t)i < wmax) rr[i] = my_stage[i];
                    }
                    if (RESID) s_e[tid] = sum;  // (a lane's last residual: what the next lane puts in front of its first one, below)
                    blk_barrier();  // every lane holds its samples: the buffer may now be rewritten in output order
                    const uint32_t base16 = RESID ? 0u : (acc_base + pre_s + incl_s - sum) & 0xffffu;  // the running sum in front of my first sample
                    // both halves of a dword take the base in one packed add
                    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
                    const u16x2 b2 = {(uint16_t)base16, (uint16_t)base16};
                    uint16_t *const op = obuf + (a0 + rel0);
                    {
                        // WHOLE dwords: a lane whose first sample sits in the high half of a dword (odd position) writes that dword
                        // with the sample in front of its first one in the low half -- which is the running sum in front of it, base16,
                        // whoever decoded it (residual mode: the lane in front's last residual, through s_e) -- and a lane whose last
                        // sample sits in a low half leaves the high half to its successor and stores that sample alone, once (both
                        // stores carry the same value).  38 four-byte stores per lane instead of 76 two-byte ones, at the same three
                        // VALU instructions per pair (add, byte permute, compare).
                        const uint32_t o = a0 + rel0;
                        const bool odd = (o & 1u) != 0u;
                        uint32_t *const dp = reinterpret_cast<uint32_t *>(obuf) + (o >> 1);
                        const uint32_t sel = odd ? 0x05040302u : 0x07060504u;  // odd: (prev.hi, cur.lo); even: cur
                        const uint32_t lim = cnt == 0u ? 0u : (odd ? cnt : cnt - 1u);  // dword j is written if 2 j < lim
                        uint32_t prevp = RESID ? (tid ? s_e[tid - 1u] << 16 : 0u) : __builtin_bit_cast(uint32_t, b2);
#pragma unroll
                        for (int i = 0; i < NR; ++i) {
                            if (2u * (uint32_t)i < wmax) {
                                const uint32_t cur = __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, rr[i]) + b2));
                                const uint32_t d = __builtin_amdgcn_perm(cur, prevp, sel);
                                if (2u * (uint32_t)i < lim) dp[i] = d;
                                prevp = cur;
                            }
                        }
                        if (cnt != 0u) op[cnt - 1u] = (uint16_t)(base16 + sum);  // (my last sample = the running sum behind my codes; residual mode: my last residual)
                    }
                    blk_barrier();
                    if (FUSE) iir_lds(a0, blk_count);
                    copy_out(0u);
                } else {
                    // some lane holds more codes than its share (long runs of tiny residuals), or codes past the waveform's
                    // last sample (a corrupt stream): decode again from f, in as many staging passes as the block needs
                    uint32_t c = 0, acc = acc_base + pre_s + incl_s - sum;
                    Qp = C - (todo ? f : B0);
                    for (uint32_t R0 = 0; R0 < blk_count; R0 += BG::kOutCap) {
                        // my samples with block-relative index below R0 + kOutCap
                        const uint32_t cmax = (rel0 >= R0 + BG::kOutCap) ? 0u : ((todo < R0 + BG::kOutCap - rel0) ? todo : R0 + BG::kOutCap - rel0);
                        // slot of sample c: a0 + rel0 + c - R0 (>= a0 for every c this pass decodes)
                        uint16_t *outp = obuf + (int32_t)(a0 + rel0 - R0);
                        blk_parse<kBlkValue, RESID>(W, k, c < cmax, Qp, 0u, c, acc, cmax, outp);
                        blk_barrier();
                        if (FUSE) iir_lds(a0, (blk_count - R0 < BG::kOutCap) ? blk_count - R0 : BG::kOutCap);
                        copy_out(R0);
                        blk_barrier();
                    }
                }
                if (FUSE && last_of_run && tid == 0u)
                    __hip_atomic_store(xstate + sidx, (1ull << 63) | (uint64_t)(xs.x & 0xffffu) | ((uint64_t)(xs.y & 0xffffu) << 16) | ((uint64_t)(xs.z & 0xffffu) << 32),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            blk_barrier();  // W, the staging buffer and the s_* words are rewritten by the next block
        }
        if (next_unit >= total_units) return;
        unit = next_unit;
        cur = nxt;
    }
