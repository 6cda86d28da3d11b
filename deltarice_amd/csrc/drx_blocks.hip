// drx_blocks.hip -- block-parallel decoder: a WORKGROUP per block of a waveform's stream.
//
// The lane-per-waveform decoder (k_decode_lanes, drx_decode_kernels.hip) needs ~10^5 waveforms to fill an MI355X.  The
// reference's own shapes often have far fewer: its default options make every chunk ONE waveform
// (src/deltaRice.c:249-258), nEDM / NOPTREX chunks are 32 waveforms of 81 920 / 500 000 samples
// (docs/Performance.md:27,38), and one H5Z call on the README's example chunk sees 20 waveforms
// (README.md:75-82).  Here the parallelism comes from inside the waveform -- what north_star calls a wavefront per
// waveform, in the only form the format permits: the Rice parse is serial (code boundaries are data dependent,
// src/deltaRice.c:155-171, and the format has no index), but it SELF-SYNCHRONISES: a parse started at an arbitrary
// bit falls into step with the true code boundaries within a few codes.
//
//   block     kWords = NT x 13 words of one waveform's payload, in LDS, reversed word order (word 0 on top) so that
//             with the bit position kept as Qp = C - P the word pair of a 32-bit window is (Qp >> 5, Qp >> 5 + 1) and
//             v_alignbit(hi, lo, Qp) is the window, also on a word boundary.  13 words per lane: an odd stride keeps the
//             NT lanes on different LDS banks while they read the same word of their segments.
//   phase 1   lane j runs up through the kBlkGuessBits in front of its segment from an ASSUMED code boundary, notes
//             the first code that starts inside its segment (f_j), then counts codes and sums residuals up to the
//             first code that starts behind it (e_j).  If lane j-1 was in step, e_{j-1} == f_j; lane 0 of block 0
//             starts exactly, so the chain of equalities proves every lane exact.  A lane whose start does not
//             match its predecessor's end restarts from that end until nothing changes (once in a blue moon for
//             noise; a slope-1 ramp, whose codes all have the same length, never falls into step and takes up to NT
//             rounds -- correct, just slow).
//   blocks    lane 0 of block b > 0 checks its f_0 against the end block b-1 published after ITS phase 1 (one hop, no
//             chain); samples and the running sum in front of a block come from a decoupled look-back over the
//             blocks of the waveform ({status | count | sum} entries, tickets as in the encoder).  A block that has to
//             correct its start after it published its end flags the waveform; flagged waveforms are decoded again
//             by the one-workgroup-per-waveform kernel (drx_decode_kernels.hip), which is also the one that judges them.
//   phase 2   phase 1 has left every lane's running sums (relative to its first code) in LDS, lane-major; once the
//             prefix sums over counts and sums are known each lane reads its own into registers, adds its base and
//             writes them to the same buffer in OUTPUT order; the block then copies whole aligned 128-byte lines to
//             HBM.  (Scattered 2- and 8-byte stores of the previous long-waveform kernel cost 2.5-5.4 x the output
//             size in HBM writes: profiles/r02_*_pmc_traffic.json.)  A block in which some lane holds more codes than
//             its share of the buffer (kBlkLaneCap; long runs of tiny residuals) decodes a second time instead, in
//             as many staging passes as it needs.
// 1.4 parses of every bit in the common case, no iteration, no sample ever stored twice.
// Delta filter only: the prefix sum over residual sums is what makes blocks independent.
#include "drx_blocks.h"

namespace drx {

// Most blocks any waveform of the batch has: info[0]; tickets of the decode launch: info[1] = info[0] x waveforms.
// One workgroup.
// (list: the waveforms of this launch, nullptr = all of them in order)
__global__ __launch_bounds__(1024) void k_blk_max(uint64_t total_waves, const uint32_t *__restrict__ wave_words,
                                                  uint32_t words_per_block, uint32_t *__restrict__ info,
                                                  const uint32_t *__restrict__ list) {
    __shared__ uint32_t wmax[16];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    uint32_t m = 0;
    for (uint64_t i = threadIdx.x; i < total_waves; i += 1024) {
        const uint32_t v = (wave_words[list ? list[i] : i] + words_per_block - 1u) / words_per_block;
        m = v > m ? v : m;
    }
    m = wave_max_u32(m);
    if (lane == 0) wmax[wv] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = wmax[w] > m ? wmax[w] : m;
        info[0] = m;
        const uint64_t t = (uint64_t)m * total_waves;
        info[1] = t > 0xffffffffull ? 0xffffffffu : (uint32_t)t;
    }
}

// The parse and the kernel's body are drx_blocks.h's (drx_blocks_body.inc: shared with k_stats_blocks, drx_stats_blocks.hip).
// (The order of the last arguments is part of the code: `out`, `wave_list` and the filter's tables are loaded on entry, the
// compiler merges adjacent ones into one wider scalar load, and another merge moves this kernel's SGPR spills.)
template <int NT, bool RESID, int SW, bool FUSE = false>
__global__ __launch_bounds__(NT) void k_decode_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words,
                                                      const uint32_t *__restrict__ info, uint32_t slots_per_wave,
                                                      uint32_t run_len, uint64_t *__restrict__ state,
                                                      uint32_t *__restrict__ ends, uint32_t *__restrict__ ticket,
                                                      uint32_t *__restrict__ fail, uint32_t *__restrict__ suspect,
                                                      DevStatus *st, int16_t *__restrict__ out, uint32_t n_list,
                                                      const uint32_t *__restrict__ itab, uint64_t *__restrict__ xstate,
                                                      const uint32_t *__restrict__ wave_list) {
    constexpr bool STATS = false, PULSES = false, WINDOWS = false, TRANSCODE = false, BINS = false;
    const BlkStatsArgs sa{0u, nullptr};
    const BlkPulseArgs pa{};
    const BlkWindowArgs wa{};
    const BlkTrcArgs ta{};
    const BlkBinsArgs ba{};
#include "drx_blocks_body.inc"
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int blocks_nt(const Geom &G) { return G.uniform ? nt_for_len(G.u_wave_len, G.k) : (int)G.rag_blk_nt; }

// blocks of `waves` waveforms of `wave_len` samples, weighted by what a block of theirs costs (1.7 for waveforms of one or two
// blocks: they pay the ticket's dependent loads -- ticket, table entry, image -- per block: 36 us measured at 256 lanes, 10
// chunks of 1166 x 12 000 and of 854 x 16 384)
static double blocks_weighted(uint64_t waves, uint32_t wave_len, uint32_t k, int nt) {
    const uint64_t typ_words = ((uint64_t)wave_len * (2u * k + 7u)) >> 6;
    const uint64_t bpw = (typ_words + blk_words((uint32_t)nt, k) - 1u) / blk_words((uint32_t)nt, k);
    return (double)(waves * bpw) * (bpw <= 2u ? 1.7 : 1.0);
}
static double blocks_us_of(double weighted_blocks, int nt, uint32_t k) {
    const double resident = nt == 256 ? 768.0 : (nt == 128 ? 1536.0 : 3072.0);
    // (measured with 11 words per lane; a block's time goes with its bits)
    const double t_blk = (nt == 256 ? 21.0 : (nt == 128 ? 28.0 : 41.0)) * (double)blk_segw_plan(k) / 11.0;
    return (double)(uint64_t)((weighted_blocks + resident - 1.0) / resident) * t_blk;  // whole rounds of the resident grid
}

// Which batches take this decoder: the delta filter or a general filter the fast kernels take (its inverse then runs in place
// behind this decoder, drx_iir.hip), waveforms of at least 2048 samples, and cheaper here than a lane per waveform.  The two
// costs (tools/len_sweep.py, profiles/r02_blocks_vs_lanes.txt, r02_len_sweep_*): a lane decodes ~17 samples per microsecond
// whatever else runs, so k_decode_lanes takes ~60 ns x WaveformLength per 98 304 waveforms; a block costs a workgroup 21 /
// 28 / 41 us at 256 / 128 / 64 lanes, full or not, with 768 / 1536 / 3072 workgroups resident.  (Round 2's first rule, "at
// most 24 576 waveforms", sent 25 chunks of 854 x 16 384 here: two blocks per waveform, the second a fifth full, 1.46 ms
// where the lane kernel takes 0.98.)  Ragged batches: decided once from the host's chunk table, blocks_plan_ragged().
// lane_us: what the lane-per-waveform kernel the caller would run instead takes per sample (the decoder's 0.06; drx_wave_stats' 0.052)
bool blocks_batch(const Geom &G, double lane_us, bool any_filter) {
    if (!any_filter && G.n_taps != 0 && !G.fast_taps) return false;
    if (!G.uniform) return G.rag_blocks != 0;
    if (!(G.total_waves <= 98304u && G.u_wave_len >= 2048u)) return false;
    const int nt = blocks_nt(G);
    const uint64_t typ_words = ((uint64_t)G.u_wave_len * (2u * G.k + 7u)) >> 6;
    const uint64_t bpw = (typ_words + blk_words((uint32_t)nt, G.k) - 1u) / blk_words((uint32_t)nt, G.k);
    const double blocks_us = blocks_us_of((double)(G.total_waves * bpw), nt, G.k) * (bpw <= 2u ? 1.7 : 1.0);
    const double lanes_us = lane_us * (double)G.u_wave_len * (double)((G.total_waves + 98303u) / 98304u);
    return blocks_us < lanes_us;
}

std::vector<uint32_t> blocks_plan_ragged(Geom &G, const ChunkDesc *d) {
    G.rag_blocks = 0;
    G.rag_blk_classes = 0;
    uint32_t max_len = 0, min_len = 0xffffffffu;
    for (uint64_t c = 0; c < G.n_chunks; ++c) {
        max_len = d[c].wave_len > max_len ? d[c].wave_len : max_len;
        min_len = d[c].wave_len < min_len ? d[c].wave_len : min_len;
    }
    if (G.total_waves > 98304u || min_len < 2048u) return {};
    const int nt = nt_for_len(max_len, G.k);
    double wb = 0;
    for (uint64_t c = 0; c < G.n_chunks; ++c) wb += blocks_weighted(d[c].n_waves, d[c].wave_len, G.k, nt);
    // a lane takes 60 ns per sample: a lane-per-waveform launch lasts as long as its longest waveform, per 98 304 of them
    const double lanes_us = 0.06 * (double)max_len * (double)((G.total_waves + 98303u) / 98304u);
    if (!(blocks_us_of(wb, nt, G.k) < lanes_us)) return {};
    // look-back slots per waveform: enough for the longest one at 25 bits per sample, in blocks of the SMALLEST class's size
    const uint64_t per = (max_payload_words(max_len) + blk_words_min(64u) - 1u) / blk_words_min(64u);
    if (G.total_waves * per * 12u > (1ull << 30)) return {};  // (one very long waveform among very many: the table would not pay)
    G.rag_blocks = 1u;
    G.rag_blk_nt = (uint32_t)nt;
    G.rag_blk_slots = (uint32_t)(per ? per : 1u);
    // classes by floor(log2 WaveformLength), longest first (the long classes start while the grid is empty)
    std::vector<uint32_t> list(G.total_waves);
    uint32_t n_cls = 0, at = 0;
    for (int b = 31; b >= 11; --b) {
        uint32_t cnt = 0, cls_max = 0;
        for (uint64_t c = 0; c < G.n_chunks; ++c) {
            if ((31 - __builtin_clz(d[c].wave_len)) != b) continue;
            for (uint32_t i = 0; i < d[c].n_waves; ++i) list[at + cnt++] = (uint32_t)(d[c].wave_base + i);
            cls_max = d[c].wave_len > cls_max ? d[c].wave_len : cls_max;
        }
        if (!cnt) continue;
        G.rag_blk_class_off[n_cls] = at;
        G.rag_blk_class_len[n_cls] = cls_max;
        at += cnt;
        ++n_cls;
    }
    G.rag_blk_class_off[n_cls] = at;
    G.rag_blk_classes = n_cls;
    return list;
}

// the fused inverse filter's tables: one set per lane share (76, 68, 60 samples), kRunTabWords each
uint32_t blocks_iir_tab_words() { return 3u * kRunTabWords; }
void blocks_iir_tables(const uint32_t fast_nt[3], uint32_t t0neg, uint32_t *tab) {
    iir_run_tables(fast_nt, t0neg, 76u, tab);
    iir_run_tables(fast_nt, t0neg, 68u, tab + kRunTabWords);
    iir_run_tables(fast_nt, t0neg, 60u, tab + 2u * kRunTabWords);
}

static uint32_t blocks_slots_per_wave(const Geom &G) {  // blocks of a waveform at 25 bits per sample
    if (!G.uniform) return G.rag_blk_slots;
    const uint64_t per = (max_payload_words(G.u_wave_len) + blk_words_min(blocks_nt(G)) - 1u) / blk_words_min(blocks_nt(G));
    return (uint32_t)(per ? per : 1u);
}

// scratch: u32 info[32][4] | u32 fail[W] | u32 suspect[W] | u32 ticket[1] (+ pad to 16 bytes) | u32 ends[slots] | u64 state[slots] | u64 xstate[slots]
struct BlkScratch {
    uint32_t *info, *fail, *suspect, *ticket, *ends;
    uint64_t *state, *xstate;  // xstate: the inverse filter's state behind every block slot (FUSE)
    uint64_t bytes;
};
static BlkScratch blocks_layout(const Geom &G, void *base) {
    const uint64_t W = G.total_waves, U = W * blocks_slots_per_wave(G);
    uint64_t n32 = 4u * kBlkMaxClasses + W + W + 1u;  // info[class][4]: {most blocks of a waveform, tickets, the class's ticket word, -}
    n32 = (n32 + 3u) & ~3ull;
    BlkScratch L;
    uint32_t *p = reinterpret_cast<uint32_t *>(base);
    L.info = p;
    L.fail = p + 4u * kBlkMaxClasses;
    L.suspect = L.fail + W;
    L.ticket = L.suspect + W;
    L.ends = p + n32;
    const uint64_t ends32 = (U + 1u) & ~1ull;
    L.state = reinterpret_cast<uint64_t *>(L.ends + ends32);
    L.xstate = L.state + U;
    L.bytes = (n32 + ends32) * 4u + 2u * U * 8u;
    return L;
}

uint64_t blocks_scratch_bytes(const Geom &G) { return blocks_batch(G) ? blocks_layout(G, nullptr).bytes : 0; }
uint64_t blocks_total_slots(const Geom &G) { return G.total_waves * blocks_slots_per_wave(G); }

static unsigned blk_resident(int nt) { return 256u * (nt == 64 ? 12u : (nt == 128 ? 6u : 3u)); }  // workgroups per CU by LDS: 50 dwords per lane in every class
// the block geometry of a call: by the stream's bits per sample as the caller states them (a wrong in_words costs speed, nothing else)
static uint64_t blk_bits10(const Geom &G, uint64_t in_words) { return G.total_samples ? 320ull * in_words / G.total_samples : 65ull; }

// What a call of the scheme begins with: the scratch, reset on the stream, and the geometry the stream's bits per sample choose
struct BlkCall {
    BlkScratch L;
    uint32_t spw;  // look-back slots per waveform
    uint64_t b10;
    int sw;
};
static hipError_t blk_call_begin(const Geom &G, uint64_t in_words, void *d_blk, hipStream_t s, BlkCall *B) {
    B->L = blocks_layout(G, d_blk);
    B->spw = blocks_slots_per_wave(G);
    B->b10 = blk_bits10(G, in_words);
    B->sw = blk_segw_bits10(B->b10);
    return hipMemsetAsync(d_blk, 0, B->L.bytes, s);
}
// The launches of the scheme for a batch: one for a uniform batch, one per length class of a ragged one, with the lanes per
// block that suit the class's longest WaveformLength.  Returns their number (at most kBlkMaxClasses)
struct BlkClass {
    const uint32_t *list;  // the launch's waveforms (nullptr: all of the batch)
    uint32_t n_waves;
    int nt;
    uint32_t wave_len;
};
static uint32_t blk_classes(const Geom &G, BlkClass *cls) {
    if (G.uniform) {
        cls[0] = BlkClass{nullptr, (uint32_t)G.total_waves, blocks_nt(G), G.u_wave_len};
        return 1u;
    }
    for (uint32_t c = 0; c < G.rag_blk_classes; ++c)
        cls[c] = BlkClass{G.rag_blk_list + G.rag_blk_class_off[c], G.rag_blk_class_off[c + 1] - G.rag_blk_class_off[c],
                          nt_for_len(G.rag_blk_class_len[c], G.k), G.rag_blk_class_len[c]};
    return G.rag_blk_classes;
}

// One launch of a kernel of this scheme, class `cls` of the batch at `nt` lanes per block: k_blk_max for its info words, the run
// length and the resident grid.
static BlkClassLaunch blk_class_launch(const BlkCall &B, uint32_t cls, const BlkClass &k, int nt, const uint32_t *d_wave_words, hipStream_t s) {
    BlkClassLaunch c;
    c.info = B.L.info + 4u * cls;
    c.list = k.list;
    c.n_waves = k.n_waves;
    c.nt = nt;
    c.sw = B.sw;
    c.spw = B.spw;
    const uint32_t words_per_block = (uint32_t)nt * (uint32_t)B.sw;
    k_blk_max<<<1, 1024, 0, s>>>(k.n_waves, d_wave_words, words_per_block, c.info, k.list);
    const uint64_t units = (uint64_t)k.n_waves * B.spw;
    // Runs of several blocks only when two runs of one waveform are RARELY in flight together (see the kernel): at least
    // as many waveforms as resident workgroups.  (Ticket order does not exclude it -- a slow workgroup holding ticket t may
    // still run when ticket t + n_waves is drawn; the later run's look-back then simply waits on the lower ticket.)  Then as long as the launch keeps kBlkRounds tickets per workgroup (the
    // tail of the last round), up to the whole waveform: only a run's first block waits for other workgroups (nEDM, 6
    // blocks per waveform: one run; NOPTREX, 36: three runs of 12: 1.40 / 0.98 ms against 1.43 / 1.00 with round 2's fixed 4).
    const uint32_t resident = blk_resident(nt);
    const uint64_t typ_words = ((uint64_t)k.wave_len * B.b10) / 320u;
    const uint64_t bpw = (typ_words + words_per_block - 1u) / words_per_block;
    uint64_t rl = ((uint64_t)k.n_waves * bpw) / ((uint64_t)kBlkRounds * resident);
    rl = rl > bpw ? bpw : rl;
    c.run_len = k.n_waves >= resident ? (uint32_t)(rl < 1u ? 1u : rl) : 1u;
    c.grid = (unsigned)(units < resident ? units : resident);  // resident: never more workgroups than there are units
    return c;
}

// The delta filter's launches for another kernel of the scheme (k_stats_blocks): the scratch reset on the stream, as
// launch_decode_blocks() does, and one BlkClassLaunch per launch
hipError_t blocks_prepare(const Geom &G, uint64_t in_words, const uint32_t *d_wave_words, void *d_blk, hipStream_t s, BlkTables *T,
                          BlkClassLaunch *launches, uint32_t *n_launches) {
    BlkCall B;
    const hipError_t e = blk_call_begin(G, in_words, d_blk, s, &B);
    if (e != hipSuccess) return e;
    *T = BlkTables{B.L.fail, B.L.suspect, B.L.ends, B.L.state};
    BlkClass cls[kBlkMaxClasses];
    *n_launches = blk_classes(G, cls);
    for (uint32_t i = 0; i < *n_launches; ++i) launches[i] = blk_class_launch(B, i, cls[i], cls[i].nt, d_wave_words, s);
    return hipGetLastError();
}

// Which batches take a call's block form, and the call's form word (drx_internal.h)
bool blocks_form_batch(const Geom &G, const void *d_blk, const BlkFormRule &r) {
    if ((G.n_taps != 0 && !r.any_filter) || !d_blk || !blocks_batch(G, r.lane_us, r.any_filter)) return false;
    return !(G.dbg & (DRX_DBG_NO_LONG_PATHS | DRX_DBG_LONG_NOT_BLOCKS | r.lanes_flag));
}
uint32_t blocks_form_word(const Geom &G, bool blocks, const BlkFormRule &r) {
    return blocks ? (DRX_STATS_FORM_BLOCKS | ((G.dbg & r.all_fallback_flag) ? DRX_STATS_FORM_FALLBACK_ALL : 0u)) : DRX_STATS_FORM_LANES;
}

hipError_t launch_decode_blocks(const StreamCall &call, void *d_blk, int16_t *d_out, const uint32_t **fail_out,
                                const uint32_t **suspect_out, bool resid, bool *fused_out) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    BlkCall B;
    const hipError_t e = blk_call_begin(G, call.in_words, d_blk, s, &B);
    if (e != hipSuccess) return e;
    const BlkScratch &L = B.L;
    BlkClass cls[kBlkMaxClasses];
    const uint32_t n_cls = blk_classes(G, cls);
    // General filters: the inverse filter inside this kernel (FUSE) where its state can pass from a run's last block to the next
    // run's first without a chain of waits, i.e. where every launch has at least as many waveforms as resident workgroups (the
    // condition under which runs are longer than one block); else residuals now and k_iir_tiles behind (DRX_DBG_IIR_SEPARATE: always).
    // (General filters run at 128 or 256 lanes per block when fused and at 256 when not: 12 of the 36 instantiations of the
    // kernel are not built; a block larger than the class's choice costs short waveforms some empty lanes, nothing else.)
    auto nt_gen = [](int nt) { return nt < 128 ? 128 : nt; };
    bool fuse = resid && G.blk_iir_tab != nullptr && !(G.dbg & DRX_DBG_IIR_SEPARATE);
    for (uint32_t i = 0; i < n_cls; ++i) fuse = fuse && cls[i].n_waves >= blk_resident(nt_gen(cls[i].nt));
    if (fused_out) *fused_out = fuse;
    for (uint32_t i = 0; i < n_cls; ++i) {
        // (k_blk_max of a class immediately in front of the class's kernel)
        const BlkClassLaunch c = blk_class_launch(B, i, cls[i], resid ? (fuse ? nt_gen(cls[i].nt) : 256) : cls[i].nt, call.d_wave_words, s);
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            auto go = [&](auto mode_tag) {
                constexpr int MODE = decltype(mode_tag)::value;  // 0 delta filter, 1 residuals (k_iir_tiles follows), 2 inverse filter fused
                // the filter's tables for runs of this geometry's lane share (76 / 68 / 60 samples)
                const uint32_t *itab = G.blk_iir_tab ? G.blk_iir_tab + kRunTabWords * (blk_lane_cap(SW) == 76u ? 0u : (blk_lane_cap(SW) == 68u ? 1u : 2u)) : nullptr;
                k_decode_blocks<NT, MODE != 0, SW, MODE == 2><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw,
                                                                                 c.run_len, L.state, L.ends, c.info + 2, L.fail, L.suspect, call.d_status, d_out,
                                                                                 c.n_waves, itab, L.xstate, c.list);
            };
            // the combinations that cannot occur (see nt_gen above) are not instantiated
            if (fuse) { if constexpr (NT >= 128) go(std::integral_constant<int, 2>{}); }
            else if (resid) { if constexpr (NT == 256) go(std::integral_constant<int, 1>{}); }
            else go(std::integral_constant<int, 0>{});
        });
    }
    *fail_out = L.fail;
    *suspect_out = L.suspect;
    return hipGetLastError();
}

}  // namespace drx
