// drx_decode_kernels.hip -- gfx950 (MI355X, CDNA4) DECODE kernels of the Delta-Rice codec, the decode launch and its dispatch
// (the header walk in front of them: drx_walk.hip, its in-launch walkers: drx_walk.h; few long waveforms: drx_blocks.hip,
// general filters behind it: drx_iir.hip; selected waveforms: drx_select.hip).
//
// Format contract (bit-exact with /root/reference/src/deltaRice.c):
//   chunk   := u32 N | { u32 n_i | u32 payload_i[n_i] }            (:415,379,427-433)
//   payload := MSB-first concatenation of one code per sample      (:229-241)
//   code(z) := (z>>k) zeros, '1', k bits      if (z>>k) < 8        (:215-222)
//              8 zeros, '1', 16 bits of z     otherwise            (:223-228)
//   z = zigzag(d), d_0 = x_0, d_j = x_j - x_{j-1} mod 2^16         (:51-63,207-211)
//
//
// The Rice parse is serial inside a waveform, so the unit of parallelism is the waveform: one lane per waveform, 64
// waveforms per wavefront; the 64 compressed streams are staged into per-lane LDS rings and the decoded samples are
// transposed through LDS so that HBM sees 16-byte stores of whole 128-byte lines per waveform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_walk.h"

namespace drx {

// Straightforward lane-per-waveform decoder: global loads and 2-byte stores.
// Kept as the simple cross-check of the staged kernel below (decode_impl = 0).
__global__ __launch_bounds__(64) void k_decode_simple(Geom G, const uint32_t *__restrict__ in,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words, DevStatus *st,
                                                      int16_t *__restrict__ out, const uint32_t *__restrict__ only) {
    const uint64_t g = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (g >= G.total_waves) return;
    if (only && !only[g]) return;  // (behind the block decoder with a general filter: the waveforms it flagged)
    const WaveRef r = locate(G, g);
    const uint32_t *s = in + wave_off[g] + 1;
    const uint32_t n = wave_words[g];
    int16_t *y = out + r.sample_off;
    int16_t hist[64];  // general prediction filters only (lives in scratch; the delta path never touches it)
    const uint64_t words = serial_wave(G, s, n, r.len, hist, 1u, [&](uint32_t i, int16_t v) __attribute__((always_inline)) { y[i] = v; });
    // a valid waveform's codes end in its last payload word: n_i = ceil(bits / 32) (src/deltaRice.c:237-241)
    if (r.len && words != n) atomicOr(&st->err, kErrCorrupt);
}

// Decoder for FEW, LONG waveforms (WaveformLength = -1, the reference's default, makes every chunk one
// waveform of millions of samples): one WORKGROUP of 8 wavefronts per waveform, its 512 lanes parse 512
// consecutive 512-bit segments of the stream at once.  A lane does not know where the first code of its segment
// starts; it assumes the segment start, parses to the end of its segment and reports where its last
// code ended.  Rice codes re-synchronise within a few codes, so that end is almost always right even
// when the start was not.  Each lane then restarts from its predecessor's end until no start changes
// (lane 0's start is known, so after at most 512 rounds every lane is exact; typically one restart),
// the sample counts and delta sums of the segments are prefix-summed over the workgroup, and a last parse
// writes the samples.  Three parses of every bit instead of one, 512 at a time.  Delta filter only (the
// prefix sum over segment sums is what makes the segments independent).
constexpr int kLongSeg = 16;  // words per lane and block
constexpr int kLongOv = 2;    // words of the next segment kept below a lane's column (a code has <= 25 bits)
constexpr uint32_t kLongSegBits = kLongSeg * 32u;
constexpr int kLongWaves = 8;                 // wavefronts per workgroup
constexpr int kLongThreads = 64 * kLongWaves;  // segments parsed at once
constexpr uint32_t kLongGuessBits = 160;  // bits in front of a segment's end from which the first guess is parsed

// One workgroup per waveform walks its blocks in order (fail != nullptr: only the waveforms it flags).  This is the
// FALLBACK of the block-parallel decoder (drx_blocks.hip), which gives every block a workgroup of its own and is 2-6 x
// faster where a parse falls into step within a few codes; waveforms where that fails (a slope-1 ramp: all codes the same
// length) are flagged and come here, where a block starts exactly where its predecessor ended.  (The workgroup-per-block
// form of THIS kernel, with a tail parse predicting block starts, was round 1's path for a handful of long waveforms; the
// new decoder replaced it: 25 x 14 M samples 1.55 -> 0.83 ms, profiles/r02_notes.md.)
__global__ __launch_bounds__(kLongThreads) void k_decode_long(Geom G, const uint32_t *__restrict__ in,
                                                              const uint64_t *__restrict__ wave_off,
                                                              const uint32_t *__restrict__ wave_words, DevStatus *st,
                                                              int16_t *__restrict__ out, const uint32_t *__restrict__ fail,
                                                              const uint32_t *__restrict__ suspect, uint32_t verdict_only) {
    constexpr uint32_t NT = kLongThreads;
    // [kLongRows - 2 - word of the segment][thread] (a lane's bank is its lane number whatever row it reads), rows
    // in REVERSE word order plus one unused row on top: with the bit position kept negated, Q = -pos, the row
    // pair (Q >> 5, Q >> 5 + 1) is (word w + 1, word w) inside a word and (word w, word w - 1) on a word
    // boundary, and v_alignbit_b32(hi, lo, Q) is the 32-bit window in both cases (as in k_decode_lanes)
    // (+ 2 rows below: a lane that has left its segment keeps reading at its last position, up to 49 bits past it)
    constexpr uint32_t kLongRows = kLongSeg + kLongOv + 3;
    __shared__ uint32_t col[kLongRows * NT];
    __shared__ uint32_t s_end[NT];
    __shared__ uint32_t s_tot[2][kLongWaves];
    const uint32_t tid = threadIdx.x;
    const int wv = (int)(tid >> 6), lane = (int)(tid & 63u);
    const uint64_t g = blockIdx.x;
    if (g >= G.total_waves) return;
    if (fail && !fail[g]) {
        // not flagged: the block-parallel decoder's output stands, and so does its verdict on the stream
        if (suspect && suspect[g] && tid == 0) atomicOr(&st->err, kErrCorrupt);
        return;
    }
    if (verdict_only) return;  // (general filters: flagged waveforms are decoded again by k_decode_simple, which judges them too)
    const WaveRef r = locate(G, g);
    const uint32_t *src = in + wave_off[g] + 1;
    const uint32_t n = wave_words[g];
    int16_t *y = out + r.sample_off;
    const uint32_t len = r.len, k = G.k;
    uint32_t blk_word = 0;  // first word of the block
    uint32_t carry_in = 0;  // bit of thread 0's segment at which the next code starts
    uint32_t done = 0;      // samples written
    uint32_t acc_base = 0;  // running sum before the block (mod 2^16)

    // parses this thread's segment from bit `start`; a code is taken when it STARTS inside the segment and inside
    // the stream.  emit: add to the running sum `acc` and store sample number idx, idx + 1, ...
    auto parse = [&](bool enable, uint32_t start, uint32_t avail_bits, auto emit_tag, uint32_t idx, uint32_t acc,
                     uint32_t &end, uint32_t &cnt, uint32_t &sum) __attribute__((always_inline)) {
        constexpr bool EMIT = decltype(emit_tag)::value;
        uint32_t c = 0, sacc = EMIT ? acc : 0u;
        uint32_t Q = 0u - start;  // minus the bit position
        const uint32_t lim = avail_bits < kLongSegBits ? avail_bits : kLongSegBits;
        const int32_t nlim = enable ? -(int32_t)lim : 1;  // a code is taken while -Q < lim, i.e. Q > -lim
        // EMIT: two samples per store where they fill an aligned dword (2-byte stores run into the L2's request rate)
        const uint32_t par4 = (uint32_t)(((uintptr_t)y >> 1) & 1u);  // sample 0's half of its aligned dword
        uint32_t held = 0, held_i = 0;  // the sample waiting for its partner
        bool holding = false;
        // LDS byte address of this thread's row of word 0
        const uint32_t row0 = lds_addr(col) + ((kLongRows - 2u) * NT + tid) * 4u;
        while (__any((int32_t)Q > nlim)) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // one vote per four codes
                const bool act = (int32_t)Q > nlim;
                typedef const uint32_t __attribute__((address_space(3))) lds_cu32;
                const lds_cu32 *wp = (const lds_cu32 *)(uintptr_t)(row0 + (uint32_t)(((int32_t)Q >> 5) * (int32_t)(NT * 4u)));
                const uint32_t lo = wp[0], hi = wp[NT];
                const uint32_t win = __builtin_amdgcn_alignbit(hi, lo, Q);
                const uint32_t q = ffbh(win);  // all-zero window (padding): the hardware's -1 is as good as any
                const uint32_t kk = (win < (1u << 24)) ? 16u : k;
                const uint32_t nu = ~(q + kk);  // minus the code length
                const uint32_t z = (q << kk) + __builtin_amdgcn_ubfe(win, nu, kk);
                const uint32_t d = (z >> 1) ^ (0u - (z & 1u));
                const uint32_t s2 = sacc + d;
                if (EMIT) {
                    if (act && idx + c < len) {
                        const uint32_t i = idx + c;
                        if (((i + par4) & 1u) == 0u) {  // low half of an aligned dword: wait for the next sample
                            held = s2 & 0xffffu;
                            held_i = i;
                            holding = true;
                        } else if (holding) {
                            *reinterpret_cast<uint32_t *>(y + i - 1u) = held | (s2 << 16);
                            holding = false;
                        } else {
                            y[i] = (int16_t)(uint16_t)s2;  // the lane's first sample sits in a high half
                        }
                    }
                }
                sacc = act ? s2 : sacc;
                Q = act ? Q + nu : Q;
                c += act ? 1u : 0u;
            }
        }
        if (EMIT && holding) y[held_i] = (int16_t)(uint16_t)held;  // the lane's last sample had no partner
        const uint32_t pos = 0u - Q;
        end = pos;
        cnt = c;
        sum = sacc;
    };

    while (done < len && blk_word < n) {
        // the block's words, transposed into per-thread columns; the first kLongOv words of segment s + 1 repeat below column s
#pragma unroll
        for (int rr = 0; rr < kLongSeg; ++rr) {
            const uint32_t j = tid + NT * (uint32_t)rr;
            const uint32_t wvl = (blk_word + j < n) ? src[blk_word + j] : 0u;
            const uint32_t sgm = j / kLongSeg, i = j % kLongSeg;
            col[(kLongRows - 2u - i) * NT + sgm] = wvl;
            if (i < (uint32_t)kLongOv && sgm >= 1u) col[(kLongRows - 2u - ((uint32_t)kLongSeg + i)) * NT + sgm - 1u] = wvl;
        }
        if (tid < (uint32_t)kLongOv) {
            const uint32_t wi = blk_word + NT * kLongSeg + tid;
            col[(kLongRows - 2u - ((uint32_t)kLongSeg + tid)) * NT + NT - 1u] = (wi < n) ? src[wi] : 0u;
        }
        __syncthreads();
        const uint32_t seg_word = blk_word + tid * kLongSeg;
        const uint32_t avail_bits = seg_word < n ? ((n - seg_word) > (1u << 26) ? 0xffffffffu : (n - seg_word) * 32u) : 0u;

        // first guess: only where the segment's last code ends is wanted, and a parse re-synchronises within a few
        // codes, so the guess starts kLongGuessBits before the segment's end (thread 0 knows its start)
        uint32_t start = tid == 0 ? carry_in : kLongSegBits - kLongGuessBits, end, cnt, sum;
        parse(true, start, avail_bits, std::false_type{}, 0u, 0u, end, cnt, sum);
        for (uint32_t it = 0; it < NT; ++it) {
            s_end[tid] = end;
            __syncthreads();
            // where the predecessor's last code ended, as a bit of MY segment (kLongSegBits = "nothing left for me")
            const uint32_t pe = tid ? s_end[tid - 1u] : 0u;
            const uint32_t ns = tid == 0 ? carry_in : (pe >= kLongSegBits ? pe - kLongSegBits : kLongSegBits);
            const bool changed = ns != start;
            if (!__syncthreads_or(changed ? 1 : 0)) break;  // (also orders the reads of s_end before its next writes)
            start = ns;
            uint32_t e2, c2, s2;
            parse(changed, start, avail_bits, std::false_type{}, 0u, 0u, e2, c2, s2);
            if (changed) { end = e2; cnt = c2; sum = s2; }
        }
        // prefix sums over the workgroup: samples before my segment, sum of deltas before my segment
        const uint32_t incl_c = wave_incl_scan_dpp(cnt), incl_s = wave_incl_scan_dpp(sum);
        if (lane == 63) { s_tot[0][wv] = incl_c; s_tot[1][wv] = incl_s; }
        s_end[tid] = end;
        __syncthreads();
        uint32_t pre_c = 0, pre_s = 0, tot_c = 0, tot_s = 0;
#pragma unroll
        for (int i = 0; i < kLongWaves; ++i) {
            const uint32_t tc = s_tot[0][i], ts = s_tot[1][i];
            if (i < wv) { pre_c += tc; pre_s += ts; }
            tot_c += tc;
            tot_s += ts;
        }
        const uint32_t end_last = s_end[NT - 1u];
        uint32_t e3, c3, s3;
        parse(true, start, avail_bits, std::true_type{}, done + pre_c + incl_c - cnt, acc_base + pre_s + incl_s - sum, e3, c3, s3);
        done = (tot_c > len - done) ? len : done + tot_c;
        acc_base += tot_s;
        carry_in = end_last >= kLongSegBits ? end_last - kLongSegBits : 0u;
        blk_word += NT * kLongSeg;
        __syncthreads();
    }
    if (done < len && tid == 0) atomicOr(&st->err, kErrCorrupt);  // the stream ended before the waveform did
}

// Staged lane-per-waveform decoder (the production kernel; generations 1-4 are in the git
// history, what each measurement changed is in DESIGN.md).
//
// Decomposition.  The Rice parse is serial inside a waveform, so the unit of parallelism is the
// waveform: one lane per waveform, 64 waveforms per wavefront.
//   stream in   each lane owns an LDS ring of RW words of its compressed stream, refilled in
//               pieces of LW words = one 128-byte line by 16-byte loads (every line of the stream is
//               requested once, by one lane, in one round).  A piece is loaded ahead of
//               need and written to the ring just before the round's stores are issued (vmcnt is
//               in order: a load issued after a store cannot be waited for without that store).
//   ring layout word-major and reversed, ring[RW - (w mod RW)][lane], plus a mirror row: a lane's
//               bank is its lane number whatever row it reads (no conflicts although the 64
//               streams drift apart), and the pair (w, w+1) is always (row+1, row).
//   per sample  the bit position is kept negated, Q = -P: row = Q[5 +: log2 RW] (v_bfe),
//               (lo, hi) = ds_read2st64_b32, win = v_alignbit(hi, lo, Q): 3 VALU + 1 LDS
//               instruction form the 32-bit window, no refill state.  Escape and ordinary codes
//               share one extraction (payload width kk = esc ? 16 : k; the 8 << 16 an escape leaves
//               above bit 15 never reaches the int16 running sum).  217 VALU instructions per group of
//               16 samples in the interior rounds (13.6 per sample; tests/test_lanes_decoder_build.py), 13
//               dependent VALU levels and one LDS round trip per pair: what bounds the parse is that chain.
//   samples out transposed through LDS; a lane-private start delay phi makes step u of every round
//               land u*2 bytes past a T*2-byte boundary, so each round stores whole aligned
//               128-byte lines (T = 64).  tools/ubench_store.hip: 16-byte stores reach 5.5 TB/s only
//               when every contiguous run is a whole line; 64-byte aligned runs give 4.2 TB/s and
//               runs that straddle lines 2.6-3.3 TB/s whatever their length.
//   pairs       two samples per ring access: three words = a 64-bit window always hold two codes
//               (2 x 25 bits); the second sample's window is v_alignbit(winA, winB, -len1).  One LDS
//               round trip on the dependent chain per two samples.
//   FUSED       the header-chain walk runs inside the same launch: workgroups take a ticket; the first
//               ceil(n_chunks/8) tickets walk (eight chunks per wave through scalar loads,
//               walk_chunks_scalar(), publishing one granule per waveform), every later ticket decodes
//               64 waveforms of one chunk as soon as their granules appear.  Decode tickets are dealt group-major (waveforms 0-63 of every chunk,
//               then 64-127 of every chunk, ...), the order in which the 2000-hop chains release them,
//               so the ~1.7 ms of dependent-load latency of the walk disappears behind the decode.
//               A ticket holder is by construction running, so waiting on a lower ticket's walker
//               cannot deadlock whatever the dispatch order.  (Uniform batches only.)
template <bool FUSED, bool GEN = false>
__global__ __launch_bounds__(64, 1) void k_decode_lanes(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                     const uint64_t *__restrict__ chunk_word_off,
                                                     uint64_t *__restrict__ wave_off,
                                                     uint32_t *__restrict__ wave_words,
                                                     uint64_t *__restrict__ granules, uint32_t *__restrict__ ticket,
                                                     DevStatus *st, int16_t *__restrict__ out) {
    constexpr int RW = 64;          // ring words per lane
    constexpr int LW = 32;          // words per stream piece: one 128-byte line
    constexpr int T = 64;           // samples per round
    constexpr int GS = 16;          // samples per group (a refill test per group)
    constexpr int LOG_RW = 6;
    constexpr int OSW = T / 2 + 4;  // output row stride in words: 16-byte aligned rows (the conflict-free 34 measured no faster)
    constexpr int PPS = T / 8;      // 16-byte pieces per stream per round
    constexpr int SPI = 64 / PPS;   // streams per write-out iteration
    constexpr int NV = LW / 4;      // 16-byte loads per piece
    constexpr uint32_t WMASK = (1u << 27) - 1u;
    constexpr uint32_t NEED_AT = GS + 2;                                   // must refill below this many words
    static_assert(T % GS == 0 && RW - LW >= GS + 2, "round length / ring slack");
    // row r: word w with RW - (w mod RW) == r; row 0 mirrors row RW and row -1 mirrors row RW - 1 (a pair reads
    // three consecutive words: rows r + 1, r, r - 1)
    __shared__ uint32_t ring_all[(RW + 2) * 64];
    uint32_t *const ring = ring_all + 64;
    __shared__ __attribute__((aligned(16))) uint32_t obuf[64 * OSW];  // doubles as the start-up tables
    uint64_t *tab_off = reinterpret_cast<uint64_t *>(obuf);  // [64] sample offset of step 0 of round 0
    uint32_t *tab_lo = obuf + 128, *tab_hi = obuf + 192;      // [64] each
    static_assert(64 * OSW >= 256, "tables fit in obuf");

    const int lane = lane_id();
    const uint32_t k = G.k;
    // Stores go through pointers with an explicit global address space: once `out` has travelled through
    // nested by-reference lambda captures the compiler no longer infers it and emits flat_store, which
    // also ticks lgkmcnt and serialises against the LDS traffic of the write-out (measured: 2x slower).
    typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
    typedef u32x4v __attribute__((address_space(1))) g_uint4;
    typedef int16_t __attribute__((address_space(1))) g_i16;
    g_i16 *const outg = (g_i16 *)out;
    uint64_t g;
    bool active;
    uint32_t len = 0, n = 0;
    uint64_t S = 1, ooff = 0;
    // Never read.  A reference bound to len (as the removed staged write-out's lambda held one) fixes the order in which
    // the compiler promotes these locals to registers; without it two independent zero moves swap places and the code
    // is no longer byte for byte that of c5db7d2.
    [[maybe_unused]] const uint32_t &len_ = len;
    const uint32_t wave_idx = blockIdx.x;  // (outside the ticketed launch)
    if (FUSED) {
        uint32_t tk = 0;
        if (lane == 0) tk = atomicAdd(ticket, 1u);
        tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk);
        // walker tickets first.  Chunks of short waveforms (tens of thousands of hops) are streamed
        // through LDS by a whole wave each (walk_chunk_block, in this wave's ring/transposition LDS),
        // the others are chased through scalar loads, kWalkChains chunks per wave.
        constexpr bool kBlockWalkFits = sizeof(ring_all) >= kWalkBlockWords * 4u && sizeof(obuf) >= kWalkHopCap * 8u;
        const bool u_short = G.uniform && G.u_wave_len <= kWalkShortLen;
        const uint32_t n_blockwalk = G.uniform ? (u_short ? (uint32_t)G.n_chunks : 0u) : G.n_short;
        const uint64_t n_chain = G.uniform ? (u_short ? 0ull : G.n_chunks) : (uint64_t)G.n_long;
        const uint32_t n_walk = n_blockwalk + (uint32_t)((n_chain + (uint32_t)kWalkChains - 1u) / (uint32_t)kWalkChains);
        if (tk < n_walk) {  // walker role
            __builtin_amdgcn_s_setprio(3);  // the chain is the critical path of the whole launch (A/B: -2.5 %)
            if (tk < n_blockwalk) {
                if constexpr (kBlockWalkFits) {
                    const uint64_t c = G.uniform ? (uint64_t)tk : (uint64_t)G.walk_short[tk];
                    walk_chunk_block(G, c, in, in_words, chunk_word_off, wave_off, wave_words, granules, st, ring_all,
                                     reinterpret_cast<uint2 *>(obuf));
                }
            } else {
                walk_chunks_scalar(G, (uint64_t)(tk - n_blockwalk) * kWalkChains, G.uniform ? nullptr : G.walk_long, n_chain,
                                   in, in_words, chunk_word_off, wave_off, wave_words, granules, st);
            }
            return;
        }
        // decode tickets, group-major: waveforms 0-63 of every chunk, then 64-127 of every chunk, ...
        const uint64_t t2 = tk - n_walk;
        uint64_t grp = t2 / G.n_chunks, c = t2 - grp * G.n_chunks;
        uint32_t idx = (uint32_t)grp * 64u + lane;  // waveform index inside chunk c
        uint64_t gr = 0;
        if (G.uniform) {
            // The chunks' LAST groups are partial (2000 waveforms: 31 full groups + 16 waveforms): several chunks' leftovers
            // share a wavefront -- 4 x 16 lanes for the headline batch, 15 625 wavefronts instead of 16 000, the last 500 of
            // them a quarter full (1920 against 2000 waveforms per chunk had measured 4 %).  Everything below is per lane.
            const uint32_t full = G.u_n_waves >> 6, rem = G.u_n_waves & 63u;
            const uint64_t t_full = (uint64_t)full * G.n_chunks;
            if (t2 < t_full) {
                active = true;
            } else {
                if (rem == 0u) return;
                const uint32_t per = 64u / rem, sub = (uint32_t)lane / rem;
                const uint64_t c0 = (t2 - t_full) * per;
                if (c0 >= G.n_chunks) return;
                c = c0 + sub;
                idx = full * 64u + ((uint32_t)lane - sub * rem);
                active = sub < per && c < G.n_chunks;
                if (!active) { c = c0; idx = 0; }
            }
            g = c * G.u_n_waves + idx;
            if (active) {
                len = (idx + 1 == G.u_n_waves) ? (G.u_n_samples - idx * G.u_wave_len) : G.u_wave_len;
                ooff = c * (uint64_t)G.u_n_samples + (uint64_t)idx * G.u_wave_len;
            }
        } else {
            // ragged: the grid covers max_groups groups of every chunk; a chunk with fewer has idle tickets
            const ChunkDesc d = G.chunks[c];
            if ((uint32_t)grp * 64u >= d.n_waves) return;
            active = idx < d.n_waves;
            g = d.wave_base + idx;
            if (active) {
                len = (idx + 1 == d.n_waves) ? (d.n_samples - idx * d.wave_len) : d.wave_len;
                ooff = d.sample_off + (uint64_t)idx * d.wave_len;
            }
        }
        uint32_t spins = 0;
        for (;;) {  // wait for this wave's granules; the walker that writes them holds a lower ticket
            if (active && !(gr & kGranValid))
                gr = __hip_atomic_load(granules + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!__any(active && !(gr & kGranValid))) break;
            __builtin_amdgcn_s_sleep(8);
            if (++spins > (1u << 24)) {  // cannot happen; never hang the GPU
                if (lane == 0) atomicOr(&st->err, kErrInternal);
                gr |= kGranValid;
                break;
            }
        }
        if (active) {
            n = granule_words(gr);
            S = chunk_word_off[c] + granule_pos(gr) + 1u;
        }
    } else if (!G.uniform && G.rag_order) {
        // ragged batch: wavefronts in order of decreasing WaveformLength (longest processing time first).  A lane takes
        // ~60 ns per sample whatever else runs, so a wavefront of 16 384-sample waveforms that starts last adds its
        // whole 1 ms to the launch (config 5: 1.9 -> 1.2 ms)
        if (wave_idx >= G.rag_groups) return;
        const uint2 e = G.rag_order[wave_idx];  // {chunk, group of 64 waveforms inside it}
        const ChunkDesc d = G.chunks[e.x];
        const uint32_t idx = e.y * 64u + (uint32_t)lane;
        active = idx < d.n_waves;
        g = d.wave_base + idx;
        if (active) {
            len = (idx + 1 == d.n_waves) ? (d.n_samples - idx * d.wave_len) : d.wave_len;
            ooff = d.sample_off + (uint64_t)idx * d.wave_len;
            S = wave_off[g] + 1u;
            n = wave_words[g];
        }
    } else {
        g = (uint64_t)wave_idx * 64u + lane;
        active = g < G.total_waves;
        if (active) {
            const WaveRef r = locate(G, g);
            len = r.len;
            ooff = r.sample_off;
            S = wave_off[g] + 1u;
            n = wave_words[g];
        }
    }
    // start delay: step u of every round sits u*2 bytes past a T*2-byte boundary
    const uint32_t phi = active ? (uint32_t)((((uintptr_t)out >> 1) + ooff) & (uint64_t)(T - 1)) : 0u;
    const uint32_t steps = wave_max_u32(len + phi);
    const uint32_t lo_max = wave_max_u32(phi);
    const uint32_t hi_min = ~wave_max_u32(~(phi + len));
    uint64_t wo_off[PPS];  // write-out constants: piece p of stream st_i, i = 0..PPS-1
    uint32_t wo_lo[PPS], wo_hi[PPS];
    tab_off[lane] = ooff - phi;
    tab_lo[lane] = phi;
    tab_hi[lane] = phi + len;
    wave_sync();
#pragma unroll
    for (int i = 0; i < PPS; ++i) {
        const int st = i * SPI + lane / PPS, p = lane % PPS;
        wo_off[i] = tab_off[st] + 8u * (uint32_t)p;
        wo_lo[i] = tab_lo[st];
        wo_hi[i] = tab_hi[st];
    }
    wave_sync();

    const uint64_t A = (S & ~(uint64_t)(RW - 1)) - (uint64_t)RW;  // s0 in [RW, 2 RW)
    const uint32_t s0 = (uint32_t)(S - A);
    const uint32_t endw = s0 + n;
    uint32_t flw = s0 & ~(uint32_t)(LW - 1);
    const bool in_vec_ok = ((uintptr_t)in & 15u) == 0;
    uint32_t *myring = ring + lane;
    typedef uint16_t __attribute__((may_alias)) u16a;
    u16a *myout = reinterpret_cast<u16a *>(obuf + lane * OSW);
    // the round's whole-line stores
    auto store16 = [&](g_i16 *dst, const uint4 &v) __attribute__((always_inline)) {
        *(g_uint4 *)dst = (u32x4v){v.x, v.y, v.z, v.w};
    };
    // 16 bytes of a stream's row: one ds_read_b128
    auto orow16 = [&](int st, int p) __attribute__((always_inline)) -> uint4 {
        return *reinterpret_cast<const uint4 *>(obuf + st * OSW + 4 * p);
    };

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
    // Q_need: position (in Q units, Q decreases) at which this lane must have its next piece;
    // 0x7fffffff away from Q means "never" (stream exhausted)
    uint32_t Q_need;
    auto set_limits = [&]() __attribute__((always_inline)) {
        // avail = flw - cw < X  <=>  cw > flw - X  <=>  Q <= ~(32 * (flw - X + 1) - 1) ... kept simple:
        // cw = (~Q) >> 5, so cw >= c  <=>  ~Q >= 32 c  <=>  Q <= ~(32 c)
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
    int32_t acc = 0;
    // GEN: inverse of a general prediction filter with taps[0] = +-1 and at most 4 taps (src/deltaRice.c:92-101):
    // y[i] = +-(d[i] - sum_{j=1..3} taps[j] y[i-j]) in int16, i.e. modulo 2^16 (only the low 16 bits of the
    // products count, so 24-bit multiplies of whatever the registers hold above bit 15 are exact).
    // acc is y[i-1]; y2, y3 the two before it; all zero before the waveform (:96 `if ((i - j) >= 0)`).
    int32_t y2 = 0, y3 = 0;
    const uint32_t nt1 = GEN ? G.fast_nt[0] & 0xffffu : 0u, nt2 = GEN ? G.fast_nt[1] & 0xffffu : 0u,
                   nt3 = GEN ? G.fast_nt[2] & 0xffffu : 0u;
    const bool t0neg = GEN && G.fast_t0neg;
    auto advance = [&](int32_t d) __attribute__((always_inline)) {
        if constexpr (GEN) {
            uint32_t a = (uint32_t)d + __umul24(nt1, (uint32_t)acc) + __umul24(nt2, (uint32_t)y2) + __umul24(nt3, (uint32_t)y3);
            if (t0neg) a = 0u - a;
            y3 = y2;
            y2 = acc;
            acc = (int32_t)a;
        } else {
            acc += d;
        }
    };

    // Where the lane's last code ended (as Q): a valid waveform's codes end inside its last payload word, i.e.
    // n_i = ceil(bits / 32) (src/deltaRice.c:237-241) -- checked after the last round, so that flipped payload bits
    // that change a code length are reported (DRX_ERR_CORRUPT) instead of decoding to garbage silently.  The last
    // step of a lane lies in an edge round or is the last step of an interior round: only those capture.
    const uint32_t hi_step = phi + len;  // this lane decodes its last sample in step hi_step - 1
    uint32_t Q_end = 0;
    auto decode_group = [&](auto first_tag, auto edge_tag, int tg, uint32_t tcur) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first_tag)::value;
        constexpr bool EDGE = decltype(edge_tag)::value;  // tcur + u is the step index; capture Q_end
        if (!FIRST) {
            // two samples per ring access: a 64-bit window (three words) always holds two codes (2 x 25 bits),
            // so the second sample's window is one v_alignbit away from the first one's length -- one LDS
            // round trip on the dependent chain per two samples instead of one per sample
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
                if constexpr (EDGE) {
                    Q_end = (tcur + (uint32_t)u + 1u == hi_step) ? Q + nu1 : Q_end;
                    Q_end = (tcur + (uint32_t)u + 2u == hi_step) ? Q + nu1 + nu2 : Q_end;
                }
                asm("v_add3_u32 %0, %1, %2, %3" : "=v"(Q) : "v"(Q), "v"(nu1), "v"(nu2));
                const uint32_t z1 = (q1 << kk1) + __builtin_amdgcn_ubfe(winA, nu1, kk1);
                const uint32_t z2 = (q2 << kk2) + __builtin_amdgcn_ubfe(win2, nu2, kk2);
                advance((int32_t)(z1 >> 1) ^ -(int32_t)(z1 & 1u));
                const uint32_t a1 = (uint32_t)acc;
                advance((int32_t)(z2 >> 1) ^ -(int32_t)(z2 & 1u));
                // low halves of the two running sums in one v_perm_b32
                *reinterpret_cast<uint32_t *>(myout + tg + u) = __builtin_amdgcn_perm((uint32_t)acc, a1, 0x05040100u);
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < GS; ++u) {
            const uint32_t row = __builtin_amdgcn_ubfe(Q, 5u, (uint32_t)LOG_RW);
            const uint32_t *wp = myring + row * 64u;
            const uint32_t lo = wp[0], hi = wp[64];
            const uint32_t win = __builtin_amdgcn_alignbit(hi, lo, Q);
            const uint32_t q = ffbh(win);  // win == 0 only past the end of a corrupt stream
            const bool esc = win < (1u << 24);
            const uint32_t kk = esc ? 16u : k;
            const uint32_t used = q + kk + 1u;
            const uint32_t rem = __builtin_amdgcn_ubfe(win, 32u - used, kk);
            const uint32_t z = (q << kk) + rem;  // escape: 8 << 16 stays above bit 15
            const int32_t d = (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
            const bool act = (uint32_t)(tg + u) >= phi;  // (the first round: one sample per access, lanes start at phi)
            const int32_t o1 = acc, o2 = y2, o3 = y3;
            advance(d);
            acc = act ? acc : o1;
            y2 = act ? y2 : o2;
            y3 = act ? y3 : o3;
            Q = act ? Q - used : Q;
            if constexpr (EDGE) Q_end = (tcur + (uint32_t)u + 1u == hi_step) ? Q : Q_end;
            myout[tg + u] = (uint16_t)acc;
        }
    };

    // piece i of an EDGE round (first / last rounds of a waveform): only the samples that belong to the stream
    auto emit_masked = [&](g_i16 *dst, uint32_t lo, uint32_t hi, uint32_t t0, const uint4 &v) __attribute__((always_inline)) {
        const int p = lane % PPS;
        const uint32_t tpos = t0 + 8u * (uint32_t)p;  // step index of the piece's first sample
        if (tpos + 8u > lo && tpos < hi) {
            if (tpos >= lo && tpos + 8u <= hi) {
                *(g_uint4 *)dst = (u32x4v){v.x, v.y, v.z, v.w};
            } else {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (tpos + (uint32_t)j >= lo && tpos + (uint32_t)j < hi)
                        dst[j] = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
            }
        }
    };
    auto write_out = [&](uint32_t t0) __attribute__((always_inline)) {
        if (t0 >= lo_max && t0 + T <= hi_min) {  // interior round: whole aligned lines only
#pragma unroll
            for (int i = 0; i < PPS; ++i) {
                const int st = i * SPI + lane / PPS, p = lane % PPS;
                const uint4 v = orow16(st, p);
                store16(outg + wo_off[i] + t0, v);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PPS; ++i) {
                const int st = i * SPI + lane / PPS, p = lane % PPS;
                const uint32_t tpos = t0 + 8u * (uint32_t)p;
                if (tpos + 8u > wo_lo[i] && tpos < wo_hi[i]) emit_masked(outg + wo_off[i] + t0, wo_lo[i], wo_hi[i], t0, orow16(st, p));
            }
        }
    };

    // round 0 (start delays; synchronous refills; runs once)
    if (steps > 0) {
#pragma unroll 1
        for (int tg = 0; tg < T; tg += GS) {
            sync_refill();
            decode_group(std::true_type{}, std::true_type{}, tg, (uint32_t)tg);
        }
        wave_sync();
        write_out(0);
        wave_sync();
    }

    // steady state.  Stream pieces are requested at the END of a round, just BEFORE the round's stores
    // are issued, and written to the ring at the end of a later round.  vmcnt retires in issue order
    // and counts loads and stores together, so a wait for loads that are OLDER than the PPS stores of
    // their own round is `s_waitcnt vmcnt(PPS)` and never waits for those stores (ablation: loads alone
    // +0.04 ms, stores alone +0.11 ms, both +1.0 ms when the commit had to drain the stores too).
    // The interior rounds (every stream fully inside its waveform: whole-line stores only) run in a
    // loop of their own whose only vector-memory operations are those loads and those PPS stores, so
    // that the compiler's waitcnt insertion can prove the count.  ONE piece per lane is in flight: a piece is
    // a whole 128-byte line, so every line of a stream is requested once, by one lane, by the NV loads of one
    // round (two 64-byte halves a round apart found a quarter of the lines gone from L2 again: 1.24 x the
    // stream in HBM reads).  A lane requests its next piece as soon as it holds none and commits it at the
    // first round end (or refill test) at which it fits, avail <= RW - LW; until then it stays in its
    // registers.  A piece that does not fit at a round's end leaves more than RW - LW words, so at a STEADY
    // rate of up to (RW - LW - NEED_AT) / 0.75 = 18 words per round (9 bits per sample; the headline's mean
    // is 13) a stream does not reach a refill test short of words, and at up to LW words per round (16 bits
    // per sample) it commits at a refill test at the earliest without waiting for a load; hungrier streams
    // take the rest through sync_refill().  That is arithmetic: rates vary from waveform to waveform and from
    // round to round, and how often the interior loop enters sync_refill() on a real batch is not counted.
    auto edge_round = [&](uint32_t t0) __attribute__((always_inline)) {  // first / last rounds: masked stores, synchronous refills
#pragma unroll 1
        for (int tg = 0; tg < T; tg += GS) {
            sync_refill();
            decode_group(std::false_type{}, std::true_type{}, tg, t0 + (uint32_t)tg);
        }
        wave_sync();
        write_out(t0);
        wave_sync();
    };
    uint32_t t0 = T;
    for (; t0 < steps && !(t0 >= lo_max && t0 + T <= hi_min); t0 += T) edge_round(t0);

    uint4 pv[NV];        // the piece in flight
    bool pneed = false;  // this lane has one in flight
    set_limits();
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
    for (; t0 + T <= hi_min && t0 < steps; t0 += T) {  // interior rounds
#pragma unroll 1
        for (int tg = 0; tg < T; tg += GS) {
            group_refill();
            decode_group(std::false_type{}, std::false_type{}, tg, 0u);
        }
        Q_end = (t0 + (uint32_t)T == hi_step) ? Q : Q_end;  // a lane whose last step closes an interior round
        wave_sync();
        commit_if_fits();  // loads of an earlier round's end: older than that round's PPS stores
        wave_sync();
        set_limits();
        if (!pneed) {
            // behind the last interior round a piece is committed once more and then dropped: there, request only what
            // fits already (a dropped piece would be fetched again by the edge rounds' sync_refill())
            const bool last = !(t0 + 2u * T <= hi_min && t0 + T < steps);
            const uint32_t avail = (flw - ((~Q) >> 5)) & WMASK;
            pneed = (flw < endw) && (!last || avail <= (uint32_t)(RW - LW));
            if (pneed) load_piece(pv);
        }
#pragma unroll
        for (int i = 0; i < PPS; ++i) {  // whole aligned lines only
            const int st = i * SPI + lane / PPS, p = lane % PPS;
            const uint4 v = orow16(st, p);
            store16(outg + wo_off[i] + t0, v);
        }
        wave_sync();
    }
    commit_if_fits();
    pneed = false;  // a piece that still does not fit is dropped (flw has not advanced: sync_refill() fetches it again)
    wave_sync();
    for (; t0 < steps; t0 += T) edge_round(t0);
    // bits of the waveform = -Q_end - 32 s0 (Q counts from A); n_i words hold them exactly
    if (active && len && (((0u - Q_end) - 32u * s0 + 31u) >> 5) != n) atomicOr(&st->err, kErrCorrupt);
}

// ---------------------------------------------------------------------------
// the lane decoder's ragged plan, the decode route and launch (host side, same translation unit so that <<<>>> stays in HIP code)
// ---------------------------------------------------------------------------
std::vector<uint2> decode_plan_ragged(Geom &G, const ChunkDesc *d) {
    const uint64_t n = G.n_chunks;
    uint32_t max_groups = 0, max_len = 0;
    for (uint64_t c = 0; c < n; ++c) {
        max_groups = std::max(max_groups, (d[c].n_waves + 63u) / 64u);
        max_len = std::max(max_len, d[c].wave_len);
    }
    G.max_groups = max_groups;
    G.max_wave_len64 = 64ull * max_len;
    // decode order: wavefronts (groups of 64 waveforms of one chunk) by decreasing WaveformLength
    std::vector<uint32_t> by_len(n);
    for (uint64_t c = 0; c < n; ++c) by_len[c] = (uint32_t)c;
    std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t a, uint32_t b) { return d[a].wave_len > d[b].wave_len; });
    std::vector<uint2> order;
    uint64_t n_long_groups = 0;
    for (uint32_t c : by_len)
        for (uint32_t j = 0; j < (d[c].n_waves + 63u) / 64u; ++j) {
            order.push_back(make_uint2(c, j));
            if (d[c].wave_len > kWalkShortLen) ++n_long_groups;
        }
    if (order.size() <= 0x7fffffffull) {
        G.rag_groups = (uint32_t)order.size();
        G.rag_groups_long = (uint32_t)n_long_groups;
    } else {
        order.clear();
    }
    return order;
}

// ---------------------------------------------------------------------------
// How a decode call is routed: ONE table, first matching row wins (route_decode()).
//
//   decoder       | when                                                                              | walk in front of it
//   --------------+-----------------------------------------------------------------------------------+--------------------------------
//   SIMPLE        | decode_impl 0; a filter the fast kernels do not take (> 4 taps, taps[0] != +-1)   | parallel walks / serial
//   BLOCKS (+IIR) | few long waveforms (blocks_batch(): geometry and cost), delta or a fast filter    | parallel walks / serial
//   LONG          | uniform, delta, long_waveform_batch() and not BLOCKS; LONG_NOT_BLOCKS             | parallel walks / serial
//   LANES fused   | decode_impl 8, not a batch the parallel walks take (short waveforms in many    | inside the launch
//                 | chunks, chunks of more than 8192 or fewer than 8 waveforms), grid not mostly idle |
//   LANES         | everything else                                                                   | parallel walks / serial
//   LANES split   | ... ragged batches behind both parallel walks: a lanes launch behind each         | both parallel walks
//
// Which walk "parallel walks / serial" is: route_walk() and its table, drx_walk.hip.
// Flags (DRX_DBG_*): NO_LONG_PATHS never BLOCKS / LONG, LONG_NOT_BLOCKS LONG instead of BLOCKS, RAGGED_ONE_LANES_LAUNCH; the
// walk's own with route_walk().
// ---------------------------------------------------------------------------
enum class Dec { Simple, Blocks, Long, LanesFused, Lanes, LanesSplit };
enum class Walk { None, InLaunch, Parallel, Serial };
struct DecodeRoute {
    Dec dec;
    Walk walk;
    WalkRoute par;  // Walk::Parallel: which of the two
    bool gen;       // a general prediction filter
};

static DecodeRoute route_decode(const Geom &G, int impl, bool tables_ready, bool have_pw, bool have_blk, bool have_side) {
    DecodeRoute R{};
    R.gen = G.n_taps != 0;
    R.par = route_walk(G, tables_ready, have_pw);
    const bool simple = impl == 0 || (R.gen && !G.fast_taps);
    const bool want_fused = !tables_ready && impl == 8;
    const bool blocks = !simple && !(G.dbg & (DRX_DBG_NO_LONG_PATHS | DRX_DBG_LONG_NOT_BLOCKS)) && have_blk && blocks_batch(G) && (!R.gen || (G.iir_tab && G.iir_state));
    const bool longp = !simple && !blocks && !R.gen && !(G.dbg & DRX_DBG_NO_LONG_PATHS) && G.uniform && long_waveform_batch(G.total_waves, G.u_wave_len);
    // ragged: the group-major grid of the fused launch has max_groups tickets per chunk; not when most of them would be idle
    const bool sparse = !G.uniform && (uint64_t)G.n_chunks * G.max_groups > 8ull * ((G.total_waves + 63u) / 64u) + 4096ull;
    R.dec = simple ? Dec::Simple : (blocks ? Dec::Blocks : (longp ? Dec::Long : Dec::Lanes));
    const bool parallel = R.par.chunk_wide || R.par.blocks;
    if (R.dec == Dec::Lanes && want_fused && !sparse && !parallel) R.dec = Dec::LanesFused;
    R.walk = tables_ready ? Walk::None : (R.dec == Dec::LanesFused ? Walk::InLaunch : (parallel ? Walk::Parallel : Walk::Serial));
    if (R.dec == Dec::Lanes && R.par.chunk_wide && R.par.blocks && have_side && G.rag_order && G.rag_groups_long &&
        G.rag_groups_long < G.rag_groups && !(G.dbg & DRX_DBG_RAGGED_ONE_LANES_LAUNCH)) R.dec = Dec::LanesSplit;
    return R;
}

hipError_t launch_decode(const StreamCall &c, int16_t *d_out, uint64_t *d_granules, int impl, void *d_blk, const SideStream *side,
                         uint32_t *path_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    uint32_t path_dummy = 0;
    uint32_t &path = path_out ? *path_out : path_dummy;
    path = 0;
    if (G.total_waves == 0) return hipSuccess;
    mark(c.ev, 0, s);
    const DecodeRoute R = route_decode(G, impl, c.tables_ready, c.d_pw != nullptr, d_blk != nullptr, side && side->s);
    const bool gen = R.gen;
    const unsigned nb_plain = blocks_for(G.total_waves, 64);

    // the lane-per-waveform launch behind a walk (tables in wave_off / wave_words): `nb` wavefronts of the frame's view and stream
    auto launch_lanes = [&](const StreamCall &v, unsigned nb) {
        path |= DRX_PATH_LANES;
        if (gen)
            k_decode_lanes<false, true><<<nb, 64, 0, v.s>>>(*v.G, v.d_in, v.in_words, v.d_chunk_word_off, v.d_wave_off, v.d_wave_words, nullptr, nullptr, v.d_status, d_out);
        else
            k_decode_lanes<false><<<nb, 64, 0, v.s>>>(*v.G, v.d_in, v.in_words, v.d_chunk_word_off, v.d_wave_off, v.d_wave_words, nullptr, nullptr, v.d_status, d_out);
    };

    // ---- the walk ----
    if (R.walk == Walk::InLaunch) {
        // granules + ticket word, zeroed before every launch (a granule is its own ready flag)
        hipError_t e = hipMemsetAsync(d_granules, 0, (G.total_waves + 2) * sizeof(uint64_t), s);
        if (e != hipSuccess) return e;
    } else if (R.walk == Walk::Parallel) {
        const bool split = R.dec == Dec::LanesSplit;
        hipError_t e = walk_scratch_reset(G, c.d_pw, s);
        if (e != hipSuccess) return e;
        // a ragged batch has both kinds of chunk and the two walks touch different chunks: the chunk-wide walk goes to the
        // context's side stream while the block walk runs here (config 5: 0.18 ms of 0.6 off the critical path)
        const bool forked = R.par.chunk_wide && R.par.blocks && side && side->s;
        hipStream_t spw = forked ? side->s : s;
        if (forked) {
            if ((e = hipEventRecord(side->fork, s)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(side->s, side->fork, 0)) != hipSuccess) return e;
        }
        if (R.par.chunk_wide) launch_walk_chunk_wide(c.on(spw), R.par.by_chains);
        // ... and so does the decoding of the long-waveform chunks, whose tables are complete long before the block walk is
        // through: their wavefronts (the first rag_groups_long of the longest-first order) are launched behind the
        // chunk-wide walk on the side stream, the rest here behind the block walk
        if (split) {
            Geom Gl = G;
            Gl.rag_groups = G.rag_groups_long;
            launch_lanes(c.view(Gl).on(spw), Gl.rag_groups);
        }
        if (forked && (e = hipEventRecord(side->join, side->s)) != hipSuccess) {
            // the side stream's kernels write this call's tables and output: never return with them unordered
            (void)hipStreamSynchronize(side->s);
            return e;
        }
        if (R.par.blocks) launch_walk_blocks(c);
        if (split) {
            mark(c.ev, 1, s);  // (the block walk's end; the other stream is decoding already)
            Geom Gs = G;
            Gs.rag_order = G.rag_order + G.rag_groups_long;
            Gs.rag_groups = G.rag_groups - G.rag_groups_long;
            launch_lanes(c.view(Gs), Gs.rag_groups);
        }
        if (forked && (e = hipStreamWaitEvent(s, side->join, 0)) != hipSuccess) {
            (void)hipStreamSynchronize(side->s);
            return e;
        }
    } else if (R.walk == Walk::Serial) {
        launch_walk_serial(c);
    }
    if (R.dec != Dec::LanesSplit) mark(c.ev, 1, s);

    // ---- the decoder ----
    switch (R.dec) {
    case Dec::LanesFused: {
        uint32_t *ticket = reinterpret_cast<uint32_t *>(d_granules + G.total_waves);
        unsigned n_walk, groups;
        unsigned nb;
        if (G.uniform) {
            n_walk = (G.u_wave_len <= kWalkShortLen) ? (unsigned)G.n_chunks : blocks_for(G.n_chunks, kWalkChains);
            groups = (G.u_n_waves + 63u) / 64u;
            // full groups of every chunk, then the chunks' partial last groups, 64 / (waveforms left) chunks to a wavefront
            const uint32_t full = G.u_n_waves >> 6, rem = G.u_n_waves & 63u;
            nb = n_walk + (unsigned)(G.n_chunks * full) + (rem ? (unsigned)((G.n_chunks + 64u / rem - 1u) / (64u / rem)) : 0u);
        } else {
            n_walk = G.n_short + blocks_for(G.n_long, kWalkChains);
            groups = G.max_groups;
            nb = n_walk + (unsigned)(G.n_chunks * groups);
        }
        path |= DRX_PATH_LANES_FUSED;
        if (gen)
            k_decode_lanes<true, true><<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off, c.d_wave_words, d_granules, ticket, c.d_status, d_out);
        else
            k_decode_lanes<true><<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off, c.d_wave_words, d_granules, ticket, c.d_status, d_out);
        break;
    }
    case Dec::Blocks: {
        // a workgroup per block of every waveform (drx_blocks.hip); waveforms it flags are decoded again, one
        // workgroup each, by the kernel that also judges them
        const uint32_t *fail = nullptr, *suspect = nullptr;
        bool fused = false;
        hipError_t e = launch_decode_blocks(c, d_blk, d_out, &fail, &suspect, gen, &fused);
        if (e != hipSuccess) return e;
        path |= DRX_PATH_BLOCKS | (gen ? (fused ? DRX_PATH_IIR_FUSED : DRX_PATH_IIR) : 0u);
        k_decode_long<<<(unsigned)G.total_waves, kLongThreads, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, c.d_status, d_out, fail, suspect, gen ? 1u : 0u);
        if (gen) {
            // (not fused: residuals -> samples, in place;) then the waveforms the block decoder flagged, serially (a slope-1 ramp)
            if (!fused && (e = launch_iir(G, G.iir_chunk_tile_base, G.iir_n_tiles, G.iir_tab, G.iir_state, fail, c.d_status, d_out, s)) != hipSuccess) return e;
            k_decode_simple<<<nb_plain, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, c.d_status, d_out, fail);
        }
        break;
    }
    case Dec::Long:  // (LONG_NOT_BLOCKS, or a long-waveform batch the block decoder does not take: one workgroup per waveform)
        path |= DRX_PATH_LONG;
        k_decode_long<<<(unsigned)G.total_waves, kLongThreads, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, c.d_status, d_out, nullptr, nullptr, 0u);
        break;
    case Dec::Lanes:
        launch_lanes(c, (!G.uniform && G.rag_order) ? G.rag_groups : nb_plain);  // (ragged: groups per chunk round up)
        break;
    case Dec::LanesSplit:  // (both launches went out behind their walks)
        break;
    case Dec::Simple:
        path |= DRX_PATH_SIMPLE;
        k_decode_simple<<<nb_plain, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, c.d_status, d_out, nullptr);
        break;
    }
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
