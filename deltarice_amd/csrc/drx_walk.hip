// drx_walk.hip -- the header-chain walk in front of the decoders: its kernels, its planner, its route and its launchers
// (the walkers that run INSIDE k_decode_lanes' launch: drx_walk.h, shared with drx_decode_kernels.hip).
//
// The format's only way to waveform i + 1 is the length header of waveform i (src/deltaRice.c:320-325).  The forms:
//   scalar chains     one lane (eight scalar-load chains per wave) per chunk, hop by hop;
//   LDS block walker  chunks of short waveforms streamed through LDS by a whole wave;
//   chunk-wide walk   k_walk_sparse (64 chains per chunk, the chunk is not read) or k_pw_scan + k_walk_parallel (candidate
//                     headers, binary lifting): chunks of long waveforms;
//   block-parallel    k_bw_blocks, k_bw_scan, then k_bw_emit or k_bw_chase: every B-word block of a chunk of short waveforms
//                     holds a header (both passes over the blocks sit on one streamer, bw_stream_blocks());
//   side-band         k_sideband_tables: no walk, the caller's n_i table checked against the stream.
// Every walker validates while it walks (sample count, n_i bounds, the chain ends at the chunk's end), and every one spells
// the format's rules through the same few helpers: a chunk's frame chunk_geom() and its headers' bounds header_bounds()
// (drx_device.h), the extent rule chunk_extent_usable() and the table entry store_entry() / store_rejected() (drx_walk.h), the
// list prefix wave_running_prefix() and its search slot_of() (here).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_walk.h"

namespace drx {

// The serial walkers (drx_walk.h) as kernels of their own.  (The LDS block walker's chase loop is held to its place in a line
// of code -- kChasePad, walk_chunk_block() -- which is worth 9 % of k_walk_block; profiles/walk_refactor_ab.txt section 3c.)
__global__ __launch_bounds__(64) void k_walk_block(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                   const uint64_t *__restrict__ chunk_word_off,
                                                   const uint32_t *__restrict__ chunk_list, uint32_t n_list,
                                                   uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                   DevStatus *st) {
    __shared__ __attribute__((aligned(16))) uint32_t blk[kWalkBlockWords];
    __shared__ __attribute__((aligned(8))) uint2 hop[kWalkHopCap];  // {position in the block, n}
    if (blockIdx.x >= n_list) return;
    const uint64_t c = chunk_list ? chunk_list[blockIdx.x] : blockIdx.x;
    walk_chunk_block<kChasePad>(G, c, in, in_words, chunk_word_off, wave_off, wave_words, nullptr, st, blk, hop);
}

// ... for the chunks the block-parallel walk flagged in `only`
__global__ __launch_bounds__(64) void k_walk_block_only(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                        const uint64_t *__restrict__ chunk_word_off,
                                                        uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                        DevStatus *st, const uint32_t *__restrict__ only) {
    __shared__ __attribute__((aligned(16))) uint32_t blk[kWalkBlockWords];
    __shared__ __attribute__((aligned(8))) uint2 hop[kWalkHopCap];
    const uint64_t c = blockIdx.x;
    if (c >= G.n_chunks || !only[c]) return;
    walk_chunk_block<kChasePad>(G, c, in, in_words, chunk_word_off, wave_off, wave_words, nullptr, st, blk, hop);
}

__global__ __launch_bounds__(64) void k_walk_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                  const uint64_t *__restrict__ chunk_word_off,
                                                  const uint32_t *__restrict__ chunk_list, uint32_t n_list,
                                                  uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                  DevStatus *st) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_list) return;
    walk_chunk(G, chunk_list[i], in, in_words, chunk_word_off, wave_off, wave_words, nullptr, st);
}

__global__ __launch_bounds__(64) void k_walk_scalar(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                    const uint64_t *__restrict__ chunk_word_off,
                                                    uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                    DevStatus *st) {
    walk_chunks_scalar(G, (uint64_t)blockIdx.x * kWalkChains, nullptr, G.n_chunks, in, in_words, chunk_word_off, wave_off,
                       wave_words, nullptr, st);
}

__global__ __launch_bounds__(64) void k_walk_scalar_only(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                         const uint64_t *__restrict__ chunk_word_off,
                                                         uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                         DevStatus *st, const uint32_t *__restrict__ only) {
    walk_chunks_scalar(G, (uint64_t)blockIdx.x * kWalkChains, nullptr, G.n_chunks, in, in_words, chunk_word_off, wave_off,
                       wave_words, nullptr, st, only);
}

// What the parallel walks share.  A running prefix over a list, 64 entries a step by one wavefront: -> the inclusive prefix of
// this lane's entry v; `run` (wave uniform) carries the steps' total on.
__device__ __forceinline__ uint32_t wave_running_prefix(uint32_t v, uint32_t &run) {
    const uint32_t incl = wave_incl_scan_dpp(v), r = run + incl;
    run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    return r;
}
// ... and the slot of such a prefix that holds unit u: pre[slot] <= u < pre[slot + 1], for pre[0] <= u < pre[n]
__device__ __forceinline__ uint32_t slot_of(const uint32_t *pre, uint32_t n, uint32_t u) {
    uint32_t lo = 0, hi = n;  // invariant: pre[lo] <= u < pre[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// The header chain WITHOUT its 2000 dependent round trips, for batches of a handful of chunks (where nothing hides
// them: 1.7 ms of a 2.2 ms decode).  A length header is a small number (n_i <= 25 bits per sample: 5469 for
// L = 7000) and payload words are Rice-coded bits, which practically never start with 19 zero bits.  So:
//   1. the whole chunk is read once (k_pw_scan, 16 workgroups per chunk) and every word <= that bound becomes a
//      CANDIDATE header (the ~2000 real ones plus a few impostors); one workgroup per chunk sorts them by position;
//   2. candidate i links to the candidate at position pos_i + n_i + 1 (binary search), to END if that is the chunk
//      end, to INVALID if no candidate sits there;
//   3. binary lifting over those links (up[k][i] = 2^k links ahead), then waveform w's header is w links from the
//      candidate at word 1: eleven steps, every waveform in parallel.  Impostors are simply never reached.
// Anything unexpected (too many candidates, a broken link, a chain that does not end at the chunk end) flags the
// chunk, and the scalar-load walker walks -- and judges -- the flagged chunks afterwards.
constexpr int kPwThreads = 1024;
constexpr uint32_t kPwCap = 4096;      // candidates per chunk
constexpr uint32_t kPwMaxParts = 128;  // slices of a chunk (pw_parts())
constexpr uint32_t kPwStride = kPwCap + kPwMaxParts;  // a chunk's scratch: its candidates, then {first, count} of every slice
constexpr int kPwLevels = 12;
constexpr uint32_t kPwMaxWaves = 3584;  // waveforms per chunk this form takes (leaves room for impostors)
constexpr uint64_t kPwMaxChunks = 224;  // the walks that READ the chunks (this form behind DRX_DBG_WALK_BY_SCAN, the block-parallel
                                        // walk): more chunks hide the serial walk behind the decoding

// 1. candidates of one slice of a chunk -> the chunk's list in global memory (cand: kPwCap x {pos, val} per chunk,
//    cand_count: one counter per chunk, zeroed before the launch)
__global__ __launch_bounds__(256) void k_pw_scan(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                 const uint64_t *__restrict__ chunk_word_off, const uint32_t *__restrict__ list,
                                                 uint2 *__restrict__ cand, uint32_t *__restrict__ cand_count, uint32_t parts) {
    const uint64_t c = list ? (uint64_t)list[blockIdx.x / parts] : blockIdx.x / parts;  // scratch is indexed by chunk
    const uint32_t part = blockIdx.x % parts, tid = threadIdx.x;
    const uint64_t begin = chunk_word_off[c], end = chunk_word_off[c + 1];
    if (!chunk_extent_usable(begin, end, in_words, kParWalkMaxWords)) return;  // k_walk_parallel flags the chunk
    const uint32_t len_w = (uint32_t)(end - begin);
    const uint32_t max_full = max_payload_words(chunk_geom(G, c).L);
    uint2 *clist = cand + c * kPwStride;
    // the slice's candidates are collected in LDS and appended with ONE global atomic (2000 atomics on one counter
    // cost 0.2 ms: same-address atomics serialise in the L2)
    __shared__ uint2 s_list[kPwCap / 4];
    __shared__ uint32_t s_n, s_base;
    if (tid == 0) s_n = 0;
    __syncthreads();
    auto consider = [&](uint32_t i, uint32_t v) __attribute__((always_inline)) {
        if (i >= 1u && i < len_w && v <= max_full) {
            const uint32_t k = atomicAdd(&s_n, 1u);
            if (k < kPwCap / 4) s_list[k] = make_uint2(i, v);
        }
    };
    // 16-byte loads, four in flight per thread (a dependent 4-byte load per word made this pass take as long as
    // the serial walk it replaces); quads are aligned, the first one may start below the chunk
    const uint32_t mis = (uint32_t)((((uintptr_t)in >> 2) + begin) & 3u);
    const uint32_t *q0 = in + begin - mis;  // words before `begin` are ignored by consider()
    const uint32_t n_quads = (len_w + mis + 3u) >> 2;
    const bool vec_ok = begin >= mis;
    const uint32_t per = (n_quads + parts - 1u) / parts;
    const uint32_t q_lo = part * per, q_hi = (q_lo + per < n_quads) ? q_lo + per : n_quads;
    constexpr uint32_t U = 4;
    for (uint32_t qb = q_lo + tid; qb < q_hi; qb += 256u * U) {
        uint4 v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t qi = qb + u * 256u;
            v[u] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            if (qi < q_hi) {
                const uint64_t w0 = begin - mis + 4ull * qi;  // absolute word index of the quad
                if (vec_ok && w0 + 4u <= in_words) {
                    v[u] = *reinterpret_cast<const uint4 *>(q0 + 4ull * qi);
                } else {
                    if (w0 + 0u < in_words && w0 + 0u >= begin) v[u].x = in[w0 + 0u];
                    if (w0 + 1u < in_words && w0 + 1u >= begin) v[u].y = in[w0 + 1u];
                    if (w0 + 2u < in_words && w0 + 2u >= begin) v[u].z = in[w0 + 2u];
                    if (w0 + 3u < in_words && w0 + 3u >= begin) v[u].w = in[w0 + 3u];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i0 = 4u * (qb + u * 256u) - mis;  // may wrap below zero for the first quad: consider() rejects
            consider(i0 + 0u, v[u].x);
            consider(i0 + 1u, v[u].y);
            consider(i0 + 2u, v[u].z);
            consider(i0 + 3u, v[u].w);
        }
    }
    __syncthreads();
    const uint32_t n_loc = s_n;
    if (n_loc > kPwCap / 4) {  // more candidates in one slice than a sane chunk has in four: let the serial walker judge
        if (tid == 0) atomicAdd(cand_count + c, kPwCap);
        return;
    }
    if (tid == 0) {
        s_base = atomicAdd(cand_count + c, n_loc);
        clist[kPwCap + part] = make_uint2(s_base, n_loc);  // k_walk_parallel puts the slices in order
    }
    __syncthreads();
    // written in position order inside the slice (rank by counting: a slice holds tens of candidates), so that
    // k_walk_parallel needs no sort
    const uint32_t b0 = s_base;
    for (uint32_t i = tid; i < n_loc; i += 256u) {
        const uint2 e = s_list[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < n_loc; ++j) r += s_list[j].x < e.x ? 1u : 0u;
        if (b0 + r < kPwCap) clist[b0 + r] = e;
    }
}

__global__ __launch_bounds__(kPwThreads) void k_walk_parallel(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                              const uint64_t *__restrict__ chunk_word_off,
                                                              uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                              uint32_t *__restrict__ fail, const uint32_t *__restrict__ list,
                                                              const uint2 *__restrict__ cand, const uint32_t *__restrict__ cand_count,
                                                              uint32_t parts) {
    __shared__ uint32_t pos[kPwCap];   // candidate positions relative to the chunk start; padding entries sort last
    __shared__ uint32_t val[kPwCap];
    __shared__ uint16_t up[kPwLevels][kPwCap];
    __shared__ uint32_t s_bad, s_start, s_first[kPwMaxParts], s_pre[kPwMaxParts + 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t c = list ? (uint64_t)list[blockIdx.x] : blockIdx.x;
    const ChunkGeom f = chunk_geom(G, c);
    const uint32_t W = f.W;
    const HeaderBounds hb = header_bounds(f.L, f.N, W, G.k);
    const uint64_t begin = chunk_word_off[c];
    const uint64_t end = chunk_word_off[c + 1];
    if (tid == 0) { s_bad = 0; s_start = 0xffffffffu; }
    __syncthreads();
    bool ok = chunk_extent_usable(begin, end, in_words, kParWalkMaxWords);
    if (ok && in[begin] != f.N) ok = false;
    if (!ok) { if (tid == 0) fail[c] = 1u; return; }  // (uniform across the workgroup)
    const uint32_t len_w = (uint32_t)(end - begin);  // words in the chunk
    const uint32_t nc = cand_count[c];
    if (nc > kPwCap - 2u || nc < W) { if (tid == 0) fail[c] = 1u; return; }
    // the candidates in position order: k_pw_scan's slices cover the chunk in order and each wrote its own in order, so the
    // slices only have to be put one behind the other (a bitonic sort of 4096 did this before: 78 barrier-separated stages)
    if (tid < 64u) {
        uint32_t run = 0;
        for (uint32_t s0 = 0; s0 < parts; s0 += 64u) {
            const uint32_t sl = s0 + tid;
            uint2 e = make_uint2(0u, 0u);
            if (sl < parts) e = cand[c * kPwStride + kPwCap + sl];
            const uint32_t incl = wave_running_prefix(e.y, run);
            if (sl < parts) { s_first[sl] = e.x; s_pre[sl + 1u] = incl; }
        }
        if (tid == 0) s_pre[0] = 0;
    }
    __syncthreads();
    if (s_pre[parts] != nc) { if (tid == 0) fail[c] = 1u; return; }  // (cannot happen: the slices' counts add up to it)
    uint32_t n_pad = 64u;  // the candidates and the two sentinel nodes
    while (n_pad < nc + 2u) n_pad <<= 1;
    for (uint32_t i = tid; i < n_pad; i += kPwThreads) {
        uint2 e = make_uint2(0xffffffffu, 0u);
        if (i < nc) {
            const uint32_t sl = slot_of(s_pre, parts, i);
            e = cand[c * kPwStride + s_first[sl] + (i - s_pre[sl])];
        }
        pos[i] = e.x;
        val[i] = e.y;
    }
    __syncthreads();
    // 2. links.  Nodes nc (END) and nc + 1 (INVALID) point to themselves.
    const uint32_t END = nc, INV = nc + 1u;
    for (uint32_t i = tid; i < n_pad; i += kPwThreads) {
        uint32_t to = i;  // padding and the two sentinels: self loops
        if (i < nc) {
            const uint64_t target = (uint64_t)pos[i] + val[i] + 1u;
            if (target == len_w) {
                to = END;
            } else if (target > len_w) {
                to = INV;
            } else {
                uint32_t lo = 0, hi = nc;  // first candidate with pos >= target
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (pos[mid] < (uint32_t)target) lo = mid + 1u; else hi = mid; }
                to = (lo < nc && pos[lo] == (uint32_t)target) ? lo : INV;
            }
            if (pos[i] == 1u) s_start = i;  // the first waveform's header follows the chunk header
        }
        up[0][i] = (uint16_t)to;
    }
    __syncthreads();
    // 3. binary lifting
    for (int k = 1; k < kPwLevels; ++k) {
        for (uint32_t i = tid; i < n_pad; i += kPwThreads) up[k][i] = up[k - 1][up[k - 1][i]];
        __syncthreads();
    }
    const uint32_t start = s_start;
    if (start == 0xffffffffu) { if (tid == 0) fail[c] = 1u; return; }
    bool bad = false;
    for (uint32_t w = tid; w < W; w += kPwThreads) {
        uint32_t node = start;
#pragma unroll
        for (int k = 0; k < kPwLevels; ++k)
            if ((w >> k) & 1u) node = up[k][node];
        if (node >= nc) { bad = true; continue; }
        const uint32_t n = val[node];
        if (!hb.ok(n, w + 1u == W)) { bad = true; continue; }
        if (w + 1u == W && up[0][node] != END) { bad = true; continue; }
        wave_off[f.base + w] = begin + pos[node];
        wave_words[f.base + w] = n;
    }
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (tid == 0 && s_bad) fail[c] = 1u;
}

// ---------------------------------------------------------------------------
// The chunk-wide walk WITHOUT reading the chunk: 64 chains per chunk, chased in parallel
// ---------------------------------------------------------------------------
// k_pw_scan reads every word of a chunk to find the ~2000 that are headers -- a second pass over the whole stream, 0.26 ms in
// front of a 1.2 ms decode at 100 chunks, 0.48 at 224.  A chain needs none of that: a header says where the next one is.  What
// a chain needs is a true header to START from, and those are easy to come by: a payload word practically never looks like
// a length header (n_i lies in a range of a few thousand out of 2^32), so the first plausible word at or behind ANY position
// is the next header.  The chunk is cut at 64 word positions; from each, one wavefront looks forward for the first plausible
// word (on average half a waveform's code away); then 64 lanes chase their chains at once, each until it arrives at the next
// lane's start -- which it must hit exactly: with lane 0 starting at the chunk's first header and the last chain ending at
// the chunk's end, the chain of equalities proves every start a true header, as in the block-parallel walk.  W / 64 dependent
// loads per lane instead of W, a few hundred KB read instead of the chunk.  Anything else (an impostor picked as a start, a
// broken chain, a count that is not W) flags the chunk for the scalar walker, which also judges it.
constexpr int kSwThreads = 1024;     // (at most: chunks of few waveforms get 256, the kernel strides by blockDim)
constexpr uint32_t kSwSegs = 64;    // chains per chunk
constexpr uint32_t kSwCap = 192;    // headers a chain may collect: chains are equal in WORDS, so one through quiet waveforms holds more than
                                    // the average W / 64 <= 56 -- up to 3.4 x (W = 2000: 6 x) before the scalar walker has to take the chunk; 48 KB of LDS
// it costs ~60 us per 512 chunks whatever their size: every uniform batch of long waveforms takes it, the headline's 500 chunks
// included (4.74 + 0.08 ms against 5.33 with the walk inside the launch)
constexpr uint64_t kSwMaxChunks = 1u << 20;
constexpr uint32_t kSwMinWaves = 8, kSwMaxWaves = 8192;  // ... chunks of 8 ... 8192 waveforms (the scan form: 64 ... kPwMaxWaves)

__global__ __launch_bounds__(kSwThreads) void k_walk_sparse(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                            const uint64_t *__restrict__ chunk_word_off,
                                                            uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                            uint32_t *__restrict__ fail, const uint32_t *__restrict__ list) {
    __shared__ uint32_t s_a[kSwSegs + 1];          // where chain s starts (word of the chunk); s_a[S] = the chunk's length
    __shared__ uint32_t s_cnt[kSwSegs], s_base[kSwSegs + 1];
    __shared__ uint32_t s_list[kSwSegs][kSwCap];   // position of every header a chain found (n_i = the distance to the next one - 1)
    __shared__ uint32_t s_bad;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wv = (uint32_t)wave_id();
    const uint64_t c = list ? (uint64_t)list[blockIdx.x] : blockIdx.x;
    const ChunkGeom f = chunk_geom(G, c);
    const uint32_t W = f.W;
    const uint64_t begin = chunk_word_off[c];
    const uint64_t end = chunk_word_off[c + 1];
    if (tid == 0) s_bad = 0;
    bool ok = chunk_extent_usable(begin, end, in_words, kParWalkMaxWords);
    if (ok && in[begin] != f.N) ok = false;
    if (!ok) { if (tid == 0) fail[c] = 1u; return; }  // (uniform across the workgroup)
    const uint32_t len_w = (uint32_t)(end - begin);
    const HeaderBounds hb = header_bounds(f.L, f.N, W, G.k);
    const uint32_t min_full = hb.min_full, max_full = hb.max_full, min_last = hb.min_last, max_last = hb.max_last;
    const uint32_t lo_any = min_full < min_last ? min_full : min_last, hi_any = max_full > max_last ? max_full : max_last;
    // chains: as many as give each a few waveforms -- and only where finding a start (half a waveform's code, read by one wavefront
    // 512 words at a time) costs less than the hops it saves: chunks of 32 x 500 000 samples are one chain of 32 hops
    uint32_t S = W / 8u;
    S = S > kSwSegs ? kSwSegs : (S < 1u ? 1u : S);
    if (len_w / W > 8192u) S = 1u;
    const uint32_t *cw = in + begin;  // the chunk's words
    // ---- 1. a start for every chain: the first plausible header at or behind its cut ----
    if (tid == 0) { s_a[0] = 1u; s_a[S] = len_w; }
    __syncthreads();  // (s_bad is cleared before any wavefront may raise it)
    auto plausible = [&](uint32_t v, uint32_t i) { return v >= lo_any && v <= hi_any && (uint64_t)i + 1u + v <= len_w; };
    for (uint32_t sg = 1u + wv; sg < S; sg += blockDim.x >> 6) {
        uint32_t from = 1u + (uint32_t)(((uint64_t)(len_w - 1u) * sg) / S);
        // (a waveform's code is at most hi_any words: a stream without a header in twice that is corrupt, and is not read to its end
        // by every cut)
        const uint32_t stop = (uint64_t)from + 2u * (hi_any + 2u) < len_w ? from + 2u * (hi_any + 2u) : len_w;
        uint32_t found = len_w;  // (none: the chains in front run to the chunk's end)
        for (uint32_t tries = 0; tries < 64u; ++tries) {
            constexpr uint32_t U = 8;
            found = len_w;
            for (uint32_t j0 = from; j0 < stop && found == len_w; j0 += 64u * U) {
                uint32_t v[U];
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t i = j0 + 64u * u + (uint32_t)lane;
                    v[u] = i < len_w ? cw[i] : 0xffffffffu;
                }
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint64_t m = __ballot(plausible(v[u], j0 + 64u * u + (uint32_t)lane));
                    if (m && found == len_w) found = j0 + 64u * u + (uint32_t)__builtin_ctzll(m);
                }
            }
            if (found >= stop) {  // (nothing in front of the stop)
                if (stop < len_w && lane == 0) atomicOr(&s_bad, 1u);
                found = len_w;
                break;
            }
            // a payload word is plausible once in a million, and this kernel looks at millions: a start counts only if the
            // word it points to is plausible too (or the chunk's end): one dependent load per cut
            const uint32_t nxt = found + 1u + rfl(cw[found]);  // (<= len_w: plausible())
            if (nxt == len_w || plausible(rfl(cw[nxt]), nxt)) break;
            from = found + 1u;
            found = len_w;
        }
        if (lane == 0) s_a[sg] = found;
    }
    __syncthreads();
    // ---- 2. the chases ----
    if (tid < S) {
        uint32_t pos = s_a[tid];
        const uint32_t target = s_a[tid + 1u];
        uint32_t cnt = 0;
        bool bad = false;
        while (pos < target) {
            const uint32_t n = cw[pos];  // (pos < len_w: inside the chunk, and the chunk inside the stream)
            if (n < lo_any || n > hi_any || cnt >= kSwCap) { bad = true; break; }
            s_list[tid][cnt] = pos;
            ++cnt;
            pos += n + 1u;  // (<= len_w + hi_any: no overflow, chunks have fewer than 2^31 words)
        }
        if (pos != target) bad = true;  // (a chain must arrive exactly where the next one started)
        s_cnt[tid] = cnt;
        if (bad) atomicOr(&s_bad, 1u);
    }
    __syncthreads();
    // ---- 3. waveform numbers, the tables ----
    if (tid < 64u) {
        const uint32_t cnt = tid < S ? s_cnt[tid] : 0u;
        const uint32_t incl = wave_incl_scan_dpp(cnt);
        s_base[tid] = incl - cnt;
        if (tid == 63u) s_base[64] = incl;
    }
    __syncthreads();
    if (s_bad || s_base[64] != W) { if (tid == 0) fail[c] = 1u; return; }
    bool bad = false;
    for (uint32_t sg = wv; sg < S; sg += blockDim.x >> 6) {
        const uint32_t cnt = rfl(s_cnt[sg]), b0 = rfl(s_base[sg]);
        for (uint32_t i = (uint32_t)lane; i < cnt; i += 64u) {
            const uint32_t at = s_list[sg][i];
            const uint32_t n = (i + 1u < cnt ? s_list[sg][i + 1u] : s_a[sg + 1u]) - at - 1u;  // (the chain arrived at the next one's start)
            const uint32_t w = b0 + i;
            if (!hb.ok(n, w + 1u == W)) bad = true;
            wave_off[f.base + w] = begin + at;
            wave_words[f.base + w] = n;
        }
    }
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (tid == 0 && s_bad) fail[c] = 1u;
}

// The same idea for chunks of SHORT waveforms (tens of thousands of headers per chunk: too many for one
// workgroup's LDS, and the chain chase through LDS still costs 0.13 us per hop, 3.6 ms for 14 M samples at
// L = 512).  A header is at most max_words = 25 L / 32 (400 for L = 512) and every B-word block of the stream with
// B > max_words holds at least one, so the BLOCKS become independent: a wavefront loads its block, takes the first word in
// [1, max_words] as the block's entry header, chases the chain through LDS to the block's end (if the chain breaks,
// the entry was an impostor: try the next small word), and reports {entry, headers, exit}.  k_bw_scan checks per
// chunk that every block's exit is the next block's entry (and word 1 / the chunk end at the two ends) and
// turns the counts into first-waveform indices; a second pass writes the table (k_bw_emit from the first pass's header lists, k_bw_chase by chasing again).  A chunk
// that does not stitch is flagged and walked by k_walk_block.
// Launch shape.  How many blocks a chunk really has is only known on the device (chunk_word_off), while the host can only
// bound it by 25 bits per sample, four times the usual: a grid with a workgroup per POSSIBLE block spent most of its time
// on empty workgroups, each holding its LDS for a few microseconds.  So the grid is a fixed number of wavefronts (as many as
// the LDS lets the chip hold) that stride over the REAL blocks, numbered through a prefix sum over the chunks' block
// counts that every wavefront computes for itself (at most kBwMaxList chunks).  B is the smallest of 1024 / 2048 / 4096
// that exceeds max_words: the chase is a chain of dependent LDS reads, so what hides it is wavefronts per CU, i.e.
// little LDS per block.  (A one-pass version -- blocks in ticket order, {headers, exit} through a decoupled look-back,
// table written straight from LDS -- was built and measured SLOWER than the two passes, 0.97 against 0.88 ms on config 5:
// the frontier of known prefixes advances one window of entries per memory round trip; profiles/r02_notes.md.)
constexpr uint32_t kBwTries = 6;  // impostors tolerated in front of a block's first real header
constexpr uint32_t kBwCandCap = 512;  // the fast path's room for a block's headers (more: the chase)
constexpr uint32_t kBwMaxList = 256;  // chunks per launch (bw_walk_blocks_max() / the plan admit at most 224)

struct BwBlock { uint32_t entry, count, exit, base; };

// pre[s] = real blocks of the listed chunks in front of chunk s (pre[n_list] = all); a chunk whose extent is unusable has
// none (k_bw_scan flags it), one longer than the host's bound is cut there (ditto)
template <uint32_t B>
__device__ __forceinline__ void bw_block_prefix(const uint64_t *__restrict__ chunk_word_off, uint64_t in_words,
                                                const uint32_t *__restrict__ list, uint32_t n_list, uint32_t blocks_max,
                                                uint32_t *pre, int lane) {
    uint32_t run = 0;
    for (uint32_t s0 = 0; s0 < n_list; s0 += 64u) {
        const uint32_t sl = s0 + (uint32_t)lane;
        uint32_t nb = 0;
        if (sl < n_list) {
            const uint64_t c = list ? (uint64_t)list[sl] : sl;
            const uint64_t begin = chunk_word_off[c], end = chunk_word_off[c + 1];
            if (chunk_extent_usable(begin, end, in_words, kParWalkMaxWords)) nb = (uint32_t)((end - begin + B - 1u) / B);
            if (nb > blocks_max) nb = blocks_max;
        }
        const uint32_t incl = wave_running_prefix(nb, run);
        if (sl < n_list) pre[sl + 1u] = incl;
    }
    if (lane == 0) pre[0] = 0;
    wave_sync();
}

// The block streamer of both passes.  A wavefront strides over the real blocks (pre[]: kBwMaxList + 1 words of LDS), a block at
// a time in blk (B words of LDS, 16-byte aligned) with the NEXT block's words in flight (registers) while body(unit, u) works
// on the current one: without that a unit was a chain of dependent latencies -- chunk table, 8 KB of loads, the LDS work, the
// stores -- of ~3.5 us, and 84 units per wavefront were the kernel's 0.3 ms on config 5 whatever the chase cost
// (profiles/r04_notes.md).  fail (optional): the chunks k_bw_scan gave up on, whose blocks are passed over.
struct BwUnit {
    bool ok;
    uint64_t begin;  // the chunk's first word
    ChunkGeom f;
    uint32_t b, b0, len_w, blk_len;  // block b of the chunk = its words [b0, b0 + blk_len), of len_w
};
template <uint32_t B, class Body>
__device__ __forceinline__ void bw_stream_blocks(const Geom &G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                 const uint64_t *__restrict__ chunk_word_off, const uint32_t *__restrict__ list,
                                                 uint32_t n_list, uint32_t blocks_max, const uint32_t *__restrict__ fail,
                                                 uint32_t *blk, uint32_t *pre, Body body) {
    constexpr int NV = B / 256;
    const int lane = lane_id();
    bw_block_prefix<B>(chunk_word_off, in_words, list, n_list, blocks_max, pre, lane);
    const uint32_t total = pre[n_list];
    uint32_t cached_slot = 0xffffffffu;
    BwUnit cached{};
    auto locate_unit = [&](uint32_t unit) __attribute__((always_inline)) {
        const uint32_t slot = slot_of(pre, n_list, unit);
        if (slot != cached_slot) {  // (a wavefront's consecutive units mostly lie in one chunk: its table entry is read once)
            cached_slot = slot;
            const uint64_t cc = list ? (uint64_t)list[slot] : slot;
            cached.f = chunk_geom(G, cc);
            cached.begin = chunk_word_off[cc];
            cached.len_w = (uint32_t)(chunk_word_off[cc + 1] - cached.begin);  // (a chunk with an unusable extent has no blocks)
            cached.ok = !(fail && fail[cc]);
        }
        BwUnit u = cached;
        u.b = unit - pre[slot];
        u.b0 = u.b * B;
        if (u.b0 >= u.len_w) u.ok = false;  // (only a chunk cut at the host's bound; flagged by k_bw_scan)
        u.blk_len = u.ok ? (u.len_w - u.b0 < B ? u.len_w - u.b0 : B) : 0u;
        return u;
    };
    // the block's words: unconditional 16-byte loads (any 4-byte alignment: a chunk starts anywhere) from an address clamped
    // into the stream; what the clamp moved and what lies behind the block is sorted out when the registers go to LDS
    const int64_t a_max = (int64_t)in_words - 4;
    auto fetch = [&](const BwUnit &u, uint4 (&v)[NV]) __attribute__((always_inline)) {
        const int64_t a0 = (int64_t)(u.begin + u.b0);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t a = a0 + (int64_t)((uint32_t)(j * 64 + lane) * 4u);
            const int64_t ac = a > a_max ? (a_max < 0 ? 0 : a_max) : a;
            v[j] = *reinterpret_cast<const uint4 *>(in + ac);
        }
    };
    auto store = [&](const BwUnit &u, const uint4 (&v)[NV]) __attribute__((always_inline)) {
        const uint64_t a0 = u.begin + u.b0;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const uint32_t i = (uint32_t)(j * 64 + lane) * 4u;
            uint4 w = v[j];
            if ((int64_t)(a0 + i) > a_max) {  // the clamp moved this piece (the last words of the batch): word by word
                auto ld = [&](uint64_t q) { return q < in_words ? in[q] : 0xffffffffu; };
                w = make_uint4(ld(a0 + i), ld(a0 + i + 1u), ld(a0 + i + 2u), ld(a0 + i + 3u));
            }
            w.x = (i + 0u < u.blk_len) ? w.x : 0xffffffffu;
            w.y = (i + 1u < u.blk_len) ? w.y : 0xffffffffu;
            w.z = (i + 2u < u.blk_len) ? w.z : 0xffffffffu;
            w.w = (i + 3u < u.blk_len) ? w.w : 0xffffffffu;
            *reinterpret_cast<uint4 *>(blk + i) = w;
        }
    };
    uint4 img[NV];
    BwUnit cur{};
    cur.ok = false;
    if (blockIdx.x < total) { cur = locate_unit(blockIdx.x); if (cur.ok) fetch(cur, img); }
    for (uint32_t unit = blockIdx.x; unit < total; unit += gridDim.x) {
        wave_sync();  // (the previous block's LDS reads are done)
        const BwUnit me = cur;
        if (me.ok) store(me, img);
        if (unit + gridDim.x < total) { cur = locate_unit(unit + gridDim.x); if (cur.ok) fetch(cur, img); }
        if (!me.ok) continue;
        wave_sync();
        body(unit, me);
    }
}

// Which of the four words v at positions i ... i + 3 of a block may be headers: in [1, max_full], at or behind `from`.  Never
// 0: a waveform has at least one payload word, while the zero-padded LAST word of a waveform is all zeros whenever its final
// code ends in zero bits -- an impostor that would chain straight into the real header behind it
struct Small4 { bool x, y, z, w; };
__device__ __forceinline__ Small4 small_words(const uint4 &v, uint32_t i, uint32_t from, uint32_t blk_len, uint32_t max_full) {
    auto small = [&](uint32_t word, uint32_t at) { return at >= from && at < blk_len && word - 1u < max_full; };
    return Small4{small(v.x, i + 0u), small(v.y, i + 1u), small(v.z, i + 2u), small(v.w, i + 3u)};
}

// First pass: a block's entry header, the number of its headers and where its chain leaves it -> info[unit]; LIST: its
// headers, {position in the block | n << 12}, -> hops[unit * hop_cap ...] for k_bw_emit
template <uint32_t B, bool LIST>
__global__ __launch_bounds__(64) void k_bw_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                  const uint64_t *__restrict__ chunk_word_off, const uint32_t *__restrict__ list,
                                                  uint32_t n_list, uint32_t blocks_max, BwBlock *__restrict__ info,
                                                  uint32_t *__restrict__ hops, uint32_t hop_cap) {
    __shared__ __attribute__((aligned(16))) uint32_t blk[B];
    __shared__ uint16_t cand[kBwCandCap];  // the fast path's candidates, in position order
    __shared__ uint32_t pre[kBwMaxList + 1];
    const int lane = lane_id();
    bw_stream_blocks<B>(G, in, in_words, chunk_word_off, list, n_list, blocks_max, nullptr, blk, pre, [&](uint32_t unit, const BwUnit &u) __attribute__((always_inline)) {
        const uint32_t b0 = u.b0, len_w = u.len_w, blk_len = u.blk_len;
        const uint32_t max_full = max_payload_words(u.f.L), min_words = min_payload_words(u.f.L, G.k);
        const uint32_t from0 = u.b == 0 ? 1u : 0u;  // (word 0 of the chunk is its sample count: block 0 starts at word 1)
        // FAST PATH.  A payload word is 32 bits of dense code: it lies in [1, max_words] (400 for WaveformLength
        // 512) about once in ten million words, so the block's words in that range ARE its headers, nearly always.  All of
        // them are found at once (the block is read 16 bytes per lane and step, as below), put in position order by ballots,
        // and held to the chain's own equalities in parallel: every candidate's position + n + 1 must be the next
        // candidate's position, the last one's must leave the block.  One impostor (or a header beyond the list's room)
        // and the block takes the chase below.  The chase is one lane following ~20 dependent LDS reads per
        // 2048-word block while 63 lanes wait: 0.13 us per hop, 0.33 ms for config 5's 278 000 blocks (profiles/r04_notes.md section 5).
        uint32_t ncand = 0;
        bool overflow = false;
        for (uint32_t base = 0; base < blk_len; base += 256u) {
            const uint32_t i = base + 4u * (uint32_t)lane;
            const uint4 v = *reinterpret_cast<const uint4 *>(blk + i);  // (all B words were written by the streamer)
            const Small4 f = small_words(v, i, from0, blk_len, max_full);
            const uint64_t m0 = __ballot(f.x), m1 = __ballot(f.y), m2 = __ballot(f.z), m3 = __ballot(f.w);
            if ((m0 | m1 | m2 | m3) == 0ull) continue;
            const uint64_t below = (1ull << lane) - 1ull;
            // candidates of lower lanes come first, then this lane's own in component order
            uint32_t r = ncand + (uint32_t)(__builtin_popcountll(m0 & below) + __builtin_popcountll(m1 & below) +
                                            __builtin_popcountll(m2 & below) + __builtin_popcountll(m3 & below));
            if (f.x) { if (r < kBwCandCap) cand[r] = (uint16_t)(i + 0u); ++r; }
            if (f.y) { if (r < kBwCandCap) cand[r] = (uint16_t)(i + 1u); ++r; }
            if (f.z) { if (r < kBwCandCap) cand[r] = (uint16_t)(i + 2u); ++r; }
            if (f.w) { if (r < kBwCandCap) cand[r] = (uint16_t)(i + 3u); ++r; }
            ncand += (uint32_t)(__builtin_popcountll(m0) + __builtin_popcountll(m1) + __builtin_popcountll(m2) + __builtin_popcountll(m3));
            overflow = overflow || ncand > kBwCandCap;
        }
        wave_sync();
        bool fast = ncand != 0u && !overflow && (!LIST || ncand <= hop_cap);
        uint32_t exit_rel = 0;
        if (fast) {
            bool bad = false;
            for (uint32_t j0 = 0; j0 < ncand; j0 += 64u) {
                const uint32_t j = j0 + (uint32_t)lane;
                if (j < ncand) {
                    const uint32_t pos = cand[j], n = blk[pos], nxt = pos + n + 1u;
                    // (as in the chase: the waveform must end inside the chunk; LIST: not below 1 + k bits per sample
                    // unless it is the chunk's last)
                    if ((uint64_t)b0 + nxt > len_w) bad = true;
                    if (LIST && n < min_words && b0 + nxt != len_w) bad = true;
                    if (j + 1u < ncand) { if (nxt != (uint32_t)cand[j + 1u]) bad = true; }
                    else { if (nxt < blk_len) bad = true; exit_rel = nxt; }
                }
            }
            fast = !__any(bad);
        }
        if (fast) {
            exit_rel = (uint32_t)__builtin_amdgcn_readlane((int)exit_rel, (int)((ncand - 1u) & 63u));
            if (LIST) {
                for (uint32_t j = (uint32_t)lane; j < ncand; j += 64u) {
                    const uint32_t pos = cand[j];
                    hops[(uint64_t)unit * hop_cap + j] = pos | (blk[pos] << 12);
                }
            }
            if (lane == 0) info[unit] = BwBlock{b0 + (uint32_t)cand[0], ncand, b0 + exit_rel, 0u};
            return;
        }
        // THE CHASE.  Candidates in position order: the first small word at or after `from`, 256 words per step
        uint32_t from = from0;
        uint32_t entry = 0xffffffffu, count = 0, exit_pos = 0;
        bool found = false;
        for (uint32_t t = 0; t < kBwTries && !found; ++t) {
            uint32_t first = 0xffffffffu;
            for (uint32_t base = from & ~255u; base < blk_len; base += 256u) {
                const uint32_t i = base + 4u * (uint32_t)lane;
                const Small4 s = small_words(*reinterpret_cast<const uint4 *>(blk + i), i, from, blk_len, max_full);
                uint32_t f = 0xffffffffu;
                if (s.w) f = i + 3u;
                if (s.z) f = i + 2u;
                if (s.y) f = i + 1u;
                if (s.x) f = i + 0u;
                first = ~wave_max_u32(~f);  // minimum over the wave
                if (first != 0xffffffffu) break;
            }
            if (first == 0xffffffffu) break;
            // chase from `first` to the block's end
            uint32_t rel = first, cnt = 0;
            bool ok = true;
            while (rel < blk_len) {
                const uint32_t n = __builtin_amdgcn_readfirstlane(blk[rel]);
                // (n == 0 is no waveform: at least one bit per sample; it also bounds the headers of a block by B / 2)
                if (n - 1u >= max_full || (uint64_t)b0 + rel + 1u + n > len_w) { ok = false; break; }
                if (LIST) {
                    // the header list for k_bw_emit: {position in the block, n}.  Its capacity counts on at least 1 + k
                    // bits per sample (min_words) for every waveform but the chunk's last, shorter one
                    if ((n < min_words && b0 + rel + 1u + n != len_w) || cnt >= hop_cap) { ok = false; break; }
                    if (lane == 0) hops[(uint64_t)unit * hop_cap + cnt] = rel | (n << 12);
                }
                rel += n + 1u;
                ++cnt;
            }
            if (ok) { found = true; entry = first; count = cnt; exit_pos = b0 + rel; }
            else from = first + 1u;
        }
        if (lane == 0) info[unit] = BwBlock{found ? b0 + entry : 0xffffffffu, count, exit_pos, 0u};
    });
}

// Second pass where the first one kept no header lists: chase again from the entry k_bw_scan accepted, then write the
// block's part of the table
template <uint32_t B>
__global__ __launch_bounds__(64) void k_bw_chase(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                 const uint64_t *__restrict__ chunk_word_off, const uint32_t *__restrict__ list,
                                                 uint32_t n_list, uint32_t blocks_max, const BwBlock *__restrict__ info,
                                                 const uint32_t *__restrict__ fail, uint64_t *__restrict__ wave_off,
                                                 uint32_t *__restrict__ wave_words, DevStatus *st) {
    __shared__ __attribute__((aligned(16))) uint32_t blk[B];
    __shared__ uint16_t hop[B / 2];  // header positions inside the block (a waveform has at least one payload word)
    __shared__ uint32_t pre[kBwMaxList + 1];
    const int lane = lane_id();
    bw_stream_blocks<B>(G, in, in_words, chunk_word_off, list, n_list, blocks_max, fail, blk, pre, [&](uint32_t unit, const BwUnit &u) __attribute__((always_inline)) {
        const BwBlock me = info[unit];
        if (me.entry == 0xffffffffu) return;  // a last block without a header (k_bw_scan)
        const HeaderBounds hb = header_bounds(u.f.L, u.f.N, u.f.W, G.k);
        uint32_t rel = me.entry - u.b0, n_hops = 0;
        while (rel < u.blk_len) {
            const uint32_t n = __builtin_amdgcn_readfirstlane(blk[rel]);
            if (lane == 0) hop[n_hops] = (uint16_t)rel;
            rel += n + 1u;
            ++n_hops;
        }
        wave_sync();
        for (uint32_t i = (uint32_t)lane; i < n_hops; i += 64u) {
            const uint32_t pos = hop[i], n = blk[pos], wi = me.base + i;  // (k_bw_scan accepted the chunk: wi < W)
            wave_off[u.f.base + wi] = u.begin + u.b0 + pos;
            wave_words[u.f.base + wi] = n;
            // the first pass held n to [1, max_words] only: no header may be below the minimum of 1 + k bits per sample, and the
            // chunk's last waveform may be shorter than the rest, with tighter bounds
            if (!hb.ok(n, wi + 1u == u.f.W)) atomicOr(&st->err, kErrCorrupt);
        }
    });
}

// one wavefront per chunk: stitch the blocks, first-waveform index of every block, verdict
template <uint32_t B>
__global__ __launch_bounds__(64) void k_bw_scan(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                const uint64_t *__restrict__ chunk_word_off, const uint32_t *__restrict__ list,
                                                uint32_t n_list, uint32_t blocks_max, BwBlock *__restrict__ info,
                                                uint32_t *__restrict__ fail) {
    __shared__ uint32_t pre[kBwMaxList + 1];
    const int lane = lane_id();
    bw_block_prefix<B>(chunk_word_off, in_words, list, n_list, blocks_max, pre, lane);
    const uint64_t slot = blockIdx.x;
    const uint64_t c = list ? (uint64_t)list[slot] : slot;
    const ChunkGeom f = chunk_geom(G, c);
    const uint64_t begin = chunk_word_off[c], end = chunk_word_off[c + 1];
    bool bad = !chunk_extent_usable(begin, end, in_words, kParWalkMaxWords);
    if (!bad && in[begin] != f.N) bad = true;
    const uint32_t len_w = bad ? 0u : (uint32_t)(end - begin);
    const uint32_t n_blocks = (len_w + B - 1u) / B;
    if (n_blocks > blocks_max) bad = true;
    BwBlock *my = info + pre[slot];
    uint32_t run = 0;
    uint32_t carry_exit = 1u;  // where the block in front of this group of 64 left (the first header follows the chunk's)
    // (four groups' records in flight: one wavefront per chunk, 88 groups for config 5's chunks -- a dependent 16-byte load per
    // group was the kernel's whole time, 0.065 ms)
    constexpr uint32_t UG = 4;
    for (uint32_t g0 = 0; g0 < n_blocks && !bad; g0 += 64u * UG) {
        BwBlock og[UG];
#pragma unroll
        for (uint32_t u = 0; u < UG; ++u) {
            const uint32_t b = g0 + 64u * u + (uint32_t)lane;
            og[u] = BwBlock{0xffffffffu, 0, 0, 0};
            if (b < n_blocks) og[u] = my[b];
        }
#pragma unroll
        for (uint32_t u = 0; u < UG; ++u) {
            const uint32_t b0 = g0 + 64u * u;
            if (b0 >= n_blocks || bad) break;  // (wave uniform)
            const uint32_t b = b0 + (uint32_t)lane;
            BwBlock o = og[u];
            // every block must have been entered, start where its predecessor left, and the ends must be the chunk's
            uint32_t prev_exit = (uint32_t)__shfl_up((int)o.exit, 1);
            if (lane == 0) prev_exit = carry_exit;
            carry_exit = (uint32_t)__builtin_amdgcn_readlane((int)o.exit, 63);
            bool lane_bad = false;
            if (b < n_blocks) {
                if (b + 1u == n_blocks && b > 0u && prev_exit == len_w) {
                    // the chain already ended inside the previous block: the last block is the tail of the last payload and
                    // has no header of its own (whatever small word it may hold is not one)
                    o.count = 0;
                    my[b].entry = 0xffffffffu;
                    my[b].count = 0;
                } else {
                    lane_bad = o.entry == 0xffffffffu || o.entry != prev_exit;
                    if (b + 1u == n_blocks && o.exit != len_w) lane_bad = true;
                }
            }
            if (__any(lane_bad)) { bad = true; break; }
            const uint32_t inc = wave_running_prefix(b < n_blocks ? o.count : 0u, run);
            if (b < n_blocks) my[b].base = inc - o.count;
        }
    }
    if (!bad && run != f.W) bad = true;
    // (the last waveform may be shorter: its header has a tighter bound than the blocks checked; the second pass holds it to it)
    if (lane == 0) fail[c] = bad ? 1u : 0u;
}

// Second pass where the first one left the header list (bw_hop_cap() != 0): a wavefront per block, striding over the real
// blocks as above, copies {position, n} into the table at the index k_bw_scan gave the block.  No LDS, no second read of
// the stream, no second chase (config 5: 0.185 -> 0.03 ms).
template <uint32_t B>
__global__ __launch_bounds__(256) void k_bw_emit(Geom G, uint64_t in_words, const uint64_t *__restrict__ chunk_word_off,
                                                 const uint32_t *__restrict__ list, uint32_t n_list, uint32_t blocks_max,
                                                 const BwBlock *__restrict__ info, const uint32_t *__restrict__ fail,
                                                 const uint32_t *__restrict__ hops, uint32_t hop_cap,
                                                 uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words, DevStatus *st) {
    __shared__ uint32_t pre[kBwMaxList + 1];
    const int lane = lane_id();
    const uint32_t wv = threadIdx.x >> 6;
    if (wv == 0) bw_block_prefix<B>(chunk_word_off, in_words, list, n_list, blocks_max, pre, lane);
    __syncthreads();
    const uint32_t total = pre[n_list];
    // A LANE per block (a wavefront per block before): a block holds ~20 headers, so 44 lanes of a wavefront had
    // nothing to do, and every block paid its chain of dependent loads (list, table entry, info) alone -- 0.12-0.14 ms on
    // config 5 for 11 MB of table.  64 blocks' chains now travel together (profiles/r04_notes.md).
    for (uint32_t unit = blockIdx.x * 256u + threadIdx.x; unit < total; unit += gridDim.x * 256u) {
        const uint32_t slot = slot_of(pre, n_list, unit), b = unit - pre[slot];
        const uint64_t c = list ? (uint64_t)list[slot] : slot;
        if (fail[c]) continue;
        const BwBlock me = info[unit];
        if (me.entry == 0xffffffffu) continue;  // a last block without a header (k_bw_scan)
        const ChunkGeom f = chunk_geom(G, c);
        const uint64_t at = chunk_word_off[c] + (uint64_t)b * B;
        const uint32_t *hp = hops + (uint64_t)unit * hop_cap;
        for (uint32_t i = 0; i < me.count; ++i) {
            const uint32_t h = hp[i], pos = h & 0xfffu, n = h >> 12, wi = me.base + i;
            wave_off[f.base + wi] = at + pos;
            wave_words[f.base + wi] = n;
            // the chunk's last waveform may be shorter than the rest: its header has tighter bounds (the others were held
            // to [min, max] by the first pass)
            if (wi + 1u == f.W && !header_bounds(f.L, f.N, f.W, G.k).ok(n, true)) atomicOr(&st->err, kErrCorrupt);
        }
    }
}

// Side-band decode (drx_decode_with_wave_words): the caller hands over the n_i table an encode left behind (SURVEY section 7:
// "reuse its offset table as a side-band"), so no header chain is walked.  Per chunk: header positions by a prefix sum over
// 1 + n_i, each checked against the stream itself (the word at that position must BE n_i, n_i within the bounds of its
// waveform, the chain must end exactly at the chunk's end, the chunk header must be the sample count) -- a table that does
// not belong to the stream is DRX_ERR_CORRUPT, never a wild read.  list (optional): the chunks to do, one per workgroup
// (drx_decode_select_with_wave_words: the chunks its selection touches; the others are not looked at).
__global__ __launch_bounds__(256) void k_sideband_tables(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                         const uint64_t *__restrict__ chunk_word_off,
                                                         const uint32_t *__restrict__ n_in, uint64_t *__restrict__ wave_off,
                                                         uint32_t *__restrict__ wave_words, DevStatus *st,
                                                         const uint32_t *__restrict__ list) {
    __shared__ uint64_t wsum[4];
    const uint64_t c = list ? (uint64_t)list[blockIdx.x] : blockIdx.x;
    const int lane = lane_id(), wv = wave_id();
    const ChunkGeom f = chunk_geom(G, c);
    const uint32_t W = f.W;
    const uint64_t base = f.base;
    const HeaderBounds hb = header_bounds(f.L, f.N, W, G.k);
    const uint64_t off0 = chunk_word_off[c], off1 = chunk_word_off[c + 1];
    // (its own, weaker extent test -- not chunk_extent_usable(): every position is checked against [off0, off1) below)
    bool bad = off1 > in_words || off0 >= off1;  // (the same in every lane here; block-wide after every round below)
    uint64_t run = 1;  // the chunk header word
    for (uint32_t i0 = 0; i0 < W; i0 += 256) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t n = (i < W) ? n_in[base + i] : 0u;
        // An entry outside the bounds of its waveform never enters the prefix sum (64-bit: 256 entries of up to 25 bits per
        // sample of a 2^31-sample waveform do not fit 32), so no later position can wrap below off0 or past 2^64; and the
        // whole chunk is rejected before any lane looks at the stream.
        const bool n_ok = i >= W || hb.ok(n, i + 1u == W);
        const uint64_t v = (i < W && n_ok) ? (uint64_t)n + 1u : 0u;
        uint64_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wv] = inc;
        bad = __syncthreads_or(bad || !n_ok) != 0;
        uint64_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint64_t s = rfl64(wsum[w]); before += (w < wv) ? s : 0u; all += s; }
        bool mine_bad = bad;
        if (i < W) {
            const uint64_t at = off0 + run + before + inc - v;
            if (!mine_bad && (at <= off0 || at >= off1 || at + 1u + n > off1)) mine_bad = true;
            if (!mine_bad && in[at] != n) mine_bad = true;
            // a rejected entry is left pointing at the chunk's own header with no payload words: the decode launch behind
            // this one runs whatever the status says, and reads nothing through such an entry
            wave_off[base + i] = mine_bad ? off0 : at;
            wave_words[base + i] = mine_bad ? 0u : n;
        }
        run += all;
        bad = __syncthreads_or(mine_bad) != 0;  // (also keeps wsum until every lane has read it)
    }
    if (threadIdx.x == 0 && !bad && (off0 + run != off1 || in[off0] != f.N)) bad = true;
    if (bad && threadIdx.x == 0) atomicOr(&st->err, kErrCorrupt);
}


// ---------------------------------------------------------------------------
// host side: which walk takes a batch, the parallel walks' scratch, the launchers
// ---------------------------------------------------------------------------
// (the limits of each parallel walk: with its kernels above)
// The chunk-wide walk takes such a chunk: the one place that spells its range
static bool chunk_wide_walk_takes(uint32_t n_waves, uint32_t wave_len) {
    return wave_len > kWalkShortLen && n_waves >= kSwMinWaves && n_waves <= kSwMaxWaves;
}

// drx_decode_select sorts the chunks its selection touches into three lists (launch_select_walk()): 0 = long waveforms, 8 ...
// 8192 of them: the chunk-wide walk by chains; 1 = WaveformLength <= kWalkShortLen: the LDS block walker, a wavefront per chunk;
// 2 = the rest (a few very long waveforms, or more than 8192 long ones): one lane per chunk, hop by hop
int select_walk_class(uint32_t n_waves, uint32_t wave_len) {
    if (wave_len <= kWalkShortLen) return 1;
    return chunk_wide_walk_takes(n_waves, wave_len) ? 0 : 2;
}

// The block-parallel walk of a batch's chunks, each of n_waves waveforms of wave_len samples (from 16), pays against the walk
// inside the decode launch (serial chase through LDS, 0.13 us per waveform of a chunk, all chunks at once, so that large
// batches hide most of it) while it walks no more chunks than one per 35 waveforms of a chunk.  Measured (chunks of 14 M
// samples, decode GB/s of the two paths at 150 / 220 chunks): L = 512 1602 / 1627 against 875 / 1265; L = 1024 1869 / 1927
// against 1521 / 1954; L = 2048 1906 / 2012 against 1673 / 2169.  Above WaveformLength 2048 the alternative is the scalar
// chain at 0.85 us per hop (L = 3072, 100 / 220 chunks: 1731 / 1459+ against 596 / 1123): one per 18.
static bool bw_walk_pays(uint64_t walked_chunks, uint32_t n_waves, uint32_t wave_len) {
    return walked_chunks <= n_waves / (wave_len <= kWalkShortLen ? 35u : 18u) && wave_len >= 16u;
}
// ... the 4096-word blocks of such a chunk: its code at 25 bits per sample with its headers, at most kBwMaxBlocks
constexpr uint64_t kBwMaxBlocks = 0xfffffu;
static uint64_t bw_chunk_blocks(uint32_t n_samples, uint32_t n_waves) {
    return (chunk_max_words(n_samples, n_waves) + kWalkBlockWords - 1u) / kWalkBlockWords;
}
// ... of a uniform batch (0: the block-parallel walk does not take it)
static uint32_t bw_walk_blocks_max(const Geom &G) {
    // every 4096-word block must hold a header: n_i <= 25 L / 32 < 4096, i.e. L <= 5000; chunks of longer
    // waveforms within the chunk-wide walk's capacity take that one
    if (!(G.uniform && bw_walk_pays(G.n_chunks, G.u_n_waves, G.u_wave_len) && G.n_chunks <= kPwMaxChunks && G.u_wave_len <= 5000u &&
          !chunk_wide_walk_takes(G.u_n_waves, G.u_wave_len))) return 0;
    const uint64_t nb = bw_chunk_blocks(G.u_n_samples, G.u_n_waves);
    return nb > kBwMaxBlocks ? 0u : (uint32_t)nb;
}

// workgroups that scan one chunk: enough of them to fill the chip when the chunks are few (one chunk of 2000 x 7000, what an
// H5Z call brings: 128 instead of 16 took the walk from 0.113 to 0.070 ms, k_pw_scan itself 9 us)
static uint32_t pw_parts(uint32_t n_chunks) { return n_chunks <= 4u ? 128u : (n_chunks <= 32u ? 32u : 16u); }

// capacity of a block's header list (0: the batch keeps the second chase): B-word blocks hold at most B / (min_words + 1)
// headers + the chunk's last.  Waveforms of fewer than 32 words keep the second chase: one lane's store per header costs
// more than it saves there (100 chunks of 14 M samples, walk with lists / with the second chase: L = 64 2.85 / 2.44 ms,
// 128 1.59 / 1.44, 512 0.64 / 0.73, 1024 0.48 / 0.64, 2048 0.45 / 0.68, 3072 0.55 / 0.97)
static uint32_t bw_hop_cap(uint32_t B, uint32_t min_len, uint32_t k) {
    const uint32_t mw = min_payload_words(min_len, k);
    if (mw < 32u || B > 4096u) return 0u;
    return B / (mw + 1u) + 2u;
}

// The parallel walks a batch takes, over which chunks, in what shape, and their scratch behind `base` -- a function of the
// geometry alone (never of debug flags), so that the plan's allocation (base == nullptr: no pointers, the byte count; 0: the
// batch takes neither walk) and every launch agree:
//   uint2 cand[n_chunks * kPwStride]   the scan form's candidate lists (only where that form may run)
//   uint32 cnt | pw_fail | bw_fail     n_chunks each: candidate counters, the chunks each walk gave up on (walk_scratch_reset())
//   BwBlock info[blocks]               the block-parallel walk's records, sized for blocks of 1024 words, the smallest
//   uint32 hops[blocks * bw_hop_cap]   ... and the header lists of its first pass (nullptr: none kept, bw_hop_cap())
struct ParWalks {
    bool pw, bw;                        // the chunk-wide walk, the block-parallel walk
    const uint32_t *pw_list, *bw_list;  // their chunks (nullptr: every chunk of the batch)
    uint32_t n_pw, n_bw;
    uint32_t bw_blocks_max;  // 4096-word blocks of the block-parallel walk's largest chunk at 25 bits per sample
    // its block size: the smallest of 1024 / 2048 / 4096 that exceeds every walked chunk's max_words (the chase is a chain of
    // dependent LDS reads: what hides it is wavefronts per CU, as many as the LDS lets the chip hold); bw_hop_cap() of that size
    uint32_t bw_B, bw_waves_per_cu, bw_hop_cap;
    uint2 *cand;
    uint32_t *cnt, *pw_fail, *bw_fail;
    BwBlock *info;
    uint32_t *hops;
    uint64_t bytes;
};
static ParWalks par_walks(const Geom &G, void *base) {
    ParWalks P{};
    if (G.uniform) {
        P.bw_blocks_max = bw_walk_blocks_max(G);
        P.bw = P.bw_blocks_max != 0;
        P.pw = G.n_chunks <= kSwMaxChunks && chunk_wide_walk_takes(G.u_n_waves, G.u_wave_len);  // (never both: bw_walk_blocks_max())
        P.n_pw = P.n_bw = (uint32_t)G.n_chunks;
    } else if (G.rag_par) {  // (walk_plan_ragged())
        P.pw = G.n_long != 0;
        P.bw = G.n_short != 0;
        P.pw_list = G.walk_long;
        P.bw_list = G.walk_short;
        P.n_pw = G.n_long;
        P.n_bw = G.n_short;
        P.bw_blocks_max = G.rag_bw_blocks_max;
    }
    if (!P.pw && !P.bw) return P;
    const uint32_t max_full = max_payload_words(G.uniform ? G.u_wave_len : kWalkShortLen);
    P.bw_B = max_full + 2u <= 1024u ? 1024u : (max_full + 2u <= 2048u ? 2048u : 4096u);
    P.bw_waves_per_cu = P.bw_B == 1024u ? 24u : (P.bw_B == 2048u ? 13u : 7u);
    P.bw_hop_cap = bw_hop_cap(P.bw_B, G.uniform ? G.u_wave_len : G.rag_bw_min_len, G.k);
    auto take = [&](uint64_t bytes) {
        char *p = base ? (char *)base + P.bytes : nullptr;
        P.bytes += bytes;
        return p;
    };
    const uint64_t n = G.n_chunks, bw_units = P.bw ? (uint64_t)P.n_bw * P.bw_blocks_max : 0;
    P.cand = (uint2 *)take(P.pw && n <= kPwMaxChunks ? n * kPwStride * sizeof(uint2) : 0);
    P.cnt = (uint32_t *)take(n * sizeof(uint32_t));
    P.pw_fail = (uint32_t *)take(n * sizeof(uint32_t));
    P.bw_fail = (uint32_t *)take((n + (n & 1u)) * sizeof(uint32_t));  // (info[] on an 8-byte boundary)
    P.info = (BwBlock *)take(bw_units * (kWalkBlockWords / 1024u) * sizeof(BwBlock));
    P.hops = (uint32_t *)take(bw_units * (kWalkBlockWords / P.bw_B) * P.bw_hop_cap * sizeof(uint32_t));
    if (!P.bw_hop_cap) P.hops = nullptr;
    return P;
}
uint64_t walk_scratch_bytes(const Geom &G) { return par_walks(G, nullptr).bytes; }
hipError_t walk_scratch_reset(const Geom &G, void *d_pw, hipStream_t s) {
    return hipMemsetAsync(par_walks(G, d_pw).cnt, 0, 3u * G.n_chunks * sizeof(uint32_t), s);
}

std::vector<uint32_t> walk_plan_ragged(Geom &G, const ChunkDesc *d) {
    const uint64_t n = G.n_chunks;
    // walk lists: chunks of short waveforms are walked through LDS, the others hop by hop
    std::vector<uint32_t> lists;
    for (uint64_t c = 0; c < n; ++c) if (d[c].wave_len <= kWalkShortLen) lists.push_back((uint32_t)c);
    G.n_short = (uint32_t)lists.size();
    for (uint64_t c = 0; c < n; ++c) if (d[c].wave_len > kWalkShortLen) lists.push_back((uint32_t)c);
    G.n_long = (uint32_t)lists.size() - G.n_short;
    // parallel header walks for small ragged batches: every long-waveform chunk within the chunk-wide walk's capacity, every
    // short-waveform chunk worth the block-parallel walk (bw_walk_pays(), bw_chunk_blocks(): the rules of uniform batches).
    // NOT chunk_wide_walk_takes(): a long-waveform chunk of a ragged batch is held to the scan form's kPwMaxWaves and to no
    // minimum (the fewest waveforms any of them has goes to rag_pw_min_waves, from which route_walk() chooses the form).  The
    // bound dates from the scan form, the only one at the time; uniform batches got the wider 8 ... 8192 with the chain walk
    // (da4efd2), ragged ones were left as they were.
    bool ok = G.n_long <= kPwMaxChunks && G.n_short <= kPwMaxChunks;
    uint64_t bmax = 0;
    uint32_t min_len = 0xffffffffu, min_long_waves = 0xffffffffu;
    for (uint64_t c = 0; c < n && ok; ++c) {
        if (d[c].wave_len > kWalkShortLen) {
            ok = d[c].n_waves <= kPwMaxWaves;
            min_long_waves = std::min(min_long_waves, d[c].n_waves);
        } else {
            ok = bw_walk_pays(G.n_short, d[c].n_waves, d[c].wave_len);
            bmax = std::max(bmax, bw_chunk_blocks(d[c].n_samples, d[c].n_waves));
            min_len = std::min(min_len, d[c].wave_len);
        }
    }
    G.rag_par = ok && bmax <= kBwMaxBlocks;
    G.rag_bw_blocks_max = (uint32_t)bmax;
    G.rag_bw_min_len = min_len;
    G.rag_pw_min_waves = min_long_waves;
    return lists;
}

// ---------------------------------------------------------------------------
// Which walk runs in front of a decoder (route_decode() in drx_decode_kernels.hip chooses the decoder, and the walk inside the
// lanes launch where no parallel walk takes the batch):
//
//   walk          | when (never with tables_ready: the caller filled wave_off / wave_words)
//   --------------+-----------------------------------------------------------------------------------
//   chunk-wide    | chunks of 8 ... 8192 waveforms longer than 2048 samples (uniform, any number of chunks: k_walk_sparse chases 64 chains per
//                 | chunk without reading it -- the headline batch too), the long-waveform chunks of a small ragged batch
//   block-parallel| bw_walk_blocks_max(): few chunks of many short waveforms (uniform), the short-waveform chunks of a small ragged batch
//   serial        | otherwise: LDS block walkers (WaveformLength <= 2048) / scalar chains, one launch in front of the decoder
//   chunk-wide by chains (k_walk_sparse), or by reading the chunks (k_pw_scan + k_walk_parallel) for one to four chunks of 64 ...
//   kPwMaxWaves waveforms.
// Flags (DRX_DBG_*): NO_PARALLEL_WALKS, WALK_BY_SCAN and WALK_BY_CHAINS (where the other form is the default).
// ---------------------------------------------------------------------------
WalkRoute route_walk(const Geom &G, bool tables_ready, bool have_scratch) {
    WalkRoute R{};
    if (tables_ready || !have_scratch || (G.dbg & DRX_DBG_NO_PARALLEL_WALKS)) return R;
    const ParWalks P = par_walks(G, nullptr);
    R.chunk_wide = P.pw;
    R.blocks = P.bw;
    // (up to four chunks the scan form is quicker: 128 workgroups read one chunk in 11 us, where a chain is 31 dependent loads;
    // so for ragged chunks of a few very long waveforms: a start costs half a waveform's code in reads)
    const bool few_waves = G.uniform && (G.u_n_waves < 64u || G.u_n_waves > kPwMaxWaves);  // (outside the scan form's range)
    const bool chains_suit = (G.dbg & DRX_DBG_WALK_BY_CHAINS) || few_waves || ((G.uniform ? G.n_chunks : G.n_long) > 4u && (G.uniform || G.rag_pw_min_waves >= 64u));
    R.by_chains = (!(G.dbg & DRX_DBG_WALK_BY_SCAN) && chains_suit) || G.n_chunks > kPwMaxChunks || few_waves;
    return R;
}

// ---------------------------------------------------------------------------
// launchers.  Each sequence exists once and takes an optional chunk list (nullptr: every chunk of the batch); a failed launch
// is the caller's hipGetLastError().
// ---------------------------------------------------------------------------
hipError_t launch_sideband_tables(const StreamCall &c, const uint32_t *d_n, const uint32_t *d_list, uint32_t n_list) {
    const Geom &G = *c.G;
    if (G.total_waves == 0 || (d_list && !n_list)) return hipSuccess;
    k_sideband_tables<<<d_list ? n_list : (unsigned)G.n_chunks, 256, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, d_n, c.d_wave_off,
                                                                            c.d_wave_words, c.d_status, d_list);
    return hipGetLastError();
}

// The chunk-wide walk over n chunks, then the scalar walker for the chunks it flagged in fail (uint32[n_chunks], zeroed by the
// caller), which also judges them.  chain_threads != 0: 64 chains per chunk chased in parallel from starts found by looking
// forward from 64 cuts, by workgroups of so many threads (the chunk is not read); 0: the scan form, candidates in cand / cnt.
static void walk_chunk_wide(const StreamCall &c, const uint32_t *d_list, uint32_t n, unsigned chain_threads, uint2 *cand, uint32_t *cnt,
                            uint32_t *fail) {
    const Geom &G = *c.G;
    if (chain_threads) {
        k_walk_sparse<<<n, chain_threads, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off, c.d_wave_words, fail, d_list);
    } else {
        const uint32_t parts = pw_parts(n);
        k_pw_scan<<<(unsigned)(n * parts), 256, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, d_list, cand, cnt, parts);
        k_walk_parallel<<<n, kPwThreads, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off, c.d_wave_words, fail, d_list, cand, cnt, parts);
    }
    k_walk_scalar_only<<<blocks_for(G.n_chunks, kWalkChains), 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off,
                                                                            c.d_wave_words, c.d_status, fail);
}
void launch_walk_chunk_wide(const StreamCall &c, bool by_chains) {
    const Geom &G = *c.G;
    const ParWalks P = par_walks(G, c.d_pw);
    const unsigned chain_threads = (G.uniform && G.u_n_waves < 256u) ? 256u : (unsigned)kSwThreads;  // (few chains: few wavefronts)
    walk_chunk_wide(c, P.pw_list, P.n_pw, by_chains ? chain_threads : 0u, P.cand, P.cnt, P.pw_fail);
}

// The block-parallel walk over the batch's short-waveform chunks, then the LDS block walker for the chunks it flagged
void launch_walk_blocks(const StreamCall &c) {
    const Geom &G = *c.G;
    const ParWalks P = par_walks(G, c.d_pw);
    const uint32_t *list = P.bw_list;
    const uint32_t n = P.n_bw;
    auto run_bw = [&](auto btag) {
        constexpr uint32_t B = decltype(btag)::value;
        const uint32_t bmax = P.bw_blocks_max * (kWalkBlockWords / B);
        const unsigned grid = 256u * P.bw_waves_per_cu;
        // (one argument list for both forms of the first pass: without lists P.hops is nullptr and P.bw_hop_cap 0, a placeholder
        // that stays -- a kernel without the two parameters would be a second signature for the same body)
        if (P.hops)
            k_bw_blocks<B, true><<<grid, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, list, n, bmax, P.info, P.hops, P.bw_hop_cap);
        else
            k_bw_blocks<B, false><<<grid, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, list, n, bmax, P.info, P.hops, P.bw_hop_cap);
        k_bw_scan<B><<<n, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, list, n, bmax, P.info, P.bw_fail);
        if (P.hops)
            k_bw_emit<B><<<256u * 8u, 256, 0, c.s>>>(G, c.in_words, c.d_chunk_word_off, list, n, bmax, P.info, P.bw_fail, P.hops, P.bw_hop_cap, c.d_wave_off, c.d_wave_words, c.d_status);
        else
            k_bw_chase<B><<<grid, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, list, n, bmax, P.info, P.bw_fail, c.d_wave_off, c.d_wave_words, c.d_status);
    };
    if (P.bw_B == 1024u) run_bw(std::integral_constant<uint32_t, 1024>{});
    else if (P.bw_B == 2048u) run_bw(std::integral_constant<uint32_t, 2048>{});
    else run_bw(std::integral_constant<uint32_t, 4096>{});
    k_walk_block_only<<<(unsigned)G.n_chunks, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off, c.d_wave_words, c.d_status, P.bw_fail);
}

// The serial walk: chunks of short waveforms streamed through LDS, a wavefront per chunk; chunks of long waveforms one
// dependent load per hop, a lane per chunk (d_long == nullptr: every chunk of the batch, by scalar loads)
static void walk_serial(const StreamCall &c, const uint32_t *d_short, uint32_t n_short, const uint32_t *d_long, uint32_t n_long) {
    const Geom &G = *c.G;
    if (n_short)
        k_walk_block<<<n_short, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, d_short, n_short, c.d_wave_off, c.d_wave_words, c.d_status);
    if (n_long && d_long)
        k_walk_list<<<blocks_for(n_long, 64), 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, d_long, n_long, c.d_wave_off, c.d_wave_words, c.d_status);
    else if (n_long)
        k_walk_scalar<<<blocks_for(G.n_chunks, kWalkChains), 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_chunk_word_off, c.d_wave_off, c.d_wave_words, c.d_status);
}
void launch_walk_serial(const StreamCall &c) {
    const Geom &G = *c.G;
    if (!G.uniform) return walk_serial(c, G.walk_short, G.n_short, G.walk_long, G.n_long);
    const uint32_t n = (uint32_t)G.n_chunks, n_short = G.u_wave_len <= kWalkShortLen ? n : 0u;
    walk_serial(c, nullptr, n_short, nullptr, n - n_short);
}

// The walk in front of a call that reads the whole batch behind it, on one stream
hipError_t launch_batch_walk(const StreamCall &c) {
    const WalkRoute R = route_walk(*c.G, false, c.d_pw != nullptr);
    if (R.chunk_wide || R.blocks) {
        const hipError_t e = walk_scratch_reset(*c.G, c.d_pw, c.s);
        if (e != hipSuccess) return e;
        if (R.chunk_wide) launch_walk_chunk_wide(c, R.by_chains);
        if (R.blocks) launch_walk_blocks(c);
    } else {
        launch_walk_serial(c);
    }
    return hipGetLastError();
}

// The walk in front of drx_decode_select: the chunks its selection touches and no others.  d_lists = the three lists of
// select_walk_class() back to back; d_fail: uint32[n_chunks], cleared here.  Always by chains, in workgroups of kSwThreads.
hipError_t launch_select_walk(const StreamCall &c, const uint32_t *d_lists, uint32_t n_sparse, uint32_t n_block, uint32_t n_chain,
                              uint32_t *d_fail) {
    if (n_sparse) {
        const hipError_t e = hipMemsetAsync(d_fail, 0, c.G->n_chunks * sizeof(uint32_t), c.s);
        if (e != hipSuccess) return e;
        walk_chunk_wide(c, d_lists, n_sparse, kSwThreads, nullptr, nullptr, d_fail);
    }
    walk_serial(c, d_lists + n_sparse, n_block, d_lists + n_sparse + n_block, n_chain);
    return hipGetLastError();
}

}  // namespace drx
