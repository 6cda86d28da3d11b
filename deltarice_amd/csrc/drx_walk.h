// drx_walk.h -- the header-chain walkers that run INSIDE a kernel (scalar chains, one lane per chunk; the LDS block walker, a
// wave per chunk of short waveforms): device functions and their constants, shared by drx_walk.hip (the walk kernels in front
// of the decoders and all the host decides about the walk) and drx_decode_kernels.hip (k_decode_lanes' first tickets walk).
// In front of them what every walker shares: the extent rule with its two limits, the granule's layout, the table entry.
#ifndef DRX_WALK_H
#define DRX_WALK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "drx_internal.h"
#include "drx_device.h"

namespace drx {

// A chunk's extent [begin, end) of the stream is usable by a walker if it lies inside the stream, holds the sample count and
// one header at least, and is no longer than max_words.  The parallel walks keep 32-bit positions and add a header's n + 1 to
// them before they look at the sum, so they stop at 2^31 - 1 words; the serial walkers count in 64 bits and are held to
// 2^32 - 1 only by the granule's 32-bit position -- a chunk in between is flagged by a parallel walk and judged by its serial fallback.
constexpr uint64_t kParWalkMaxWords = 0x7fffffffull, kSerialWalkMaxWords = 0xffffffffull;
__device__ __forceinline__ bool chunk_extent_usable(uint64_t begin, uint64_t end, uint64_t in_words, uint64_t max_words) {
    return !(end > in_words || begin + 2 > end || end - begin > max_words);
}

// granules (optional): one 8-byte word per waveform, {valid:1 | n_i:31 | header position relative to
// the chunk start:32}, stored with one agent-scope relaxed atomic each -- the word is its own flag
// (it is zero until written), so a decoder wave in the SAME launch can consume waveform w of a
// chunk while the walk of that chunk is still at waveform w+1.
constexpr uint64_t kGranValid = 1ull << 63;
__device__ __forceinline__ uint32_t granule_words(uint64_t gr) { return (uint32_t)(gr >> 32) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t granule_pos(uint64_t gr) { return (uint32_t)gr; }

// Waveform i's table entry: its header at word `here` of the stream, n payload words (and its granule, the chunk starting at `begin`)
__device__ __forceinline__ void store_entry(uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                            uint64_t *__restrict__ granules, uint64_t i, uint64_t begin, uint64_t here, uint32_t n) {
    wave_off[i] = here;
    wave_words[i] = n;
    if (granules)
        __hip_atomic_store(granules + i, kGranValid | ((uint64_t)n << 32) | (uint64_t)(uint32_t)(here - begin), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
// ... of a rejected waveform: it points at the chunk's own header with no words (keeps later loads in bounds; decoded as zero
// words), its granule a bare kGranValid
__device__ __forceinline__ void store_rejected(uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                               uint64_t *__restrict__ granules, uint64_t i, uint64_t begin) {
    store_entry(wave_off, wave_words, granules, i, begin, begin, 0u);
}

// Header chain walk (:320-325) with validation; one lane per chunk.
__device__ __forceinline__ void walk_chunk(const Geom &G, uint64_t c, const uint32_t *__restrict__ in,
                                           uint64_t in_words, const uint64_t *__restrict__ chunk_word_off,
                                           uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                           uint64_t *__restrict__ granules, DevStatus *st) {
    const ChunkGeom f = chunk_geom(G, c);
    const HeaderBounds hb = header_bounds(f.L, f.N, f.W, G.k);
    const uint64_t begin = chunk_word_off[c];
    uint64_t end = chunk_word_off[c + 1];
    bool bad = false;
    if (!chunk_extent_usable(begin, end, in_words, kSerialWalkMaxWords)) { bad = true; end = begin; }
    if (!bad && in[begin] != f.N) bad = true;  // :306 totalNumberPoints
    uint64_t at = begin + 1;
    for (uint32_t w = 0; w < f.W; ++w) {
        uint32_t n = 0;
        uint64_t here = at;
        if (!bad && at < end) {
            n = in[at];
            if (!hb.ok(n, w + 1 == f.W) || at + 1u + n > end) { bad = true; n = 0; }
            else at += (uint64_t)n + 1u;
        } else {
            bad = true;
            here = begin;
        }
        store_entry(wave_off, wave_words, granules, f.base + w, begin, here, n);
    }
    if (!bad && at != end) bad = true;
    if (bad) atomicOr(&st->err, kErrCorrupt);
}

// The same walk for kWalkChains chunks of a uniform batch per wavefront (lanes 0..kWalkChains-1), with the
// header loads issued as SCALAR loads (s_load_dword through the scalar cache): under the decode's
// ~3.6 TB/s of vector traffic a dependent vector load takes ~2.9 us per hop (it queues behind the other
// waves' 64-line gathers in the CU's vector memory pipeline) and the chain becomes the critical path of
// the fused launch; the scalar path does not share that queue.
constexpr int kWalkChains = 8;

__device__ __forceinline__ void walk_chunks_scalar(const Geom &G, uint64_t c0, const uint32_t *__restrict__ list,
                                                   uint64_t n_list, const uint32_t *__restrict__ in,
                                                   uint64_t in_words, const uint64_t *__restrict__ chunk_word_off,
                                                   uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                   uint64_t *__restrict__ granules, DevStatus *st,
                                                   const uint32_t *__restrict__ only = nullptr) {
    // lanes 0..kWalkChains-1 take entries c0.. of the chunk list (list == nullptr: chunk index = entry);
    // only != nullptr: just the chunks it flags (the ones k_walk_parallel gave up on)
    const int lane = lane_id();
    const uint64_t e = c0 + (uint64_t)lane;
    bool mine = lane < kWalkChains && e < n_list;
    const uint64_t c = mine ? (list ? (uint64_t)list[e] : e) : 0;
    if (only && mine && !only[c]) mine = false;
    if (only && !__any(mine)) return;
    const ChunkGeom f = mine ? chunk_geom(G, c) : ChunkGeom{0u, 1u, 0u, 0ull};
    const uint32_t W = f.W;
    const HeaderBounds hb = header_bounds(f.L, f.N, W, G.k);
    const uint32_t W_max = wave_max_u32(W);
    uint64_t begin = 0, end = 0;
    bool bad = false;
    if (mine) {
        begin = chunk_word_off[c];
        end = chunk_word_off[c + 1];
        if (!chunk_extent_usable(begin, end, in_words, kSerialWalkMaxWords)) { bad = true; end = begin; }
    }
    if (in_words == 0) {  // nothing to load from (every chunk is bad)
        if (mine) {
            for (uint32_t w = 0; w < W; ++w) store_rejected(wave_off, wave_words, granules, f.base + w, begin);
            atomicOr(&st->err, kErrCorrupt);
        }
        return;
    }
    // word `a` of the stream for lanes 0..kWalkChains-1 (a < in_words), one scalar load per chain
    auto sload = [&](uint64_t a) __attribute__((always_inline)) -> uint32_t {
        static_assert(kWalkChains == 8, "the asm block below issues eight loads");
        uint64_t p[kWalkChains];
#pragma unroll
        for (int i = 0; i < kWalkChains; ++i) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)a, i);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(a >> 32), i);
            p[i] = (uint64_t)(uintptr_t)(in + (((uint64_t)hi << 32) | lo));
        }
        uint32_t v0, v1, v2, v3, v4, v5, v6, v7;
        // one block: all eight loads in flight before the wait (left to itself the compiler waits after seven)
        asm volatile(
            "s_load_dword %0, %8, 0x0\n\ts_load_dword %1, %9, 0x0\n\ts_load_dword %2, %10, 0x0\n\t"
            "s_load_dword %3, %11, 0x0\n\ts_load_dword %4, %12, 0x0\n\ts_load_dword %5, %13, 0x0\n\t"
            "s_load_dword %6, %14, 0x0\n\ts_load_dword %7, %15, 0x0\n\ts_waitcnt lgkmcnt(0)"
            : "=&s"(v0), "=&s"(v1), "=&s"(v2), "=&s"(v3), "=&s"(v4), "=&s"(v5), "=&s"(v6), "=&s"(v7)
            : "s"(p[0]), "s"(p[1]), "s"(p[2]), "s"(p[3]), "s"(p[4]), "s"(p[5]), "s"(p[6]), "s"(p[7])
            : "memory");
        const uint32_t v[kWalkChains] = {v0, v1, v2, v3, v4, v5, v6, v7};
        uint32_t r = 0;
#pragma unroll
        for (int i = 0; i < kWalkChains; ++i) r = (lane == i) ? v[i] : r;
        return r;
    };
    const uint32_t head = sload((mine && !bad) ? begin : 0ull);
    if (mine && !bad && head != f.N) bad = true;  // :306 totalNumberPoints
    uint64_t at = begin + 1;
    for (uint32_t w = 0; w < W_max; ++w) {
        const bool live = mine && w < W;  // chunks of a ragged batch differ in their number of waveforms
        const bool can = live && !bad && at < end;
        const uint32_t nn = sload(can ? at : 0ull);
        uint32_t n = 0;
        uint64_t here = at;
        if (can) {
            n = nn;
            if (!hb.ok(n, w + 1 == W) || at + 1u + n > end) { bad = true; n = 0; }
            else at += (uint64_t)n + 1u;
        } else if (live) {
            bad = true;
            here = begin;
        }
        if (live) store_entry(wave_off, wave_words, granules, f.base + w, begin, here, n);
    }
    if (mine && !bad && at != end) bad = true;
    if (mine && bad) atomicOr(&st->err, kErrCorrupt);
}

// Header-chain walk for chunks of SHORT waveforms (one wavefront per chunk).  With n_i of a few
// hundred words a chunk holds tens of thousands of waveforms and the per-hop HBM round trip of
// walk_chunk() adds up to tens of milliseconds (27 343 hops for 14 M samples at L = 512).  Here the
// wave streams the chunk through a 16 KB LDS block with coalesced 16-byte loads and lane 0 chases the
// chain inside LDS (~0.07 us per hop); the price is one extra read of the chunk's stream.
constexpr uint32_t kWalkBlockWords = 4096;
constexpr uint32_t kWalkShortLen = 2048;  // WaveformLength up to which a chunk is walked through LDS

constexpr uint32_t kWalkHopCap = 1024;   // hops buffered in LDS between coalesced flushes
constexpr int kChasePad = 15;            // k_walk_block, k_walk_block_only: PAD of walk_chunk_block()

// blk: kWalkBlockWords words (16-byte aligned), hop: kWalkHopCap entries, both in LDS and private to the wave.
// PAD >= 0 holds the chase loop where it is fast (below: the two kernels of drx_walk.hip); -1: left to the compiler (k_decode_lanes).
template <int PAD = -1>
__device__ __forceinline__ void walk_chunk_block(const Geom &G, uint64_t c, const uint32_t *__restrict__ in,
                                                 uint64_t in_words, const uint64_t *__restrict__ chunk_word_off,
                                                 uint64_t *__restrict__ wave_off, uint32_t *__restrict__ wave_words,
                                                 uint64_t *__restrict__ granules, DevStatus *st, uint32_t *blk, uint2 *hop) {
    constexpr uint32_t B = kWalkBlockWords;
    constexpr int NV = B / 256;  // 16-byte loads per lane and block
    const int lane = lane_id();
    const ChunkGeom f = chunk_geom(G, c);
    const uint32_t W = f.W;
    const uint64_t base = f.base;
    const HeaderBounds hb = header_bounds(f.L, f.N, W, G.k);
    const uint64_t begin = chunk_word_off[c];
    uint64_t end = chunk_word_off[c + 1];
    bool bad = false;
    if (!chunk_extent_usable(begin, end, in_words, kSerialWalkMaxWords)) { bad = true; end = begin; }
    if (!bad && in[begin] != f.N) bad = true;
    // blocks on a fixed grid from g0 (16-byte aligned when the stream is), so that block k + 1 can be
    // requested before the chase through block k starts
    const bool vec_ok = ((uintptr_t)in & 15u) == 0;
    const uint64_t g0 = begin & ~3ull;
    uint64_t at = begin + 1;  // header of waveform w (wave uniform)
    uint32_t w = 0;
    uint4 pre[NV];
    uint64_t pre_b0 = ~0ull;  // block the registers hold
    auto request = [&](uint64_t b0) __attribute__((always_inline)) {
        pre_b0 = b0;
        if (vec_ok && b0 + B <= end) {
#pragma unroll
            for (int j = 0; j < NV; ++j) pre[j] = *reinterpret_cast<const uint4 *>(in + b0 + (uint32_t)(j * 64 + lane) * 4u);
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const uint64_t i = b0 + (uint32_t)(j * 64 + lane) * 4u;
                uint4 v;
                v.x = (i + 0u < end) ? in[i + 0u] : 0u;
                v.y = (i + 1u < end) ? in[i + 1u] : 0u;
                v.z = (i + 2u < end) ? in[i + 2u] : 0u;
                v.w = (i + 3u < end) ? in[i + 3u] : 0u;
                pre[j] = v;
            }
        }
    };
    if (!bad) request(g0);
    // Where the chase below lies in a 64-byte line of code decides its speed: k_walk_block takes 3.55 ms with the loop's backward
    // branch landing 56 bytes into a line, 3.87 with it four bytes earlier (25 chunks of 14 M samples at L = 512; measured,
    // profiles/walk_refactor_ab.txt section 3c), and left to the compiler the place moves with any change in front of it.  PAD
    // >= 0: the code from here on starts on a line of its own plus PAD s_nop, run once per chunk (tests/test_walk_build.py).
    if constexpr (PAD >= 0) asm volatile(".p2align 6\n\t.rept %0\n\ts_nop 0\n\t.endr" : : "n"(PAD));
    while (w < W && !bad && at < end) {
        const uint64_t b0 = g0 + (at - g0) / B * B;
        if (pre_b0 != b0) request(b0);  // a hop longer than a block skipped the requested one
#pragma unroll
        for (int j = 0; j < NV; ++j) *reinterpret_cast<uint4 *>(blk + (uint32_t)(j * 64 + lane) * 4u) = pre[j];
        wave_sync();
        if (b0 + B < end) request(b0 + B);
        const uint32_t blk_len = (end - b0 < B) ? (uint32_t)(end - b0) : B;
        // the chunk's end relative to the block, clamped to 32 bits (b0 may lie three words below begin)
        const uint32_t end_rel = (end - b0 < 0xffffffffu) ? (uint32_t)(end - b0) : 0xffffffffu;
        uint32_t rel = (uint32_t)(at - b0);
        while (w < W && rel < blk_len && !bad) {
            // chase up to kWalkHopCap hops inside the block; every value here is wave uniform (SGPRs)
            const uint32_t w0 = w;
            uint32_t hops = 0;
            while (w < W && rel < blk_len && hops < kWalkHopCap) {
                const uint32_t n = __builtin_amdgcn_readfirstlane(blk[rel]);
                if (!hb.ok(n, w + 1 == W) || rel + 1u + n > end_rel) { bad = true; break; }
                hop[hops] = make_uint2(rel, n);
                rel += n + 1u;
                ++w;
                ++hops;
            }
            wave_sync();
            for (uint32_t i = lane; i < hops; i += 64) {
                const uint2 h = hop[i];
                store_entry(wave_off, wave_words, granules, base + w0 + i, begin, b0 + h.x, h.y);
            }
            wave_sync();
        }
        at = b0 + rel;
    }
    if (w < W) bad = true;
    if (!bad && at != end) bad = true;
    if (bad) {
        for (uint32_t i = w + lane; i < W; i += 64) store_rejected(wave_off, wave_words, granules, base + i, begin);
        if (lane == 0) atomicOr(&st->err, kErrCorrupt);
    }
}

}  // namespace drx
#endif
