// drx_device.h -- device-side helpers shared by the kernel translation units (not installed).
#ifndef DRX_DEVICE_H
#define DRX_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_internal.h"

namespace drx {

// ---------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// Wave-uniform values the compiler does not keep in scalar registers: it cannot prove threadIdx.x >> 6 uniform, so
// everything addressed or computed through the wave index is divergent to it; and the result of an LDS or vector-memory
// load arrives in a VGPR even where the address is provably uniform.  Read such a value from lane 0 into scalar registers
// at its SOURCE (the wave index, the word published through LDS), so that what is computed from it -- indices, bit counts,
// limits, loop and branch conditions -- is scalar code and the branches are s_cbranch, not exec-mask regions; a load whose
// address the compiler already knows to be uniform needs nothing.  ONLY for values that are
// uniform by construction: kernel arguments, blockIdx, threadIdx.x >> 6, readlane results, and a word that every lane of
// the wavefront loads from the same address behind the barrier or wave_sync() that orders its write.  Never for anything
// per lane: the other 63 values are dropped without a trace.
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) { return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v); }
__device__ __forceinline__ int wave_id() { return (int)rfl(threadIdx.x >> 6); }  // wavefront of the workgroup (1-D blocks)

__device__ __forceinline__ void wave_sync() {
    // All lanes of a wave run in lock step and its LDS operations complete in order;
    // this only stops the compiler from moving LDS accesses across a phase boundary.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        uint32_t t = __shfl_xor(v, d);
        v = t > v ? t : v;
    }
    return v;
}

// Bounds on a waveform's payload word count n_i: a code has between 1 + k (q = 0, src/deltaRice.c:215-222) and 25 bits
// (escape, :223-228).  Every walker rejects a header outside [min, max]: the chain of a valid stream never leaves them.
__host__ __device__ __forceinline__ uint32_t max_payload_words(uint32_t len) { return (uint32_t)(((uint64_t)len * 25u + 31u) >> 5); }
__host__ __device__ __forceinline__ uint32_t min_payload_words(uint32_t len, uint32_t k) {
    return (uint32_t)(((uint64_t)len * (k + 1u) + 31u) >> 5);
}
// ... of the headers of one chunk of W waveforms of L samples, N in all: the full waveforms' and the shorter last one's
struct HeaderBounds {
    uint32_t min_full, max_full, min_last, max_last;
    __host__ __device__ __forceinline__ bool ok(uint32_t n, bool is_last) const {
        return !(n > (is_last ? max_last : max_full) || n < (is_last ? min_last : min_full));
    }
};
__host__ __device__ __forceinline__ HeaderBounds header_bounds(uint32_t L, uint32_t N, uint32_t W, uint32_t k) {
    // (a chunk without waveforms has no last one.  The guard stands on the two RESULTS: on last_len the compiler turns ok() into
    // the bounds of a selected length, worked out again for every header: the LDS block walker's hop 0.13 -> 0.15 us, profiles/walk_refactor_ab.txt section 3b)
    const uint32_t last_len = N - (W - 1u) * L;
    return HeaderBounds{min_payload_words(L, k), max_payload_words(L), W ? min_payload_words(last_len, k) : 0u,
                        W ? max_payload_words(last_len) : 0u};
}

// count-leading-zeros with the ISA's result for 0 (-1) instead of the source language's undefined behaviour: the
// decoders meet an all-zero window only past the end of a corrupt stream, where any value will do, but it has to BE a value
__device__ __forceinline__ uint32_t ffbh(uint32_t x) {
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// A row of N int64 results: by 16-byte stores where the caller found the row 16-byte aligned (vec), by 8-byte stores
// otherwise (the ABI asks 8-byte alignment of such outputs)
template <int N>
__device__ __forceinline__ void store_i64_row(int64_t *__restrict__ row, bool vec, const int64_t (&v)[N]) {
    static_assert(N % 2 == 0, "whole 16-byte stores");
    if (vec) {
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        typedef u32x4v __attribute__((address_space(1))) g_uint4;
        g_uint4 *dst = (g_uint4 *)row;
#pragma unroll
        for (int j = 0; j < N / 2; ++j)
            dst[j] = (u32x4v){(uint32_t)v[2 * j], (uint32_t)((uint64_t)v[2 * j] >> 32), (uint32_t)v[2 * j + 1], (uint32_t)((uint64_t)v[2 * j + 1] >> 32)};
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) row[j] = v[j];
    }
}

struct WaveRef {
    uint64_t chunk;       // chunk index
    uint64_t sample_off;  // first sample of this waveform in the raw batch
    uint32_t idx;         // waveform index inside its chunk
    uint32_t len;         // samples in this waveform
    uint32_t n_samples;   // samples in the chunk
};

// waveform g -> chunk and extent.  Uniform batches are pure arithmetic; ragged
// batches bisect the chunk table (once per waveform, i.e. once per ~L samples).
__device__ __forceinline__ WaveRef locate(const Geom &G, uint64_t g) {
    WaveRef r;
    uint32_t L, W;
    uint64_t c, soff;
    if (G.uniform) {
        c = g / G.u_n_waves;
        r.idx = (uint32_t)(g - c * G.u_n_waves);
        L = G.u_wave_len;
        W = G.u_n_waves;
        r.n_samples = G.u_n_samples;
        soff = c * (uint64_t)G.u_n_samples;
    } else {
        uint64_t lo = 0, hi = G.n_chunks;  // invariant: wave_base[lo] <= g < wave_base[hi]
        while (hi - lo > 1) {
            uint64_t mid = (lo + hi) >> 1;
            if (G.chunks[mid].wave_base <= g) lo = mid; else hi = mid;
        }
        c = lo;
        const ChunkDesc d = G.chunks[c];
        r.idx = (uint32_t)(g - d.wave_base);
        L = d.wave_len;
        W = d.n_waves;
        r.n_samples = d.n_samples;
        soff = d.sample_off;
    }
    r.chunk = c;
    r.sample_off = soff + (uint64_t)r.idx * L;
    r.len = (r.idx + 1 == W) ? (r.n_samples - r.idx * L) : L;  // trailing partial waveform (:420-425)
    return r;
}
// chunk c -> its frame: W waveforms of L samples (the last one shorter), N samples in all, `base` = its first waveform's index
// in the batch's tables.  (The walks' one spelling of the uniform / ragged branch; the other kernels still carry their own.)
struct ChunkGeom {
    uint32_t W, L, N;
    uint64_t base;
};
__device__ __forceinline__ ChunkGeom chunk_geom(const Geom &G, uint64_t c) {
    if (G.uniform) return ChunkGeom{G.u_n_waves, G.u_wave_len, G.u_n_samples, c * G.u_n_waves};
    const ChunkDesc d = G.chunks[c];
    return ChunkGeom{d.n_waves, d.wave_len, d.n_samples, d.wave_base};
}
// the same for a wave-uniform g: the result in scalar registers (the ragged form reads the chunk table)
__device__ __forceinline__ WaveRef locate_uniform(const Geom &G, uint64_t g) {
    WaveRef r = locate(G, rfl64(g));
    r.chunk = rfl64(r.chunk);
    r.sample_off = rfl64(r.sample_off);
    r.idx = rfl(r.idx);
    r.len = rfl(r.len);
    r.n_samples = rfl(r.n_samples);
    return r;
}

// inclusive prefix sum over the 64 lanes (DPP: row shifts, then row broadcasts)
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return v;
}

// v of the lane below; lane 0 receives the wave-uniform `first` (one v_writelane from a scalar register, where a select
// on lane == 0 costs a move and a v_cndmask)
__device__ __forceinline__ uint32_t wave_shr1_carry(uint32_t v, uint32_t first) {
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);  // wave_shr:1
    asm("v_writelane_b32 %0, %1, 0" : "+v"(r) : "s"(rfl(first)));
    return r;
}

__device__ __forceinline__ uint32_t lds_addr(const uint32_t *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t *)p;
}

}  // namespace drx
#endif
