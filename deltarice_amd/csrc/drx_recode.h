// drx_recode.h -- what the kernels that write an encoded batch from an encoded batch share, a LANE per waveform: the re-code
// kernels (drx_transcode.hip: another RiceParameter, the residuals as they are) and the re-filter kernels (drx_refilter.hip:
// another prediction filter as well, a stage of arithmetic between the parse and the sink).  The parse over the shared reader
// (parse_lane()), which waveform a lane takes (recode_lane_wave()), the lane's output ring with its emit and flush (OutRing), and
// the two bodies -- recode_sizes() and recode_pack() -- over a value map: map(z) receives the canonical zig-zag value of every
// sample of the lane's waveform in order and returns the value that is sized or coded.  SameValue is drx_transcode's.
// Device code; included by the .hip units.  Not installed.
#ifndef DRX_RECODE_H
#define DRX_RECODE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_blocks.h"

namespace drx {

namespace {

constexpr int kOW = 32;      // output ring words per lane
constexpr int kOL = 16;      // words per output segment: half a line, 64 bytes
// the output ring is looked at once per group: a lane holds at most kFlushAt - 1 words then, a group adds at most 13.  (A ring of
// 64 words written out in whole 128-byte lines leaves the LDS room for four wavefronts per CU instead of six and was measured
// 40 % slower, 15.7 against 11.2 ms on the headline batch: DESIGN.md section 4.2g)
constexpr uint32_t kFlushAt = 20;
static_assert(kFlushAt - 1 + (kGS * 25 + 31) / 32 <= kOW && kFlushAt >= kOL, "output ring slack");
constexpr int kOutRingWords = kOW * 64;

// the residuals as they are: drx_transcode's value map
struct SameValue {
    __device__ __forceinline__ uint32_t operator()(uint32_t z) const { return z; }
};

// The parse of one waveform per lane over the shared reader (drx_lane_reader.inc): sink(z) receives the canonical zig-zag value
// of every sample in order, group_end() runs once per group of kGS samples with the whole wavefront converged.  Returns whether
// the lane's codes ended in its last payload word.  ring: the wavefront's ring_all + 64, S: the payload's first word, n: its
// words, k: the stream's parameter.
template <typename Sink, typename GroupEnd>
__device__ __forceinline__ bool parse_lane(uint32_t *__restrict__ ring, const uint32_t *__restrict__ in, uint64_t in_words, uint64_t S,
                                           uint32_t n, uint32_t len, uint32_t k, int lane, Sink &&sink, GroupEnd &&group_end) {
#include "drx_lane_reader.inc"
    // the int16 residual the decoders take from a code, as its zig-zag value: below k = 13 an ordinary code's value fits 15 bits
    // and an escape's sixteen payload bits ARE it (the extraction leaves 8 << 16 above them)
    const bool wide = k >= 13u;
    auto canon = [&](uint32_t z) __attribute__((always_inline)) -> uint32_t {
        if (wide) {
            const int32_t d = (int32_t)(int16_t)(uint16_t)((z >> 1) ^ (0u - (z & 1u)));
            return (((uint32_t)d << 1) ^ (uint32_t)(d >> 31)) & 0xffffu;
        }
        return z & 0xffffu;
    };
    const uint32_t steps = wave_max_u32(len);
    set_limits();
    for (uint32_t i = 0; i < steps; i += (uint32_t)kGS) {
        group_refill();
        if (i + (uint32_t)kGS <= len) {
            // ---- the unmasked group: eight pairs, two codes per ring access
#pragma unroll
            for (int u = 0; u < kGS; u += 2) {
                LANE_PAIR(z1, z2)
                sink(canon(z1));
                sink(canon(z2));
            }
        } else if (i < len) {
            // ---- the masked group: the lane's waveform ends inside it.  One sample per ring access.
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)kGS; ++u) {
                if (i + u < len) {
                    LANE_ONE(z)
                    sink(canon(z));
                }
            }
        }
        group_end();
        round_end(i);
    }
    return !(len && LANE_MISSES_LAST_WORD());
}

// which waveform a lane takes: lane_wave(), or (LIST) entry 64 * wavefront + lane of the list
template <bool LIST>
__device__ __forceinline__ bool recode_lane_wave(const Geom &G, uint64_t wf, int lane, const uint32_t *list, const uint32_t *n_list, LaneWave &w) {
    if (!LIST) return lane_wave(G, wf, lane, w);
    const uint64_t j = wf * 64u + (uint32_t)lane;
    w.g = 0; w.chunk = 0; w.idx = 0; w.len = 0; w.n_samples = 0;
    w.active = j < (uint64_t)*n_list;
    if (w.active) {
        w.g = list[j];
        const WaveRef r = locate(G, w.g);
        w.chunk = r.chunk; w.idx = r.idx; w.len = r.len; w.n_samples = r.n_samples;
    }
    return true;
}

// A lane's side of the output: its column of the wavefront's output ring (oring_all: kOutRingWords words of LDS, 16-byte aligned,
// word-major like the input ring) and the region of `out` the sizes pass gave its waveform -- the header word at `pos`, n2
// payload words behind it.  emit() codes one value at 2^k2 into the ring, flush_line() stores a 64-byte segment, group_end() is
// the look once per group with the wavefront converged, lane_flush() the same look for one lane alone (the serial kernels), and
// finish() writes what is left.  Every word of the region is stored exactly once, none outside it.
struct OutRing {
    uint32_t *myout, *outB;  // the lane's column; out + B, B a multiple of kOL: positions below are relative to B
    bool out_vec_ok;
    uint32_t end;   // of the lane's region
    uint32_t ow;    // next word the lane produces; a word's row of the ring is its position mod kOW
    uint32_t fl;    // next word to be stored to out
    uint64_t acc;   // bits not yet in the ring, in its low nacc bits
    uint32_t nacc;  // (< 32 between samples)

    __device__ __forceinline__ void open(uint32_t *oring_all, int lane, uint32_t *__restrict__ out, uint64_t pos, uint32_t n2) {
        // the payload is words [B + ow0, B + end) of out
        const uint64_t B = (pos + 1u) & ~(uint64_t)(kOL - 1);
        const uint32_t ow0 = (uint32_t)(pos + 1u - B);
        end = ow0 + n2;
        outB = out + B;
        out_vec_ok = ((uintptr_t)out & 15u) == 0;
        myout = oring_all + lane;
        ow = ow0;
        fl = ow0;
        acc = 0;
        nacc = 0;
    }
    // stores the words [fl, segment's end) of the 64-byte segment that holds fl: a whole one by 16-byte stores, a waveform's
    // first one (it starts behind the header word) word by word
    __device__ __forceinline__ void flush_line() {
        const uint32_t le = (fl | (uint32_t)(kOL - 1)) + 1u;
        if ((fl & (uint32_t)(kOL - 1)) == 0u && out_vec_ok) {
            typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
            typedef u32x4v __attribute__((address_space(1))) g_uint4;
            const uint32_t *src = myout + (fl & (uint32_t)(kOW - 1)) * 64u;
            g_uint4 *dst = (g_uint4 *)(outB + fl);
#pragma unroll
            for (int j = 0; j < kOL / 4; ++j)
                dst[j] = (u32x4v){src[(4 * j + 0) * 64], src[(4 * j + 1) * 64], src[(4 * j + 2) * 64], src[(4 * j + 3) * 64]};
        } else {
            for (uint32_t x = fl; x < le; ++x) outB[x] = myout[(x & (uint32_t)(kOW - 1)) * 64u];
        }
        fl = le;
    }
    __device__ __forceinline__ void emit(uint32_t z, uint32_t k2) {
        // rice_code()'s code and length (drx_encode_kernels.hip), from the zig-zag value
        const uint32_t q = z >> k2;
        const bool esc = q >= 8u;
        const uint32_t nb = esc ? 25u : q + 1u + k2;
        const uint32_t code = esc ? (0x10000u | z) : ((1u << k2) | (z & ((1u << k2) - 1u)));
        acc = (acc << nb) | code;
        nacc += nb;
        if (nacc >= 32u) {
            nacc -= 32u;
            if (ow < end) {  // (a lane never goes beyond the region the sizes pass gave it)
                myout[(ow & (uint32_t)(kOW - 1)) * 64u] = (uint32_t)(acc >> nacc);
                ++ow;
            }
        }
    }
    __device__ __forceinline__ void group_end() {
        if (__any(ow - fl >= kFlushAt)) {
            wave_sync();
            while (__any(ow > (fl | (uint32_t)(kOL - 1)))) {
                if (ow > (fl | (uint32_t)(kOL - 1))) flush_line();
            }
            wave_sync();
        }
    }
    // one lane on its own, behind every emit(): a segment goes out as soon as the ring holds all of it (a lane reads what it
    // wrote itself, in program order)
    __device__ __forceinline__ void lane_flush() {
        if (ow > (fl | (uint32_t)(kOL - 1))) flush_line();
    }
    // the last word left aligned, zero padded (:237-241), then what the ring still holds: whole segments, and the ragged last
    // words of the waveform's region
    __device__ __forceinline__ void finish() {
        if (nacc && ow < end) {
            myout[(ow & (uint32_t)(kOW - 1)) * 64u] = (uint32_t)(acc << (32u - nacc));
            ++ow;
        }
        wave_sync();
        while (ow > (fl | (uint32_t)(kOL - 1))) flush_line();
        for (uint32_t x = fl; x < ow; ++x) outB[x] = myout[(x & (uint32_t)(kOW - 1)) * 64u];
    }
};

}  // namespace

// Sizes.  ALLK = false: new_words[g] (and out_wave_words[g], where given) = n_i' at k2.  ALLK = true: est[k] += the batch's
// words at k, headers included.  A lane whose payload fails the end check raises kErrCorrupt (what it stored is then undefined).
// LIST: lane 0 of the launch leaves the list's length in the status word for drx_plan_last_transcode_listed.
// (The body of k_recode_sizes, k_recode_sizes_list and k_refilter_sizes.)
template <bool ALLK, bool LIST, typename Map>
__device__ __forceinline__ void recode_sizes(const Geom &G, const uint32_t *__restrict__ in, uint64_t in_words,
                                             const uint64_t *__restrict__ wave_off, const uint32_t *__restrict__ wave_words,
                                             uint64_t wf_base, uint32_t k2, DevStatus *st, uint32_t *__restrict__ new_words,
                                             uint32_t *__restrict__ out_wave_words, unsigned long long *__restrict__ est,
                                             const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list, Map &&map) {
    constexpr int NK = ALLK ? 16 : 1;
    __shared__ uint32_t ring_all[kInRingWords];
    const int lane = lane_id();
    if (LIST && blockIdx.x == 0 && threadIdx.x == 0) st->listed = *n_list;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
    LaneWave w;
    if (!recode_lane_wave<LIST>(G, wf_base + blockIdx.x, lane, list, n_list, w)) return;
    uint64_t S = 1;
    uint32_t n = 0;
    if (w.active) {
        S = wave_off[w.g] + 1u;
        n = wave_words[w.g];
    }
    uint64_t bits[NK];
    uint32_t gb[NK];  // of the current group: at most 16 x 25
#pragma unroll
    for (int j = 0; j < NK; ++j) { bits[j] = 0; gb[j] = 0; }
    const bool ok = parse_lane(ring_all + 64, in, in_words, S, n, w.len, G.k, lane,
        [&](uint32_t z0) __attribute__((always_inline)) {
            const uint32_t z = map(z0);
#pragma unroll
            for (int j = 0; j < NK; ++j) gb[j] += trc_code_bits(z, ALLK ? (uint32_t)j : k2);
        },
        [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < NK; ++j) { bits[j] += gb[j]; gb[j] = 0; }
        });
    if (w.active && !ok) atomicOr(&st->err, kErrCorrupt);
    if (ALLK) {
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            // a header word per waveform, and one per chunk (its first waveform's lane adds it)
            const uint64_t mine = w.active ? 1u + ((bits[j] + 31u) >> 5) + (w.idx == 0 ? 1u : 0u) : 0u;
            const uint64_t all = wave_sum_u64(mine);
            if (lane == 0) atomicAdd(est + j, (unsigned long long)all);
        }
    } else if (w.active) {
        const uint32_t nw = (uint32_t)((bits[0] + 31u) >> 5);
        new_words[w.g] = nw;
        if (out_wave_words) out_wave_words[w.g] = nw;
    }
}

// Pack.  new_words / new_rel / out_chunk_off: the sizes pass's table and what k_chunk_scan / k_chunk_offsets made of it.
// Nothing is written where the status word holds an error (a walker's or the sizes pass's kErrCorrupt, kErrCapacity).
// (The body of k_recode_pack, k_recode_pack_list and k_refilter_pack.)
template <bool LIST, typename Map>
__device__ __forceinline__ void recode_pack(const Geom &G, const uint32_t *__restrict__ in, uint64_t in_words,
                                            const uint64_t *__restrict__ wave_off, const uint32_t *__restrict__ wave_words,
                                            uint64_t wf_base, uint32_t k2, const DevStatus *st, const uint32_t *__restrict__ new_words,
                                            const uint32_t *__restrict__ new_rel, const uint64_t *__restrict__ out_chunk_off,
                                            uint32_t *__restrict__ out, const uint32_t *__restrict__ list,
                                            const uint32_t *__restrict__ n_list, Map &&map) {
    __shared__ uint32_t ring_all[kInRingWords];
    __shared__ __attribute__((aligned(16))) uint32_t oring_all[kOutRingWords];
    const int lane = lane_id();
    if (st->err) return;
    LaneWave w;
    if (!recode_lane_wave<LIST>(G, wf_base + blockIdx.x, lane, list, n_list, w)) return;
    uint64_t S = 1;
    uint32_t n = 0, n2 = 0;
    uint64_t pos = 0;  // of the lane's header word in out
    if (w.active) {
        S = wave_off[w.g] + 1u;
        n = wave_words[w.g];
        n2 = new_words[w.g];
        pos = out_chunk_off[w.chunk] + new_rel[w.g];
        out[pos] = n2;                               // :379
        if (w.idx == 0) out[pos - 1] = w.n_samples;  // chunk header, :415
    }
    OutRing o;
    o.open(oring_all, lane, out, pos, n2);
    (void)parse_lane(ring_all + 64, in, in_words, S, n, w.len, G.k, lane,
        [&](uint32_t z) __attribute__((always_inline)) { o.emit(map(z), k2); },
        [&]() __attribute__((always_inline)) { o.group_end(); });
    if (!w.active) return;
    o.finish();
}

}  // namespace drx
#endif
