// drx_transcode.hip -- re-code an encoded batch to another RiceParameter without decoding it (drx_transcode), and the size of
// the batch at every RiceParameter from the stream alone (drx_estimate_words_encoded).  Under a fixed prediction filter the codes
// of one sample at any two RiceParameters carry the same zig-zag value z (src/deltaRice.c:207-228), so re-coding is parse, size,
// scan, pack on residuals: no filter arithmetic, no sample in memory, and nothing here depends on the plan's filter.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of these launches
// (launch_transcode(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   (k_recode_sizes_list / k_recode_pack_list: the same bodies over a device list of waveforms, behind the block form)
//   k_recode_sizes<false>  one LANE per waveform, the stream side the shared reader's (drx_lane_reader.inc) with its
//                          end-of-payload check.  Adds the length of every z at the new parameter and stores
//                          n_i' = ceil(bits / 32).
//   k_recode_sizes<true>   the same parse with sixteen bit counts per lane: the batch's words at every k = 0..15, added as
//                          k_estimate_words adds them (a header word per waveform and per chunk), one atomic per wavefront and k.
//   (k_chunk_scan / k_chunk_offsets of drx_encode_kernels.hip turn the table of n_i' into header positions, chunk offsets, the
//   total and kErrCapacity: launch_chunk_offsets())
//   k_recode_pack          the same parse; every z is emitted at the new parameter into a lane-private LDS output ring (32 words,
//                          word-major like the input ring) and written out in whole 64-byte half lines by 16-byte stores where
//                          d_out's alignment allows; the ragged first and last words of a waveform's region go out by word stores
//                          (neighbouring waveforms share lines, never words).  The lane writes its header word n_i', the first
//                          lane of a chunk N_c.  Every output word is stored exactly once.
//
// A residual is the int16 the decoders take from its code, in canonical form: an ordinary code whose value exceeds 65535
// (k >= 13 in a foreign stream) folds as drx_decode folds it, an escape that holds a small value comes out as an ordinary code.
//
// Few long waveforms (the batches blocks_form_batch() admits under kTranscodeForm, whatever the plan's filter) take the block form
// of drx_transcode_blocks.hip: a workgroup per block of a waveform's stream for the sizes and again for the pack, with these lane
// kernels behind each for the waveforms the blocks list (LIST: lane j of the launch takes waveform list[j], j < *n_list, a list
// and a length written on the device; the launch is sized for the whole batch).  The listed waveforms get their n_i' -- or their
// sixteen sums -- and their verdict here, and k_recode_pack writes every word of their regions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

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

}  // namespace

// Sizes.  ALLK = false: new_words[g] (and out_wave_words[g], where given) = n_i' at k2.  ALLK = true: est[k] += the batch's
// words at k, headers included.  A lane whose payload fails the end check raises kErrCorrupt (what it stored is then undefined).
// LIST: lane 0 of the launch leaves the list's length in the status word for drx_plan_last_transcode_listed.
// (The body of k_recode_sizes and k_recode_sizes_list; the kernels below are its two instantiations per ALLK.)
template <bool ALLK, bool LIST>
__device__ __forceinline__ void recode_sizes(const Geom &G, const uint32_t *__restrict__ in, uint64_t in_words,
                                             const uint64_t *__restrict__ wave_off, const uint32_t *__restrict__ wave_words,
                                             uint64_t wf_base, uint32_t k2, DevStatus *st, uint32_t *__restrict__ new_words,
                                             uint32_t *__restrict__ out_wave_words, unsigned long long *__restrict__ est,
                                             const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
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
        [&](uint32_t z) __attribute__((always_inline)) {
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

template <bool ALLK>
__global__ __launch_bounds__(64) void k_recode_sizes(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                     const uint64_t *__restrict__ wave_off,
                                                     const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                     DevStatus *st, uint32_t *__restrict__ new_words,
                                                     uint32_t *__restrict__ out_wave_words,
                                                     unsigned long long *__restrict__ est) {
    recode_sizes<ALLK, false>(G, in, in_words, wave_off, wave_words, wf_base, k2, st, new_words, out_wave_words, est, nullptr, nullptr);
}
template <bool ALLK>
__global__ __launch_bounds__(64) void k_recode_sizes_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                          const uint64_t *__restrict__ wave_off,
                                                          const uint32_t *__restrict__ wave_words, uint32_t k2, DevStatus *st,
                                                          uint32_t *__restrict__ new_words, uint32_t *__restrict__ out_wave_words,
                                                          unsigned long long *__restrict__ est, const uint32_t *__restrict__ list,
                                                          const uint32_t *__restrict__ n_list) {
    recode_sizes<ALLK, true>(G, in, in_words, wave_off, wave_words, 0u, k2, st, new_words, out_wave_words, est, list, n_list);
}

// Pack.  new_words / new_rel / out_chunk_off: the sizes pass's table and what k_chunk_scan / k_chunk_offsets made of it.
// Nothing is written where the status word holds an error (a walker's or the sizes pass's kErrCorrupt, kErrCapacity).
// (The body of k_recode_pack and k_recode_pack_list, below.)
template <bool LIST>
__device__ __forceinline__ void recode_pack(const Geom &G, const uint32_t *__restrict__ in, uint64_t in_words,
                                            const uint64_t *__restrict__ wave_off, const uint32_t *__restrict__ wave_words,
                                            uint64_t wf_base, uint32_t k2, const DevStatus *st, const uint32_t *__restrict__ new_words,
                                            const uint32_t *__restrict__ new_rel, const uint64_t *__restrict__ out_chunk_off,
                                            uint32_t *__restrict__ out, const uint32_t *__restrict__ list,
                                            const uint32_t *__restrict__ n_list) {
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
    // the payload is words [B + ow0, B + end) of out, B a multiple of kOL: positions below are relative to B, and a word's
    // row of the output ring is its position mod kOW
    const uint64_t B = (pos + 1u) & ~(uint64_t)(kOL - 1);
    const uint32_t ow0 = (uint32_t)(pos + 1u - B), end = ow0 + n2;
    uint32_t *__restrict__ outB = out + B;
    const bool out_vec_ok = ((uintptr_t)out & 15u) == 0;
    uint32_t *myout = oring_all + lane;
    uint32_t ow = ow0;  // next word the lane produces
    uint32_t fl = ow0;  // next word to be stored to out
    uint64_t acc = 0;   // bits not yet in the ring, in its low nacc bits
    uint32_t nacc = 0;  // (< 32 between samples)

    // stores the words [fl, segment's end) of the 64-byte segment that holds fl: a whole one by 16-byte stores, a waveform's
    // first one (it starts behind the header word) word by word
    auto flush_line = [&]() __attribute__((always_inline)) {
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
    };

    (void)parse_lane(ring_all + 64, in, in_words, S, n, w.len, G.k, lane,
        [&](uint32_t z) __attribute__((always_inline)) {
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
        },
        [&]() __attribute__((always_inline)) {
            if (__any(ow - fl >= kFlushAt)) {
                wave_sync();
                while (__any(ow > (fl | (uint32_t)(kOL - 1)))) {
                    if (ow > (fl | (uint32_t)(kOL - 1))) flush_line();
                }
                wave_sync();
            }
        });
    if (!w.active) return;
    // the last word left aligned, zero padded (:237-241), then what the ring still holds: whole segments, and the ragged last
    // words of the waveform's region
    if (nacc && ow < end) {
        myout[(ow & (uint32_t)(kOW - 1)) * 64u] = (uint32_t)(acc << (32u - nacc));
        ++ow;
    }
    wave_sync();
    while (ow > (fl | (uint32_t)(kOL - 1))) flush_line();
    for (uint32_t x = fl; x < ow; ++x) outB[x] = myout[(x & (uint32_t)(kOW - 1)) * 64u];
}

__global__ __launch_bounds__(64) void k_recode_pack(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                    const uint64_t *__restrict__ wave_off,
                                                    const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                    const DevStatus *st, const uint32_t *__restrict__ new_words,
                                                    const uint32_t *__restrict__ new_rel,
                                                    const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out) {
    recode_pack<false>(G, in, in_words, wave_off, wave_words, wf_base, k2, st, new_words, new_rel, out_chunk_off, out, nullptr, nullptr);
}
__global__ __launch_bounds__(64) void k_recode_pack_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                         const uint64_t *__restrict__ wave_off,
                                                         const uint32_t *__restrict__ wave_words, uint32_t k2, const DevStatus *st,
                                                         const uint32_t *__restrict__ new_words, const uint32_t *__restrict__ new_rel,
                                                         const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out,
                                                         const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    recode_pack<true>(G, in, in_words, wave_off, wave_words, 0u, k2, st, new_words, new_rel, out_chunk_off, out, list, n_list);
}

// The estimate: the walk and k_recode_sizes<true> alone, or (the block form) the blocks' sizes launch with sixteen counts and
// k_recode_sizes<true> over the waveforms it lists.  ev: {start, walk's end, kernel's end, end}
hipError_t launch_estimate_words_encoded(const StreamCall &c, unsigned long long *d_est, void *d_blk, void *d_tb, uint32_t *form_out) {
    const Geom &G = *c.G;
    const bool blocks = d_tb != nullptr && blocks_form_batch(G, d_blk, kTranscodeForm);
    if (form_out) *form_out = blocks_form_word(G, blocks, kTranscodeForm);
    if (G.total_waves == 0) return hipSuccess;
    hipError_t e = batch_walk_prologue(c);
    if (e == hipSuccess) e = hipMemsetAsync(d_est, 0, 16 * sizeof(unsigned long long), c.s);
    if (e != hipSuccess) return e;
    if (blocks) {
        BlkFallbackList fl;
        if ((e = launch_trc_blocks_sizes(c, d_blk, d_tb, 0u, TrcScratch{}, nullptr, d_est, &fl)) != hipSuccess) return e;
        k_recode_sizes_list<true><<<blocks_for(G.total_waves, 64), 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, 0u, c.d_status,
                                                                                 nullptr, nullptr, d_est, fl.listed, fl.n_listed);
    } else {
        for_wavefront_slices(G, true, [&](uint64_t base, unsigned nb) {
            k_recode_sizes<true><<<nb, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, 0u, c.d_status, nullptr, nullptr, d_est);
        });
    }
    mark(c.ev, 2, c.s);
    mark(c.ev, 3, c.s);
    return hipGetLastError();
}

// ev: {start, walk's end, offsets' end, end}.  out.d_out == nullptr: as far as the offsets (the sizing call).
hipError_t launch_transcode(const StreamCall &c, uint32_t k2, const TrcScratch &t, const EncOut &out, void *d_blk, void *d_tb, uint32_t *form_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    const bool blocks = d_tb != nullptr && blocks_form_batch(G, d_blk, kTranscodeForm);
    if (form_out) *form_out = blocks_form_word(G, blocks, kTranscodeForm);
    if (G.total_waves == 0) return hipSuccess;
    // ---- the walk (drx_walk.hip): launch_batch_walk()
    hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    // ---- sizes, scan, offsets (the block form: the blocks, then the lane kernel over the waveforms they list; the launch is sized
    // from here, at most a lane per waveform of the batch, and the list's length is read on the device)
    BlkFallbackList fl{};
    if (blocks) {
        if ((e = launch_trc_blocks_sizes(c, d_blk, d_tb, k2, t, out.d_wave_words, nullptr, &fl)) != hipSuccess) return e;
        k_recode_sizes_list<false><<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, k2, c.d_status,
                                                                                t.words, out.d_wave_words, nullptr, fl.listed, fl.n_listed);
    } else {
        for_wavefront_slices(G, true, [&](uint64_t base, unsigned nb) {
            k_recode_sizes<false><<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, k2, c.d_status, t.words, out.d_wave_words, nullptr);
        });
    }
    e = launch_chunk_offsets(G, t.words, t.rel, t.chunk_words, out.d_chunk_word_off, out.d_out ? out.out_cap : ~0ull, c.d_status, s);
    if (e != hipSuccess) return e;
    mark(c.ev, 2, s);
    // ---- pack
    if (out.d_out && blocks) {
        if ((e = launch_trc_blocks_pack(c, d_blk, d_tb, k2, t, out)) != hipSuccess) return e;
        k_recode_pack_list<<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, k2, c.d_status, t.words,
                                                                        t.rel, out.d_chunk_word_off, out.d_out, fl.listed, fl.n_listed);
    } else if (out.d_out) {
        for_wavefront_slices(G, true, [&](uint64_t base, unsigned nb) {
            k_recode_pack<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, k2, c.d_status, t.words, t.rel, out.d_chunk_word_off, out.d_out);
        });
    }
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
