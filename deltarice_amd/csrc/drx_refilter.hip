// drx_refilter.hip -- re-code an encoded batch under another prediction filter AND another RiceParameter without decoding it to
// memory (drx_transcode_filter), and the size of the result at every RiceParameter (drx_estimate_words_encoded_filter).  The
// result is, byte for byte, drx_encode under the target filter of the samples drx_decode gives for the source.  It is the
// re-code of drx_transcode.hip -- walk, sizes, scan, offsets, pack, the same tables and verdicts -- with one stage of arithmetic
// between the parse and the sink: the source's inverse filter gives the sample, the target's forward filter the new residual.
// No sample goes to memory; the plan's own filter, RiceParameter and tables describe the source and are not changed.
//
//   k_refilter_sizes<ALLK> / k_refilter_pack   the FAST pair: recode_sizes() / recode_pack() of drx_recode.h over the value map
//       RefilterValue.  Source delta or G.fast_taps (at most 4 taps, lead +-1), target of at most 4 taps with any non-zero lead.
//       A lane keeps the last three samples y1, y2, y3 (mod 2^16, zero at a waveform's start: the reference's (i - j) >= 0
//       guards, and the delta filter's output[0] = input[0]); per canonical z
//           d  = un-zig-zag(z)                        a  = d + nt0 y1 + nt1 y2 + nt2 y3        y = t0neg ? -a : a
//           d' = e0 y + e1 y1 + e2 y2 + e3 y3         z' = zig-zag((int16)d')                  all mod 2^16
//       with nt = -taps[1..3] of the source ({1, 0, 0}: delta) and e = the target's taps mod 2^16 ({1, 0xffff, 0, 0}: delta).
//       The operands are 16-bit, so the products are seven v_mad_u32_u24 per sample (RefilterValue::mad24()); the coefficients
//       are kernel arguments and stay in scalar registers.  A code is at most 25 bits under any filter: the output ring's slack holds.
//   k_refilter_sizes_serial<ALLK> / k_refilter_pack_serial   every other pair (more than 4 taps on either side, a source lead
//       other than +-1 -- the reference's division towards zero -- or DRX_DBG_REFILTER_SERIAL): a lane per waveform over
//       serial_wave() (drx_lane_stream.h, global loads), the last 64 samples in an LDS column that the source's inverse filter
//       and the target's forward filter both read (serial_wave() stores none for a delta source: the sink stores every sample).
//       The target's 64 taps arrive by value.  The verdict is serial_wave()'s word count against n_i.  The pack emits through
//       the same OutRing, a lane flushing on its own.  Correct, not tuned.
//
// Always a lane per waveform.  drx_transcode's block form works on residuals and has no samples at a block's start, so a plan
// whose geometry takes that form for drx_transcode takes THESE kernels for a re-filter; a waveform of millions of samples in
// one lane is slow, and how slow has not been measured.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_blocks.h"
#include "drx_recode.h"

namespace drx {

namespace {

// The fast pair's coefficients, every one a value mod 2^16
struct RefilterCoef {
    uint32_t nt[3], t0neg;  // source: -taps[1..3], taps[0] == -1
    uint32_t e[4];          // target: taps[0..3]
};

// The stage between the parse and the sink: z of the source -> z' of the target; the lane's history in y1, y2, y3
struct RefilterValue {
    const RefilterCoef &c;
    uint32_t y1 = 0, y2 = 0, y3 = 0;
    __device__ __forceinline__ explicit RefilterValue(const RefilterCoef &coef) : c(coef) {}
    // coef * v + acc on the low 24 bits of coef and v: exact mod 2^16 whatever lies above bit 15 of either, so nothing here is
    // masked before the end.  Written out: the compiler sees that only sixteen bits of the sums are used, drops the masks of
    // __umul24() and is left with full 32-bit multiplies at a quarter of the rate.  coef: wave-uniform, a scalar register
    static __device__ __forceinline__ uint32_t mad24(uint32_t coef, uint32_t v, uint32_t acc) {
        uint32_t r;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "s"(coef), "v"(v), "v"(acc));
        return r;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t z) {
        const uint32_t d = (z >> 1) ^ (0u - (z & 1u));
        const uint32_t a = mad24(c.nt[0], y1, mad24(c.nt[1], y2, mad24(c.nt[2], y3, d)));  // (the newest sample last)
        const uint32_t y = c.t0neg ? 0u - a : a;
        const uint32_t r = mad24(c.e[0], y, mad24(c.e[1], y1, mad24(c.e[2], y2, mad24(c.e[3], y3, 0u))));
        y3 = y2; y2 = y1; y1 = y;
        const int32_t d2 = (int32_t)(int16_t)(uint16_t)r;
        return (uint32_t)((d2 << 1) ^ (d2 >> 31)) & 0xffffu;
    }
};

// The target of the serial pair, by value: 256 bytes of taps
struct RefilterTaps {
    int32_t t[DRX_MAX_TAPS];
    uint32_t n;
};

// the serial pair's stage: sample i of the waveform -> z' (src/deltaRice.c:64-74 over the samples that exist, mod 2^16).
// col: the lane's column of the last 64 samples, entry (i mod 64) * 64
__device__ __forceinline__ uint32_t serial_refilter(const RefilterTaps &T, int16_t *col, uint32_t i, int16_t y) {
    col[(i & 63u) * 64u] = y;
    uint32_t r = (uint32_t)(int32_t)y * (uint32_t)T.t[0];
    for (uint32_t j = 1; j < T.n && j <= i; ++j) r += (uint32_t)(int32_t)col[((i - j) & 63u) * 64u] * (uint32_t)T.t[j];
    const int32_t d2 = (int32_t)(int16_t)(uint16_t)r;
    return (uint32_t)((d2 << 1) ^ (d2 >> 31)) & 0xffffu;
}

}  // namespace

template <bool ALLK>
__global__ __launch_bounds__(64) void k_refilter_sizes(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                       const uint64_t *__restrict__ wave_off,
                                                       const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                       RefilterCoef coef, DevStatus *st, uint32_t *__restrict__ new_words,
                                                       uint32_t *__restrict__ out_wave_words,
                                                       unsigned long long *__restrict__ est) {
    RefilterValue map(coef);
    recode_sizes<ALLK, false>(G, in, in_words, wave_off, wave_words, wf_base, k2, st, new_words, out_wave_words, est, nullptr, nullptr, map);
}

__global__ __launch_bounds__(64) void k_refilter_pack(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                      RefilterCoef coef, const DevStatus *st, const uint32_t *__restrict__ new_words,
                                                      const uint32_t *__restrict__ new_rel,
                                                      const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out) {
    RefilterValue map(coef);
    recode_pack<false>(G, in, in_words, wave_off, wave_words, wf_base, k2, st, new_words, new_rel, out_chunk_off, out, nullptr, nullptr, map);
}

// Lanes map plainly, g = 64 * wavefront + lane, as in k_wave_stats_serial.  A payload is read inside [wave_off + 1,
// wave_off + 1 + n_i) alone, which the walk (or the side-band's check) has held inside [0, in_words).
template <bool ALLK>
__global__ __launch_bounds__(64) void k_refilter_sizes_serial(Geom G, const uint32_t *__restrict__ in,
                                                              const uint64_t *__restrict__ wave_off,
                                                              const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                              RefilterTaps T, DevStatus *st, uint32_t *__restrict__ new_words,
                                                              uint32_t *__restrict__ out_wave_words,
                                                              unsigned long long *__restrict__ est) {
    constexpr int NK = ALLK ? 16 : 1;
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    const uint32_t lane = threadIdx.x;
    const uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;  // (as k_recode_sizes)
    const bool active = g < G.total_waves;
    uint64_t bits[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) bits[j] = 0;
    uint32_t idx = 1;
    if (active) {
        const WaveRef r = locate(G, g);
        idx = r.idx;
        const uint32_t n = wave_words[g];
        const uint64_t words = serial_wave(G, in + wave_off[g] + 1, n, r.len, &hist[0][lane], 64u, [&](uint32_t i, int16_t y) __attribute__((always_inline)) {
            const uint32_t z = serial_refilter(T, &hist[0][lane], i, y);
#pragma unroll
            for (int j = 0; j < NK; ++j) bits[j] += trc_code_bits(z, ALLK ? (uint32_t)j : k2);
        });
        if (r.len && words != n) atomicOr(&st->err, kErrCorrupt);
    }
    if (ALLK) {
        // (every lane of the wavefront is here: the sums are the wavefront's)
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const uint64_t mine = active ? 1u + ((bits[j] + 31u) >> 5) + (idx == 0 ? 1u : 0u) : 0u;
            const uint64_t all = wave_sum_u64(mine);
            if (lane == 0) atomicAdd(est + j, (unsigned long long)all);
        }
    } else if (active) {
        const uint32_t nw = (uint32_t)((bits[0] + 31u) >> 5);
        new_words[g] = nw;
        if (out_wave_words) out_wave_words[g] = nw;
    }
}

__global__ __launch_bounds__(64) void k_refilter_pack_serial(Geom G, const uint32_t *__restrict__ in,
                                                             const uint64_t *__restrict__ wave_off,
                                                             const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                             RefilterTaps T, const DevStatus *st, const uint32_t *__restrict__ new_words,
                                                             const uint32_t *__restrict__ new_rel,
                                                             const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out) {
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    __shared__ __attribute__((aligned(16))) uint32_t oring_all[kOutRingWords];
    const uint32_t lane = threadIdx.x;
    const uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;  // (as k_recode_pack: a walker's or the sizes pass's verdict, kErrCapacity)
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    const uint32_t n2 = new_words[g];
    const uint64_t pos = out_chunk_off[r.chunk] + new_rel[g];
    out[pos] = n2;
    if (r.idx == 0) out[pos - 1] = r.n_samples;
    OutRing o;
    o.open(oring_all, (int)lane, out, pos, n2);
    (void)serial_wave(G, in + wave_off[g] + 1, wave_words[g], r.len, &hist[0][lane], 64u, [&](uint32_t i, int16_t y) __attribute__((always_inline)) {
        o.emit(serial_refilter(T, &hist[0][lane], i, y), k2);
        o.lane_flush();
    });
    o.finish();
}

namespace {

struct RefilterRoute {
    bool serial;
    RefilterCoef coef;
    RefilterTaps taps;
};
RefilterRoute refilter_route(const Geom &G, const RefilterTarget &T) {
    RefilterRoute r{};
    r.serial = !(G.n_taps == 0 || G.fast_taps) || T.n_taps > 4u || (G.dbg & DRX_DBG_REFILTER_SERIAL) != 0u;
    for (uint32_t j = 0; j < 3; ++j) r.coef.nt[j] = (G.n_taps == 0 ? (j == 0 ? 1u : 0u) : G.fast_nt[j]) & 0xffffu;
    r.coef.t0neg = G.n_taps != 0 && G.fast_t0neg;
    for (uint32_t j = 0; j < 4; ++j) r.coef.e[j] = j < T.n_taps ? (uint32_t)T.taps[j] & 0xffffu : 0u;
    for (uint32_t j = 0; j < DRX_MAX_TAPS; ++j) r.taps.t[j] = j < T.n_taps ? T.taps[j] : 0;
    r.taps.n = T.n_taps;
    return r;
}
uint32_t refilter_form_word(const RefilterRoute &r) {
    return DRX_TRANSCODE_FORM_LANES | DRX_TRANSCODE_FORM_REFILTER | (r.serial ? DRX_TRANSCODE_FORM_REFILTER_SERIAL : 0u);
}

}  // namespace

// ev: {start, walk's end, kernel's end, end}
hipError_t launch_estimate_words_refiltered(const StreamCall &c, const RefilterTarget &T, unsigned long long *d_est, uint32_t *form_out) {
    const Geom &G = *c.G;
    const RefilterRoute r = refilter_route(G, T);
    if (form_out) *form_out = refilter_form_word(r);
    if (G.total_waves == 0) return hipSuccess;
    hipError_t e = batch_walk_prologue(c);
    if (e == hipSuccess) e = hipMemsetAsync(d_est, 0, 16 * sizeof(unsigned long long), c.s);
    if (e != hipSuccess) return e;
    for_wavefront_slices(G, !r.serial, [&](uint64_t base, unsigned nb) {
        if (r.serial)
            k_refilter_sizes_serial<true><<<nb, 64, 0, c.s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, 0u, r.taps, c.d_status, nullptr, nullptr, d_est);
        else
            k_refilter_sizes<true><<<nb, 64, 0, c.s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, 0u, r.coef, c.d_status, nullptr, nullptr, d_est);
    });
    mark(c.ev, 2, c.s);
    mark(c.ev, 3, c.s);
    return hipGetLastError();
}

// ev: {start, walk's end, offsets' end, end}.  out.d_out == nullptr: as far as the offsets (the sizing call).
hipError_t launch_refilter(const StreamCall &c, uint32_t k2, const RefilterTarget &T, const TrcScratch &t, const EncOut &out, uint32_t *form_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    const RefilterRoute r = refilter_route(G, T);
    if (form_out) *form_out = refilter_form_word(r);
    if (G.total_waves == 0) return hipSuccess;
    hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    // ---- sizes, scan, offsets
    for_wavefront_slices(G, !r.serial, [&](uint64_t base, unsigned nb) {
        if (r.serial)
            k_refilter_sizes_serial<false><<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, k2, r.taps, c.d_status, t.words, out.d_wave_words, nullptr);
        else
            k_refilter_sizes<false><<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, k2, r.coef, c.d_status, t.words, out.d_wave_words, nullptr);
    });
    e = launch_chunk_offsets(G, t.words, t.rel, t.chunk_words, out.d_chunk_word_off, out.d_out ? out.out_cap : ~0ull, c.d_status, s);
    if (e != hipSuccess) return e;
    mark(c.ev, 2, s);
    // ---- pack
    if (out.d_out) {
        for_wavefront_slices(G, !r.serial, [&](uint64_t base, unsigned nb) {
            if (r.serial)
                k_refilter_pack_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, k2, r.taps, c.d_status, t.words, t.rel, out.d_chunk_word_off, out.d_out);
            else
                k_refilter_pack<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, k2, r.coef, c.d_status, t.words, t.rel, out.d_chunk_word_off, out.d_out);
        });
    }
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
