// Packed 16-bit Rice coding of a 512-sample tile (64 lanes x 8 samples), its emission into an LDS bit buffer, and the loops
// the single-pass encoders build from them.  Device code only; included by the .hip translation units.  Who uses what:
//   packed_codes .. place_words   the tile arithmetic: every user below, and k_encode_pieces' own tile (drx_pieces.hip), which
//                                 rewrites a lane's history per waveform and so keeps its own front half
//   code_tile, put_tile           four dwords -> codes, lengths, scan, and into LDS: k_encode_fused, for_segment_tiles
//                                 (drx_encode_kernels.hip), k_encode_stream, k_encode_stream_segs (drx_encode_stream.hip),
//                                 recode_tiles
//   for_full_tiles                the three-deep load pipeline: k_encode_fused and k_encode_stream_segs
//   code_tail_tile, put_tail_tile, for_tiles
//                                 k_encode_stream: a waveform's trailing partial tile on the full tile's arithmetic, and the
//                                 pipeline with that tile in it and nothing but unconditional loads
//   recode_waveform, recode_range, history_before
//                                 a waveform or a sample range whose code outgrew its LDS buffer, coded again straight to its
//                                 place: k_encode_fused, both stream kernels, k_encode_pieces
#ifndef DRX_ENCODE_H
#define DRX_ENCODE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_device.h"

namespace drx {

constexpr int kTile = 512;  // samples per wave tile: 64 lanes x 8 samples (16 B per lane)

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int16_t i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_u16x2(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ i16x2 as_i16x2(uint32_t x) { return __builtin_bit_cast(i16x2, x); }
__device__ __forceinline__ uint32_t as_u32(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ u16x2 splat(uint32_t v) { return (u16x2){(uint16_t)v, (uint16_t)v}; }

// Packed code parameters of the 8 samples a lane holds as 4 dwords (low half = earlier sample).
//   nb   code length,
//   c16  the code's low 16 bits: payload with the terminating '1' above it (k low bits of z | 1 << k), or the
//        16 payload bits of an escape, whose terminator is bit 16:
//   e    1 for an escape, else 0.  The code word is (e << 16) | c16, its leading zeros are implicit.
struct PackedCodes { uint32_t nb[4], c16[4], e[4]; };

// x[j]: samples 2j, 2j+1; xprev: dword whose HIGH half is the sample just before x[0]'s low half.
// GEN: general forward filter (src/deltaRice.c:64-74) d[i] = sum_j taps[j] x[i-j] modulo 2^16, at most four taps
// (tp[j] = taps[j] in both halves); xprev2: the dword before xprev (samples i-4, i-3 of the lane's first pair).
template <bool GEN>
__device__ __forceinline__ void packed_codes(const uint32_t x[4], uint32_t xprev, uint32_t xprev2, const u16x2 (&tp)[4],
                                             uint32_t k, PackedCodes &c) {
    const u16x2 kv = splat(k), kp1 = splat(k + 1u), c16k = splat(16u - k);
    const u16x2 mlo = splat((1u << k) - 1u), mdelta = splat(0xffffu - ((1u << k) - 1u));
    // stage by stage over the four dwords rather than dword by dword: consecutive instructions are then
    // independent and the packed-math / op_sel hazards need no s_nop (21 per tile before)
    u16x2 z[4], qc[4], e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t xm1 = j ? x[j - 1] : xprev;                                           // samples 2j-2, 2j-1
        const uint32_t before = __builtin_amdgcn_alignbit(x[j], xm1, 16);                    // samples 2j-1, 2j
        i16x2 d;
        if (GEN) {
            const uint32_t xm2 = j >= 2 ? x[j - 2] : (j == 1 ? xprev : xprev2);
            const uint32_t before3 = __builtin_amdgcn_alignbit(xm1, xm2, 16);                // samples 2j-3, 2j-2
            d = __builtin_bit_cast(i16x2, (u16x2)(as_u16x2(x[j]) * tp[0] + as_u16x2(before) * tp[1] +
                                                  as_u16x2(xm1) * tp[2] + as_u16x2(before3) * tp[3]));
        } else {
            d = as_i16x2(x[j]) - as_i16x2(before);                                           // :51-63, mod 2^16
        }
        z[j] = __builtin_bit_cast(u16x2, (i16x2)(d << (int16_t)1)) ^
               __builtin_bit_cast(u16x2, (i16x2)(d >> (int16_t)15));                         // zig-zag :207-211
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) qc[j] = __builtin_elementwise_min((u16x2)(z[j] >> kv), splat(8u));  // min(q, 8)
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = qc[j] >> (uint16_t)3;                                         // 1 = escape (:215)
#pragma unroll
    for (int j = 0; j < 4; ++j) c.nb[j] = as_u32(e[j] * c16k + (qc[j] + kp1));   // q+1+k, or 8+1+16
    // c16 = z & (M-1) | M, or z for an escape: one v_bfi_b32 per dword, mask = M-1 or 0xffff per half (bit k of the
    // word 1 << k lies outside M-1, and an escape's mask lets nothing of it through)
    const uint32_t mword = as_u32(splat(1u << k));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t mask = as_u32(e[j] * mdelta + mlo);
        c.c16[j] = (mask & as_u32(z[j])) | (~mask & mword);
        c.e[j] = as_u32(e[j]);
    }
}

constexpr uint32_t kEncCapWords = 2048;  // LDS words per waveform buffer (8 KB): 9.3 bits/sample at L = 7000

// Loads this lane's 8 samples of the tile as 4 dwords; returns the number that exist.
__device__ __forceinline__ int load8_dwords(const int16_t *__restrict__ x, uint32_t len, uint32_t t0, int lane,
                                            bool vec_ok, uint32_t w[4]) {
    const uint32_t i0 = t0 + 8u * (uint32_t)lane;
    const int nv = (i0 >= len) ? 0 : (int)((len - i0) < 8u ? (len - i0) : 8u);
    if (vec_ok && nv == 8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(x + i0);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = (2 * j < nv) ? (uint32_t)(uint16_t)x[i0 + 2 * j] : 0u;
            const uint32_t b = (2 * j + 1 < nv) ? (uint32_t)(uint16_t)x[i0 + 2 * j + 1] : 0u;
            w[j] = a | (b << 16);
        }
    }
    return nv;
}

// Zeroes the code lengths of the samples a lane does not have (trailing partial tile): a
// zero-length code contributes no bits and, in emit_tile<false>, no set bits either.
__device__ __forceinline__ void mask_tail(PackedCodes &c, int nv) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t m = (2 * j + 1 < nv) ? 0xffffffffu : ((2 * j < nv) ? 0x0000ffffu : 0u);
        c.nb[j] &= m;
    }
}

// Bits of this lane's 8 codes.
__device__ __forceinline__ uint32_t lane_tile_bits(const PackedCodes &c) {
    const u16x2 s = as_u16x2(c.nb[0]) + as_u16x2(c.nb[1]) + as_u16x2(c.nb[2]) + as_u16x2(c.nb[3]);
    const uint32_t v = as_u32(s);
    return (v & 0xffffu) + (v >> 16);
}

// ORs this lane's codes into LDS.  pb = 8 * (LDS byte address of the buffer's word 0) + bit position
// of the lane's first code, so (pb >> 3) & ~3 is the LDS byte address of the word holding that bit.
// FULL = false: lengths may have been zeroed by mask_tail(); such codes must not set any bit.
template <bool FULL>
__device__ __forceinline__ void emit_tile(const PackedCodes &c, uint32_t pb) {
    typedef uint32_t __attribute__((address_space(3))) lds_u32;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t n = (j & 1) ? (c.nb[j >> 1] >> 16) : (c.nb[j >> 1] & 0xffffu);
        // terminator + payload; the leading zeros are implicit
        uint32_t code32 = __builtin_amdgcn_perm(c.e[j >> 1], c.c16[j >> 1], (j & 1) ? 0x07060302u : 0x05040100u);
        if (!FULL) code32 = n ? code32 : 0u;
        const uint32_t pe = pb + n;        // end of this code = start of the next
        // left-align the code at bit (pb & 31) of a 64-bit window: shift = 64 - (pb & 31) - n,
        // which is ((pb & 32) - pe) mod 64; v_lshlrev_b64 reads 6 bits of the shift
        const uint64_t v = (uint64_t)code32 << (((pb & 32u) - pe) & 63u);
        lds_u32 *w = (lds_u32 *)(uintptr_t)((pb >> 3) & ~3u);
        __hip_atomic_fetch_or(w, (uint32_t)(v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((uint32_t)v) __hip_atomic_fetch_or(w + 1, (uint32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        pb = pe;
    }
}

// The same for a full tile, with fewer LDS operations: the lane first concatenates its 8 codes in
// registers (a right-aligned 128-bit string w3:w2:w1:w0, one funnel shift per word and code), then ORs
// whole words.  pe = 8 * (LDS byte address of the buffer's word 0) + bit position of the END of the lane's
// last code; lane_bits <= 128 (the caller checks; 8 codes are 52 bits on the headline data and can
// only pass 128 with three escapes or more).  Every code is at least one bit long (full tile), so
// 32 - n is a valid funnel shift.  Words before the lane's first one receive an OR with zero: the
// buffers carry a 4-word pad in front for that.
__device__ __forceinline__ void concat_codes(const PackedCodes &c, uint32_t (&w)[4]) {
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        // v_alignbit_b32 / v_lshl_or_b32 read 5 bits of the shift: for the low half the packed register serves as is
        const uint32_t nbj = c.nb[j >> 1];
        const uint32_t n = (j & 1) ? (nbj >> 16) : nbj;
        const uint32_t code32 = __builtin_amdgcn_perm(c.e[j >> 1], c.c16[j >> 1], (j & 1) ? 0x07060302u : 0x05040100u);
        const uint32_t s = 0u - n;  // == 32 - n (mod 32)
        if (j >= 3) w3 = __builtin_amdgcn_alignbit(w3, w2, s);
        if (j >= 2) w2 = __builtin_amdgcn_alignbit(w2, w1, s);
        if (j >= 1) w1 = __builtin_amdgcn_alignbit(w1, w0, s);
        w0 = (w0 << (n & 31u)) | code32;
    }
    w[0] = w0; w[1] = w1; w[2] = w2; w[3] = w3;
}

__device__ __forceinline__ void place_words(const uint32_t (&wd)[4], uint32_t pe) {
    typedef uint32_t __attribute__((address_space(3))) lds_u32;
    // B << (32 - e) == (B << 32) >> e with e = pe & 31: x0 is the word that holds bit pe
    const uint32_t x0 = __builtin_amdgcn_alignbit(wd[0], 0u, pe);
    const uint32_t x1 = __builtin_amdgcn_alignbit(wd[1], wd[0], pe);
    const uint32_t x2 = __builtin_amdgcn_alignbit(wd[2], wd[1], pe);
    const uint32_t x3 = __builtin_amdgcn_alignbit(wd[3], wd[2], pe);
    const uint32_t x4 = __builtin_amdgcn_alignbit(0u, wd[3], pe);
    lds_u32 *w = (lds_u32 *)(uintptr_t)(((pe >> 3) & ~3u) - 16u);  // word of x4: positive DS offsets from here
    __hip_atomic_fetch_or(w + 4, x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_or(w + 3, x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_or(w + 2, x2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (x3 | x4) {
        __hip_atomic_fetch_or(w + 1, x3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (x4) __hip_atomic_fetch_or(w, x4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// ---------------------------------------------------------------------------
// one tile, from its samples to LDS
// ---------------------------------------------------------------------------
constexpr uint32_t kBufFront = 4;  // pad words in front of an LDS bit buffer (place_words writes up to four words below a lane's last)

__device__ __forceinline__ void zero_row(uint32_t *row, uint32_t words, int lane) {  // (16-byte aligned, a multiple of four words)
    for (int i = lane; i < (int)(words / 4u); i += 64) reinterpret_cast<uint4 *>(row)[i] = make_uint4(0, 0, 0, 0);
}

// A tile's codes: cw = the lane's 8 codes as one string (FULLT only), incl = inclusive scan of lane_bits over the lanes.
struct TileCodes {
    PackedCodes c;
    uint32_t cw[4], lane_bits, incl, tile_bits;
};

// w: the lane's 8 samples; carry / carry2: the dwords whose high halves are samples -1 and -3 of the tile (wave uniform;
// x[-1] := 0 in front of a waveform, src/deltaRice.c:53-54), moved on to the next tile.  FULLT: all 512 samples exist;
// otherwise nv of the lane's 8.
template <bool GEN, bool FULLT>
__device__ __forceinline__ TileCodes code_tile(const uint32_t (&w)[4], int nv, uint32_t &carry, uint32_t &carry2, const u16x2 (&tp)[4],
                                               uint32_t k) {
    TileCodes t;
    const uint32_t xprev = wave_shr1_carry(w[3], carry);
    carry = (uint32_t)__builtin_amdgcn_readlane((int)w[3], 63);
    uint32_t xprev2 = 0;
    if (GEN) {
        xprev2 = wave_shr1_carry(w[2], carry2);
        carry2 = (uint32_t)__builtin_amdgcn_readlane((int)w[2], 63);
    }
    packed_codes<GEN>(w, xprev, xprev2, tp, k, t.c);
    if (!FULLT) mask_tail(t.c, nv);
    t.lane_bits = lane_tile_bits(t.c);
    if (FULLT) concat_codes(t.c, t.cw);  // independent of the scan: fills its DPP wait states
    t.incl = wave_incl_scan_dpp(t.lane_bits);
    t.tile_bits = (uint32_t)__builtin_amdgcn_readlane((int)t.incl, 63);
    return t;
}

// The tile into LDS: at(bit) = 8 * (LDS byte address of the buffer's word 0) + the buffer bit of the tile's bit `bit`.
template <bool FULLT, typename At>
__device__ __forceinline__ void put_tile(const TileCodes &t, At &&at) {
    if (FULLT && !__any(t.lane_bits > 128u))
        place_words(t.cw, at(t.incl));
    else
        emit_tile<FULLT>(t.c, at(t.incl - t.lane_bits));
}

// ---- a waveform's trailing tile on the full tile's arithmetic (k_encode_stream) ----
// w3:w2:w1:w0 >> n, any n (128 and more: zero)
__device__ __forceinline__ void shr128(uint32_t (&w)[4], uint32_t n) {
    const uint32_t ws = n >> 5;
    const uint32_t y0 = ws == 0u ? w[0] : ws == 1u ? w[1] : ws == 2u ? w[2] : ws == 3u ? w[3] : 0u;
    const uint32_t y1 = ws == 0u ? w[1] : ws == 1u ? w[2] : ws == 2u ? w[3] : 0u;
    const uint32_t y2 = ws == 0u ? w[2] : ws == 1u ? w[3] : 0u;
    const uint32_t y3 = ws == 0u ? w[3] : 0u;
    w[0] = __builtin_amdgcn_alignbit(y1, y0, n);
    w[1] = __builtin_amdgcn_alignbit(y2, y1, n);
    w[2] = __builtin_amdgcn_alignbit(y3, y2, n);
    w[3] = y3 >> (n & 31u);
}

// The trailing tile's codes: nv of the lane's 8 samples exist, the missing ones are its LAST and were loaded as zeros.
// concat_codes needs every code to be at least a bit long (32 - 0 is no funnel shift), so the lane's string is built from
// all eight codes as they come out of packed_codes -- a missing sample has a code like any other, k + 1 bits or more -- and
// what the missing ones put at its low end is shifted out again.  `ragged` (wave uniform: the length is no multiple of 8):
// one lane holds 1..7 samples and the string is shifted by the bits of its missing codes; otherwise a lane holds eight
// samples or none, and a select per word does.  t.c keeps the unmasked lengths: put_tail_tile() masks them for emit_tile.
// `wide` (wave uniform): a lane's eight codes are more than 128 bits, the strings are not valid.
template <bool GEN>
__device__ __forceinline__ TileCodes code_tail_tile(const uint32_t (&w)[4], int nv, bool ragged, uint32_t &carry, uint32_t &carry2,
                                                    const u16x2 (&tp)[4], uint32_t k, bool &wide) {
    TileCodes t;
    const uint32_t xprev = wave_shr1_carry(w[3], carry);
    carry = (uint32_t)__builtin_amdgcn_readlane((int)w[3], 63);
    uint32_t xprev2 = 0;
    if (GEN) {
        xprev2 = wave_shr1_carry(w[2], carry2);
        carry2 = (uint32_t)__builtin_amdgcn_readlane((int)w[2], 63);
    }
    packed_codes<GEN>(w, xprev, xprev2, tp, k, t.c);
    const uint32_t all_bits = lane_tile_bits(t.c);
    concat_codes(t.c, t.cw);
    if (ragged) {
        PackedCodes cm = t.c;
        mask_tail(cm, nv);
        t.lane_bits = lane_tile_bits(cm);
        shr128(t.cw, all_bits - t.lane_bits);
    } else {
        t.lane_bits = nv ? all_bits : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) t.cw[j] = nv ? t.cw[j] : 0u;
    }
    wide = __any((nv ? all_bits : 0u) > 128u);
    t.incl = wave_incl_scan_dpp(t.lane_bits);
    t.tile_bits = (uint32_t)__builtin_amdgcn_readlane((int)t.incl, 63);
    return t;
}

// The trailing tile into LDS (at: as put_tile's).  A lane without samples ORs zeros into the words its neighbour ends in.
template <typename At>
__device__ __forceinline__ void put_tail_tile(const TileCodes &t, int nv, bool wide, At &&at) {
    if (!wide) {
        place_words(t.cw, at(t.incl));
    } else {
        PackedCodes c = t.c;
        mask_tail(c, nv);
        emit_tile<false>(c, at(t.incl - t.lane_bits));
    }
}

// The full tiles of x[0, 512 n_full): full(w) for each, between() in front of every group of kDepth.
// kDepth tiles of loads in flight, in kDepth fixed register sets (the loop is unrolled by kDepth so that no
// loaded-but-not-yet-arrived register is ever copied): with 4 waves per SIMD a tile takes ~2.6 K cycles of wall time, less
// than one HBM round trip under load (PMC: 76 % of the wave cycles were s_waitcnt with one tile in flight).  16-byte loads at
// any int16 alignment (unaligned access is on for HSA queues): a WaveformLength like 3500 puts every other waveform 8 bytes
// off a 16-byte boundary, an odd one 2 bytes off a dword, and the per-sample fallback is 2x slower.
template <typename B, typename F>
__device__ __forceinline__ void for_full_tiles(const int16_t *__restrict__ x, uint32_t n_full, int lane, B &&between, F &&full) {
    constexpr int kDepth = 3;
    const uint4 *xv = reinterpret_cast<const uint4 *>(x) + lane;  // tile t: xv[64 * t]
    uint4 q[kDepth];
    uint32_t t = 0;
#pragma unroll
    for (int u = 0; u < kDepth; ++u) {
        q[u] = make_uint4(0, 0, 0, 0);
        if ((uint32_t)u < n_full) q[u] = xv[64 * (size_t)u];
    }
    // while every register set has a successor tile: consume a set, then refill it -- no predicate on the load, so no copy
    // of a set and a plain vmcnt(kDepth - 1) in front of each tile
#pragma unroll 1
    for (; t + 2u * kDepth <= n_full; t += kDepth) {
        between();
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
            full(w);
            q[u] = xv[64 * (size_t)(t + u + kDepth)];
        }
    }
    // drain: the last kDepth..2 kDepth - 1 full tiles
#pragma unroll 1
    for (; t < n_full; t += kDepth) {
        between();
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            if (t + (uint32_t)u < n_full) {
                const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                full(w);
                if (t + (uint32_t)u + kDepth < n_full) q[u] = xv[64 * (size_t)(t + u + kDepth)];
            }
        }
    }
}

// The pipeline for a waveform WITH its trailing partial tile (k_encode_stream; for_full_tiles above stays as the other
// encoders compile it): full(w) for each of the n_full full tiles, tailf(w) for the trailing one (`tail`), between(again)
// in front of every group of kDepth -- again = false in front of the last, short one, behind which nobody would read what
// a look-up brings (its register is the next tile's scratch, which then waits for it at once).  len >= 8.  Two things
// differ from for_full_tiles.
//   * The trailing tile is tile n_full of the same pipeline: its load is issued kDepth tiles ahead like any other.  Only
//     the lanes that hold eight of its samples get them; tailf() must not look at the other lanes' registers.
//   * EVERY load is unconditional: kDepth in the prologue, one behind every tile.  The compiler's s_waitcnt in front of a
//     tile counts what is in flight on the WORST path into it, feasible or not.  Behind a prologue of `if (u < n_full)`
//     loads that is a path on which the tile's own load is the youngest, and the wait was vmcnt(0) at the head of every
//     group of kDepth tiles: the whole pipeline drained, the look-up that between() had just issued included (the assembly
//     of for_full_tiles shows it).  Here a load beyond the waveform's last tile is that tile again (in the cache by
//     then), and a lane whose 16 bytes would end behind x[len - 1] reads the waveform's last 16 bytes instead: no lane
//     reads in front of x[0] or behind x[len - 1], and every tile's wait is vmcnt(kDepth - 1).
template <typename B, typename F, typename T>
__device__ __forceinline__ void for_tiles(const int16_t *__restrict__ x, uint32_t len, uint32_t n_full, bool tail, int lane,
                                          B &&between, F &&full, T &&tailf) {
    constexpr int kDepth = 3;
    const uint32_t last = tail ? n_full : n_full - 1u;  // the waveform's last tile (n_full or tail: len >= 8)
    const uint32_t imax = len - 8u;                     // the last sample a lane's 16 bytes may begin at
    auto load = [&](uint32_t tile) -> uint4 {           // (tile: wave uniform)
        tile = tile < last ? tile : last;
        uint32_t i = tile * (uint32_t)kTile + 8u * (uint32_t)lane;
        i = i < imax ? i : imax;
        return *reinterpret_cast<const uint4 *>(x + i);
    };
    uint4 q[kDepth];
    // (in THIS order: the scheduler issued them last tile first, which makes the first tile's load the youngest again)
#pragma unroll
    for (int u = 0; u < kDepth; ++u) {
        q[u] = load((uint32_t)u);
        __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t t = 0;
#pragma unroll 1
    for (; t + kDepth <= n_full; t += kDepth) {
        between(true);
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
            full(w);
            q[u] = load(t + (uint32_t)u + kDepth);
        }
    }
    // tile t + u is in set u: up to kDepth - 1 full tiles, then the trailing one
    const uint32_t left = n_full - t;
    static_assert(kDepth == 3, "the straight code below");
    if (left) {
        between(false);
        const uint32_t w0[4] = {q[0].x, q[0].y, q[0].z, q[0].w};
        full(w0);
        if (left > 1u) {
            const uint32_t w1[4] = {q[1].x, q[1].y, q[1].z, q[1].w};
            full(w1);
        }
    }
    if (tail) {
        // (component by component: a select between the sets themselves is one between their addresses)
        auto sel = [left](uint32_t a, uint32_t b, uint32_t c) -> uint32_t { return left == 0u ? a : (left == 1u ? b : c); };
        const uint32_t w[4] = {sel(q[0].x, q[1].x, q[2].x), sel(q[0].y, q[1].y, q[2].y), sel(q[0].z, q[1].z, q[2].z),
                               sel(q[0].w, q[1].w, q[2].w)};
        tailf(w);
    } else {
        // Loads beyond the last tile are in flight and nobody reads them, but the next waveform's first write to one of
        // their registers would wait for them -- with a vmcnt(0) that waits for the stores issued since as well (a
        // ticket's total, wave_words).  Behind a trailing tile nothing is in flight: its selects have waited.
        __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
    }
}

// ---------------------------------------------------------------------------
// coded once more, tile by tile, straight to its place
// ---------------------------------------------------------------------------
// What a waveform, segment or part whose code outgrew its LDS buffer gets: a second read of its samples, each tile coded
// through the first words of the (cleared) row -- from bit P0 of outp[0] on, so that staged words ARE output words -- and
// its full words stored at once; the partly filled word becomes word 0 of the next tile.  The next tile's samples travel
// while this one is coded.  WINDOW: only the words [skip, limit) below `cap` are stored.  Returns the bit behind the last
// code; the row is left zeroed.
template <bool GEN, bool WINDOW>
__device__ __forceinline__ uint64_t recode_tiles(const int16_t *__restrict__ x, uint32_t len, uint32_t carry, uint32_t carry2,
                                                 const u16x2 (&tp)[4], uint32_t k, int lane, uint32_t *row, uint32_t row_words,
                                                 uint32_t *__restrict__ outp, uint32_t P0, uint32_t skip, uint32_t limit, uint64_t cap) {
    zero_row(row, row_words, lane);
    wave_sync();
    uint32_t *buf = row + kBufFront;
    const uint32_t buf_bits = lds_addr(buf) * 8u;
    auto mine = [&](uint64_t idx) -> bool { return !WINDOW || (idx >= skip && idx < limit && idx < cap); };
    uint64_t P = P0;
    uint32_t wn[4];
    int nvn = load8_dwords(x, len, 0u, lane, true, wn);
    for (uint32_t t0 = 0; t0 < len; t0 += kTile) {
        const uint32_t w[4] = {wn[0], wn[1], wn[2], wn[3]};
        const int nv = nvn;
        if (t0 + kTile < len) nvn = load8_dwords(x, len, t0 + kTile, lane, true, wn);
        const TileCodes t = code_tile<GEN, false>(w, nv, carry, carry2, tp, k);
        const uint64_t wfirst = P >> 5;  // first staged word
        const uint32_t at0 = buf_bits + (uint32_t)(P & 31u);
        put_tile<false>(t, [&](uint32_t bit) -> uint32_t { return at0 + bit; });
        P += t.tile_bits;
        wave_sync();
        const uint32_t nfull = (uint32_t)((P >> 5) - wfirst);
        for (uint32_t i = lane; i < nfull; i += 64) {
            if (mine(wfirst + i)) outp[wfirst + i] = buf[i];
            buf[i] = 0;
        }
        wave_sync();
        if (nfull && lane == 0) { const uint32_t cwd = buf[nfull]; buf[nfull] = 0; buf[0] = cwd; }
        wave_sync();
    }
    if (lane == 0) {
        if ((P & 31u) && mine(P >> 5)) outp[P >> 5] = buf[0];  // last word left aligned, zero padded (:237-241)
        buf[0] = 0;
    }
    wave_sync();
    return P;
}

// a whole waveform x[0, len), from bit 0 of outp[0]; returns its bits
template <bool GEN>
__device__ __forceinline__ uint64_t recode_waveform(const int16_t *__restrict__ x, uint32_t len, const u16x2 (&tp)[4], uint32_t k, int lane,
                                                    uint32_t *row, uint32_t row_words, uint32_t *__restrict__ outp) {
    return recode_tiles<GEN, false>(x, len, 0u, 0u, tp, k, lane, row, row_words, outp, 0u, 0u, 0u, 0ull);
}

// The filter's history in front of x[0], a sample that does not begin its waveform: the dwords a tile's first lane takes
// for the lane below (carry: samples -2, -1; GEN only: carry2: samples -4, -3).
template <bool GEN>
__device__ __forceinline__ void history_before(const int16_t *__restrict__ x, uint32_t &carry, uint32_t &carry2) {
    carry = (uint32_t)(uint16_t)x[-1] << 16;
    if (GEN) {
        carry |= (uint32_t)(uint16_t)x[-2];
        carry2 = (uint32_t)(uint16_t)x[-4] | ((uint32_t)(uint16_t)x[-3] << 16);
    }
}

// Samples [s_begin, s_end) of the waveform xw[0, wf_len), whose code is bits [Bp, Bp + bits_mine) of the waveform's stream
// payload[0, cap_words).  The word in which they start belongs to whoever codes the samples in front; the word in which they
// end is completed from the (up to) 32 samples that follow (at least a bit each), coded here too: wavefronts exchange nothing
// and no word is written twice.
template <bool GEN>
__device__ __forceinline__ void recode_range(const int16_t *__restrict__ xw, uint32_t wf_len, uint32_t s_begin, uint32_t s_end, uint64_t Bp,
                                             uint32_t bits_mine, const u16x2 (&tp)[4], uint32_t k, int lane, uint32_t *row,
                                             uint32_t row_words, uint32_t *__restrict__ payload, uint64_t cap_words) {
    const uint32_t P0 = (uint32_t)(Bp & 31u);
    const uint64_t wbase = Bp >> 5;
    const uint32_t more = wf_len - s_end < 32u ? wf_len - s_end : 32u;
    uint32_t carry = 0, carry2 = 0;
    if (s_begin) history_before<GEN>(xw + s_begin, carry, carry2);
    recode_tiles<GEN, true>(xw + s_begin, s_end - s_begin + more, carry, carry2, tp, k, lane, row, row_words, payload + wbase, P0,
                            P0 ? 1u : 0u, (P0 + bits_mine + 31u) >> 5, cap_words > wbase ? cap_words - wbase : 0ull);
}

}  // namespace drx
#endif
