// drx_bins.hip -- binned statistics of every waveform straight from the encoded stream (drx_wave_bins): every waveform is parsed
// as drx_decode parses it and reduced to n_bins rows of four int64 (DRX_BIN_* of include/deltarice_hip.h: sum, sum of squares,
// minimum, maximum), one row per stretch of `bin` samples from a per-waveform origin.  drx_wave_stats' two HEAD columns, for any
// number of equal windows.  The batch is read once (the stream) and 32 bytes per bin are written; no sample goes to memory.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_wave_bins(): the walks of drx_walk.hip, or the side-band's tables), as launch_wave_stats() does.
//
//   k_wave_bins         delta filter: one LANE per waveform, 64 waveforms per wavefront, the stream side the shared reader's
//                       (drx_lane_reader.inc); the reader's ring (16 896 bytes) is all the LDS there is.
//   k_wave_bins_serial  every other prediction filter: one lane per waveform, the serial parse of the same header
//                       (serial_wave()) with the filter's history in an LDS column.  Correct, not tuned.
//
// Bins along a waveform.  The bins of waveform g tile [a_g, a_g + n_bins * bin); the samples are [0, len_g).  The bins that
// receive a sample are therefore CONSECUTIVE: b0 .. b1, with only empty bins in front of b0 and behind b1.  A lane writes the
// empty rows in front of b0 before it parses, every bin's row as it passes the bin's end, and the empty rows behind b1 when it
// is through: each of the n_bins rows once, in order, none read, no launch in front.  What tells a lane where it is is a
// cursor (BinCursor) of the next BORDER -- the sample index at which the current stretch ends -- and the row that is due;
// both depend on the geometry alone, never on the stream, so a corrupt stream cannot move a store.
//
// Few long waveforms go through the same lane-per-waveform kernels by default: correct, and 50-60 ns per sample and lane whatever
// else runs.  Under the context option "bins_impl" = 1 they take the block form instead (drx_bins_blocks.hip; kBinsForm,
// drx_internal.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_bin_cursor.h"
#include "drx_lane_stream.h"

namespace drx {

// (s16x2, as_pair(), as_word(), kNarrow: drx_lane_stream.h, as in drx_stats.hip)
constexpr uint32_t kMnId = 0x7fff7fffu, kMxId = 0x80008000u;  // the packed identities of min and max

// (kNoBorder, bins_origin(), BinCursor, bins_begin() -- here from sample 0 -- and bins_border(): drx_bin_cursor.h)

// a bin's row: four int64, by 16-byte stores where the row allows them, by 8-byte stores otherwise (the ABI asks 8-byte
// alignment of d_out; rows are 32 bytes, so a waveform's rows are aligned alike).  Not store_i64_row() (drx_device.h): through
// it the two sign extensions move in front of the branch and k_wave_bins is no longer the kernel that was measured
__device__ __forceinline__ void store_bin(int64_t *__restrict__ rows, bool vec, uint32_t b, int64_t sum, uint64_t sq, int32_t mn, int32_t mx) {
    int64_t *row = rows + (uint64_t)b * (uint64_t)DRX_BIN_COLS;
    static_assert(DRX_BIN_SUM == 0 && DRX_BIN_SUMSQ == 1 && DRX_BIN_MIN == 2 && DRX_BIN_MAX == 3 && DRX_BIN_COLS == 4, "the row's order");
    if (vec) {
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        typedef u32x4v __attribute__((address_space(1))) g_uint4;
        g_uint4 *dst = (g_uint4 *)row;
        const int64_t mn64 = mn, mx64 = mx;
        dst[0] = (u32x4v){(uint32_t)sum, (uint32_t)((uint64_t)sum >> 32), (uint32_t)sq, (uint32_t)(sq >> 32)};
        dst[1] = (u32x4v){(uint32_t)mn64, (uint32_t)((uint64_t)mn64 >> 32), (uint32_t)mx64, (uint32_t)((uint64_t)mx64 >> 32)};
    } else {
        row[0] = sum;
        row[1] = (int64_t)sq;
        row[2] = mn;
        row[3] = mx;
    }
}
__device__ __forceinline__ void store_empty_bins(int64_t *__restrict__ rows, bool vec, uint32_t from, uint32_t to) {
    for (uint32_t b = from; b < to; ++b) store_bin(rows, vec, b, 0, 0u, 32767, -32768);
}

// Lanes map by LANE_WAVE_G_ACTIVE_LEN (drx_lane_stream.h).  wf_base: first wavefront of this launch (for_wavefront_slices()).
//
// A group is 16 samples, as in k_wave_stats, and costs what it costs there less the positions of the extremes: a lane whose
// group lies inside its waveform and is not its first runs the UNMASKED group -- eight pairs, folded as packed pairs of int16
// into the current bin's packed extremes (v_pk_min / v_pk_max; the halves are joined when the row is stored), v_dot2 chains for
// the sum and the sum of squares.  The squares go by k_wave_stats' rule: while every sample of the waveform so far lies within
// +-kNarrow a group's sum of squares is one 32-bit chain and one 64-bit add, otherwise the pairs' are added one by one.
//
// A border inside an unmasked group (bin >= 16: a group holds at most one) does not send the group through the masked form:
// with per-waveform origins some lane has a border in nearly every group, and the masked form would then run for the whole
// wavefront all the time.  The group is parsed unmasked and its eight registers are SPLIT at the lane's own position
// s = border - i: a per-pair mask keeps the samples in front of s (two compares), the masked-out halves are zero for the two
// sums and the identity for min and max (v_bfi), and the part behind s is the same under the inverted mask.  The part in front
// of s closes the bin -- its row is stored -- and the part behind opens the next.  Only lanes with a border run this.
//
// The first group of a waveform, the group in which it ends, and every group where bin < 16 (several borders per group) run
// the masked form, a sample per ring access with the border test per sample.
__global__ __launch_bounds__(64) void k_wave_bins(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                  const uint64_t *__restrict__ wave_off, const uint32_t *__restrict__ wave_words,
                                                  uint64_t wf_base, const int64_t *__restrict__ start, uint64_t start_stride,
                                                  int64_t offset, uint32_t bin, uint32_t n_bins, DevStatus *st,
                                                  int64_t *__restrict__ out, uint64_t out_wave_stride) {
    constexpr int GS = kGS;
    __shared__ uint32_t ring_all[kInRingWords];
    const int lane = lane_id();
    const uint32_t k = G.k;
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
    LANE_WAVE_G_ACTIVE_LEN(G, wf_base + blockIdx.x, lane)
    uint32_t n = 0;
    uint64_t S = 1;
    BinCursor c = {kNoBorder, 0u, false};
    int64_t *rows = out;
    bool vec = false;
    if (active) {
        S = wave_off[g] + 1u;
        n = wave_words[g];
        rows = out + g * out_wave_stride;
        vec = ((uintptr_t)rows & 15u) == 0;
        store_empty_bins(rows, vec, 0u, bins_begin(c, bins_origin(start, start_stride, offset, g), bin, n_bins, len, 0u));
    }
    uint32_t *const ring = ring_all + 64;
#include "drx_lane_reader.inc"

    const uint32_t steps = wave_max_u32(len);
    const bool wide = bin >= (uint32_t)GS;  // at most one border per group
    int32_t acc = 0;                        // running sum of the deltas: the sample in its low 16 bits
    // the current stretch's: sums, and packed extremes of its samples of even and of odd index
    int64_t sum = 0;
    uint64_t sq = 0;
    s16x2 rmn = as_pair(kMnId), rmx = as_pair(kMxId);
    bool narrow = true;  // every sample of the waveform so far lies within +-kNarrow
    auto within = [&](s16x2 lo, s16x2 hi) __attribute__((always_inline)) {  // (the identities pass)
        const s16x2 a = __builtin_elementwise_min(lo, (s16x2){(short)-kNarrow, (short)-kNarrow});
        const s16x2 b = __builtin_elementwise_max(hi, (s16x2){(short)kNarrow, (short)kNarrow});
        return as_word(a) == as_word((s16x2){(short)-kNarrow, (short)-kNarrow}) && as_word(b) == as_word((s16x2){(short)kNarrow, (short)kNarrow});
    };
    auto close_bin = [&]() __attribute__((always_inline)) {  // the row of the bin that ends here
        if (c.live)
            store_bin(rows, vec, c.cur, sum, sq, rmn.x < rmn.y ? (int32_t)rmn.x : (int32_t)rmn.y, rmx.x > rmx.y ? (int32_t)rmx.x : (int32_t)rmx.y);
    };
    set_limits();
    for (uint32_t i = 0; i < steps; i += (uint32_t)GS) {
        group_refill();
        if (wide && i != 0u && i + (uint32_t)GS <= len) {
            // ---- the unmasked group: eight pairs, two samples per ring access
            LANE_GROUP_PAIRS(acc, pr, 0u)  // the group's samples, two to a register (the earlier one in the low half)
            const uint32_t s = c.nb - i;  // (every border in front of i has been passed: nb >= i)
            if (s >= (uint32_t)GS) {
                // ---- no border: the whole group belongs to the current stretch
                s16x2 nmn = rmn, nmx = rmx;
                int32_t gsum = 0, gsq = 0;
#pragma unroll
                for (int j = 0; j < GS / 2; ++j) {
                    const s16x2 p = as_pair(pr[j]);
                    nmn = __builtin_elementwise_min(nmn, p);
                    nmx = __builtin_elementwise_max(nmx, p);
                    gsum = __builtin_amdgcn_sdot2(p, (s16x2){1, 1}, gsum, false);
                    gsq = __builtin_amdgcn_sdot2(p, p, gsq, false);
                }
                if (((as_word(nmn) ^ as_word(rmn)) | (as_word(nmx) ^ as_word(rmx))) != 0u) {
                    rmn = nmn;
                    rmx = nmx;
                    narrow = narrow && within(nmn, nmx);
                }
                sum += (int64_t)gsum;
                if (narrow) {
                    sq += (uint64_t)(uint32_t)gsq;  // sixteen squares of at most kNarrow^2: below 2^32
                } else {
#pragma unroll
                    for (int j = 0; j < GS / 2; ++j) sq += (uint64_t)(uint32_t)__builtin_amdgcn_sdot2(as_pair(pr[j]), as_pair(pr[j]), 0, false);
                }
            } else {
                // ---- a border at sample i + s: samples u < s close the current stretch, the others open the next
                uint32_t po[GS / 2], pn[GS / 2];  // the two parts, the other part's samples zero
                s16x2 omn = rmn, omx = rmx, nmn = as_pair(kMnId), nmx = as_pair(kMxId);
#pragma unroll
                for (int j = 0; j < GS / 2; ++j) {
                    const uint32_t m = (s > 2u * (uint32_t)j + 1u ? 0xffff0000u : 0u) | (s > 2u * (uint32_t)j ? 0xffffu : 0u);
                    po[j] = pr[j] & m;
                    pn[j] = pr[j] ^ po[j];
                    omn = __builtin_elementwise_min(omn, as_pair(po[j] | (~m & kMnId)));
                    omx = __builtin_elementwise_max(omx, as_pair(po[j] | (~m & kMxId)));
                    nmn = __builtin_elementwise_min(nmn, as_pair(pn[j] | (m & kMnId)));
                    nmx = __builtin_elementwise_max(nmx, as_pair(pn[j] | (m & kMxId)));
                }
                narrow = narrow && within(omn, omx) && within(nmn, nmx);
                int32_t gso = 0, gsn = 0;
                uint64_t sqo = 0, sqn = 0;
#pragma unroll
                for (int j = 0; j < GS / 2; ++j) {
                    gso = __builtin_amdgcn_sdot2(as_pair(po[j]), (s16x2){1, 1}, gso, false);
                    gsn = __builtin_amdgcn_sdot2(as_pair(pn[j]), (s16x2){1, 1}, gsn, false);
                }
                if (narrow) {
                    int32_t qo = 0, qn = 0;
#pragma unroll
                    for (int j = 0; j < GS / 2; ++j) {
                        qo = __builtin_amdgcn_sdot2(as_pair(po[j]), as_pair(po[j]), qo, false);
                        qn = __builtin_amdgcn_sdot2(as_pair(pn[j]), as_pair(pn[j]), qn, false);
                    }
                    sqo = (uint32_t)qo;
                    sqn = (uint32_t)qn;
                } else {
#pragma unroll
                    for (int j = 0; j < GS / 2; ++j) {
                        sqo += (uint64_t)(uint32_t)__builtin_amdgcn_sdot2(as_pair(po[j]), as_pair(po[j]), 0, false);
                        sqn += (uint64_t)(uint32_t)__builtin_amdgcn_sdot2(as_pair(pn[j]), as_pair(pn[j]), 0, false);
                    }
                }
                sum += (int64_t)gso;
                sq += sqo;
                rmn = omn;
                rmx = omx;
                close_bin();
                bins_border(c, bin, n_bins, len);
                sum = (int64_t)gsn;
                sq = sqn;
                rmn = nmn;
                rmx = nmx;
            }
        } else if (i < len) {
            // ---- the masked group: the waveform's first or last, or bins shorter than a group.  One sample per ring access.
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)GS; ++u) {
                const uint32_t idx = i + u;
                if (idx < len) {
                    if (idx == c.nb) {
                        close_bin();
                        bins_border(c, bin, n_bins, len);
                        sum = 0;
                        sq = 0;
                        rmn = as_pair(kMnId);
                        rmx = as_pair(kMxId);
                    }
                    LANE_ONE(z)
                    acc += (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);
                    const int32_t y = (int32_t)(int16_t)(uint16_t)acc;
                    sum += y;
                    sq += (uint64_t)(uint32_t)(y * y);
                    const s16x2 yy = {(short)y, (short)y};
                    rmn = __builtin_elementwise_min(rmn, yy);
                    rmx = __builtin_elementwise_max(rmx, yy);
                    narrow = narrow && y >= -kNarrow && y <= kNarrow;
                }
            }
        }
        round_end(i);
    }
    if (!active) return;
    if (len && LANE_MISSES_LAST_WORD()) atomicOr(&st->err, kErrCorrupt);
    // the bin the waveform ends in, and the empty ones behind it
    close_bin();
    store_empty_bins(rows, vec, c.cur + (c.live ? 1u : 0u), n_bins);
}

// General prediction filters: a lane per waveform, serial_wave() (global loads); the last 64 outputs of every
// lane in an LDS column (taps <= DRX_MAX_TAPS = 64).  The same cursor, a border test per sample.
// Not on serial_frame() (drx_lane_stream.h): through it this kernel was measured 0.4 % slower, profiles/serial_frame_refactor_ab.txt.
__global__ __launch_bounds__(64) void k_wave_bins_serial(Geom G, const uint32_t *__restrict__ in, const uint64_t *__restrict__ wave_off,
                                                         const uint32_t *__restrict__ wave_words, uint64_t wf_base,
                                                         const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset,
                                                         uint32_t bin, uint32_t n_bins, DevStatus *st, int64_t *__restrict__ out,
                                                         uint64_t out_wave_stride) {
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    const uint32_t lane = threadIdx.x;
    const uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;  // (as k_wave_bins)
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    const uint32_t *s = in + wave_off[g] + 1;
    const uint32_t n = wave_words[g];
    int64_t *rows = out + g * out_wave_stride;
    const bool vec = ((uintptr_t)rows & 15u) == 0;
    BinCursor c;
    store_empty_bins(rows, vec, 0u, bins_begin(c, bins_origin(start, start_stride, offset, g), bin, n_bins, r.len, 0u));
    int32_t mn = 32767, mx = -32768;
    int64_t sum = 0;
    uint64_t sq = 0;
    const uint64_t words = serial_wave(G, s, n, r.len, &hist[0][lane], 64u, [&](uint32_t i, int16_t y16) __attribute__((always_inline)) {
        if (i == c.nb) {
            if (c.live) store_bin(rows, vec, c.cur, sum, sq, mn, mx);
            bins_border(c, bin, n_bins, r.len);
            sum = 0;
            sq = 0;
            mn = 32767;
            mx = -32768;
        }
        const int32_t y = y16;
        sum += y;
        sq += (uint64_t)(uint32_t)(y * y);
        mn = y < mn ? y : mn;
        mx = y > mx ? y : mx;
    });
    if (r.len && words != n) atomicOr(&st->err, kErrCorrupt);
    if (c.live) store_bin(rows, vec, c.cur, sum, sq, mn, mx);
    store_empty_bins(rows, vec, c.cur + (c.live ? 1u : 0u), n_bins);
}

hipError_t launch_wave_bins(const StreamCall &c, void *d_blk, void *d_list, int bins_impl, const int64_t *d_start, uint64_t start_stride,
                            int64_t offset, uint32_t bin, uint32_t n_bins, int64_t *d_out, uint64_t out_wave_stride, uint32_t *form_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    // bins_impl 0 (the default): a lane per waveform whatever the batch, and the form's debug flags are inert
    const bool blocks = bins_impl == 1 && d_list != nullptr && blocks_form_batch(G, d_blk, kBinsForm);
    if (form_out) *form_out = blocks_form_word(G, blocks, kBinsForm);
    if (G.total_waves == 0) return hipSuccess;
    // ---- the walk (drx_walk.hip): launch_batch_walk()
    const hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    if (blocks) {
        // ---- few long waveforms: the identity rows, a workgroup per block of a waveform's stream, then a lane per waveform that
        // form lists (drx_bins_blocks.hip)
        const hipError_t eb = launch_bins_blocks(c, d_blk, d_list, d_start, start_stride, offset, bin, n_bins, d_out, out_wave_stride);
        if (eb != hipSuccess) return eb;
        mark(c.ev, 2, s);
        mark(c.ev, 3, s);
        return hipGetLastError();
    }
    // ---- the kernel: a wavefront per 64 waveforms
    const bool serial = G.n_taps != 0;
    for_wavefront_slices(G, !serial, [&](uint64_t base, unsigned nb) {
        if (serial)
            k_wave_bins_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, d_start, start_stride, offset, bin, n_bins,
                                                 c.d_status, d_out, out_wave_stride);
        else
            k_wave_bins<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, d_start, start_stride, offset, bin, n_bins,
                                          c.d_status, d_out, out_wave_stride);
    });
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
