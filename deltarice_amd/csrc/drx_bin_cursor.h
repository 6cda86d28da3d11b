// drx_bin_cursor.h -- where a sample lies among a waveform's bins (drx_wave_bins; not installed): the origin, and a cursor of
// the next BORDER and the row that is due.  Shared by the lane kernels (drx_bins.hip: a lane walks its waveform from sample 0)
// and the block form (drx_bins_blocks.hip, drx_blocks_bins.inc: a lane walks its share of a block from any sample).  Both depend
// on the geometry alone, never on the stream.  Host and device: tests/bins_rule_host.cpp compiles it for the host and holds it
// to a 128-bit model.
#ifndef DRX_BIN_CURSOR_H
#define DRX_BIN_CURSOR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace drx {

constexpr uint32_t kNoBorder = 0xffffffffu;  // (a waveform has fewer than 2^31 samples)

// a_g = start[g * stride] + offset; the sum saturates (as drx_decode_window's)
__host__ __device__ __forceinline__ int64_t bins_origin(const int64_t *__restrict__ start, uint64_t start_stride, int64_t offset, uint64_t g) {
    int64_t a = offset;
    if (start) {
        const int64_t v = start[g * start_stride];
        if (__builtin_add_overflow(v, offset, &a)) a = v < 0 ? INT64_MIN : INT64_MAX;
    }
    return a;
}

// Where a lane is among its bins.  live: the current stretch of samples is bin `cur`; otherwise it lies in front of bin 0
// (cur == 0, the border is a_g) or behind the last bin (no border is left).  cur is the next row to be written.
struct BinCursor {
    uint32_t nb;   // the sample index at which the current stretch ends; kNoBorder: at the waveform's end
    uint32_t cur;
    bool live;
};
// ... at sample i0 (i0 < len, or 0).  Returns the first bin that receives a sample at or behind i0 -- from i0 == 0: the empty
// rows in front of the first bin that receives a sample at all (n_bins: no bin receives one).
// The ends are formed in 64 bits from values below 2^63 + 2^32: nothing wraps.
__host__ __device__ __forceinline__ uint32_t bins_begin(BinCursor &c, int64_t a, uint32_t bin, uint32_t n_bins, uint32_t len, uint32_t i0) {
    c.nb = kNoBorder;
    c.cur = n_bins;
    c.live = false;
    if (a >= (int64_t)len) return n_bins;  // (len == 0 included)
    c.cur = 0;
    if (a > (int64_t)i0) {  // samples [i0, a) belong to no bin
        c.nb = (uint32_t)a;
        return 0u;
    }
    const uint64_t ua = (uint64_t)i0 - (uint64_t)a;  // (2^63 + i0 for INT64_MIN)
    const uint64_t b0 = ua / bin;
    if (b0 >= n_bins) {
        c.cur = n_bins;
        return n_bins;
    }
    const uint64_t end = (uint64_t)i0 + ((b0 + 1u) * bin - ua);  // i0 + (0, bin]
    c.cur = (uint32_t)b0;
    c.live = true;
    c.nb = end < len ? (uint32_t)end : kNoBorder;
    return (uint32_t)b0;
}
// ... at the border, behind the store of the bin that ends there
__host__ __device__ __forceinline__ void bins_border(BinCursor &c, uint32_t bin, uint32_t n_bins, uint32_t len) {
    const uint64_t end = (uint64_t)c.nb + bin;
    if (c.live) ++c.cur;  // (cur < n_bins while live)
    c.live = c.cur < n_bins;
    c.nb = (c.live && end < len) ? (uint32_t)end : kNoBorder;
}

}  // namespace drx
#endif
