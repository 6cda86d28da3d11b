// drx_window_rows.h -- what a window is and how a row's pads are written, shared by the kernels of drx_decode_window
// (drx_window.hip) and drx_decode_windows (drx_windows.hip, drx_windows_blocks.hip, drx_blocks_body.inc).  Not installed.
#ifndef DRX_WINDOW_ROWS_H
#define DRX_WINDOW_ROWS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace drx {

// Samples [s, e) of the waveform go to row elements [pf, pf + e - s); pad fills [0, pf) and [pf + e - s, width).  A window
// that holds no sample of the waveform is s = e = 0, pf = width: the lane parses nothing.
struct Win {
    uint32_t s, e, pf;
};
// start + offset, saturating at the int64 ends
__device__ __forceinline__ int64_t window_start(int64_t v, int64_t offset) {
    int64_t a;
    if (__builtin_add_overflow(v, offset, &a)) a = v < 0 ? INT64_MIN : INT64_MAX;
    return a;
}
// the window of `width` samples from sample a on, in a waveform of len samples
__device__ __forceinline__ Win window_at(int64_t a, uint32_t width, uint32_t len) {
    Win w = {0u, 0u, width};
    if (a >= (int64_t)len) return w;
    const int64_t t = a + (int64_t)width;  // (a < 2^31: no overflow)
    if (t <= 0) return w;
    w.e = t < (int64_t)len ? (uint32_t)t : len;
    w.s = a < 0 ? 0u : (uint32_t)a;
    w.pf = a < 0 ? (uint32_t)(0 - a) : 0u;  // (0 < -a < width here)
    return w;
}

// row elements [from, to) = pad: dword stores between a 2-byte store at either end where the address asks for one
__device__ __forceinline__ void fill_pad(int16_t *row, uint32_t from, uint32_t to, uint32_t pad2) {
    if (from >= to) return;
    if ((((uintptr_t)row >> 1) + from) & 1u) row[from++] = (int16_t)pad2;
    for (; from + 2u <= to; from += 2u) *(uint32_t *)(row + from) = pad2;
    if (from < to) row[from] = (int16_t)pad2;
}

// drx_decode_windows: K window slots per waveform.  Slot p of waveform g is LIVE when p < min(count[g], n_win) (count ==
// nullptr: every slot); a live window starts at start[g * start_wave_stride + p * start_win_stride] + offset (saturating) and
// its row is out + g * out_wave_stride + p * out_win_stride.  Passed to the kernels by value.
struct WinList {
    const int64_t *start;
    uint64_t start_wave_stride, start_win_stride;
    const uint32_t *count;
    uint32_t n_win, width;
    int64_t offset;
    uint32_t pad2;  // pad in both halves of a dword
    int16_t *out;
    uint64_t out_wave_stride, out_win_stride;

    __device__ __forceinline__ uint32_t live(uint64_t g) const {
        if (!count) return n_win;
        const uint32_t c = count[g];
        return c < n_win ? c : n_win;
    }
    __device__ __forceinline__ int64_t at(uint64_t g, uint32_t p) const {
        return window_start(start[g * start_wave_stride + (uint64_t)p * start_win_stride], offset);
    }
    __device__ __forceinline__ int16_t *row(uint64_t g, uint32_t p) const { return out + g * out_wave_stride + (uint64_t)p * out_win_stride; }
};

}  // namespace drx
#endif
