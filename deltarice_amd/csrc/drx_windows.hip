// drx_windows.hip -- SEVERAL windows of every waveform, at per-window starts, straight from the encoded stream
// (drx_decode_windows): waveform g has n_win window slots, of which the first min(count[g], n_win) are live; it is parsed as
// drx_decode parses it, from its first code to the last code of its last window (sample e_g, the largest window end) and no
// further, and the `width` samples of every live window go to that window's row (`pad` where the window leaves the waveform, and
// all over a row that is not live).  The starts are taken as drx_find_pulses writes them, so the samples around every pulse of
// every waveform come with no host round trip and without decoding the batch to memory.
//
// The header tables (wave_off / wave_words) are valid for the whole batch: the host runs the walk in front of this launch
// (launch_decode_windows(): the walks of drx_walk.hip, or the side-band's tables), as launch_decode_window() does.
//
//   k_decode_windows         delta filter: one LANE per waveform, 64 waveforms per wavefront, the stream side the shared reader's
//                            early-ending form (drx_lane_reader.inc with DRX_LANE_EARLY) as in k_decode_window: a lane ends
//                            behind e_g and a wavefront runs wave_max(e_g) samples.  In its prologue a lane reads its live
//                            starts once: e_g, whether they are non-decreasing, and the pads and dead rows.  A SORTED list
//                            (as drx_find_pulses numbers its pulses) takes a cursor: the current window's [s, e) and row and
//                            the next window's start stay in registers, and a group of 16 samples that touches no window
//                            costs one compare.  A group in which windows overlap takes a plain loop over the windows
//                            concerned, and every group of an UNSORTED list a scan of all live windows.
//   k_decode_windows_list    the same kernel over a device list of waveforms: behind the block form (drx_windows_blocks.hip),
//                            which lists the waveforms it flagged; their rows are written again, all of them, and judged here.
//   k_decode_windows_serial  every other prediction filter: one lane per waveform, the serial parse of the same header to e_g
//                            inside the serial kernels' frame (serial_frame(), drx_lane_stream.h), with a sink that loops
//                            over the live windows.  Correct, not tuned.
//
// Few long waveforms under the delta filter (the batches drx_wave_stats gives to its block form) take the block form of
// drx_windows_blocks.hip: a workgroup per block of a waveform's stream, which puts its samples in order only where a window
// meets the block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"
#include "drx_lane_stream.h"
#include "drx_window_rows.h"

namespace drx {

// A lane's prologue: its live starts, read once.  Writes the pads of every live row and the whole of every dead one; returns e_g
// (0: no window holds a sample), and leaves the number of live slots and whether their starts are non-decreasing.
__device__ __forceinline__ uint32_t windows_prologue(const WinList &wl, uint64_t g, uint32_t len, uint32_t &nlive, bool &sorted) {
    nlive = wl.live(g);
    sorted = true;
    uint32_t e = 0;
    int64_t prev = INT64_MIN;
    for (uint32_t p = 0; p < wl.n_win; ++p) {
        int16_t *row = wl.row(g, p);
        if (p < nlive) {
            const int64_t a = wl.at(g, p);
            const Win w = window_at(a, wl.width, len);
            fill_pad(row, 0u, w.pf, wl.pad2);
            fill_pad(row, w.pf + (w.e - w.s), wl.width, wl.pad2);
            e = w.e > e ? w.e : e;
            sorted = sorted && a >= prev;
            prev = a;
        } else {
            fill_pad(row, 0u, wl.width, wl.pad2);
        }
    }
    return e;
}

// Lanes map by LANE_WAVE_G_ACTIVE_LEN (drx_lane_stream.h).  wf_base: first wavefront of this launch (for_wavefront_slices()).
// The body is drx_windows_lane_body.inc; the stores: a group that lies inside a window whose row puts it on a dword boundary goes
// out as eight dword stores, every other group that meets a window as 2-byte stores under a compare per sample.
__global__ __launch_bounds__(64) void k_decode_windows(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                       const uint64_t *__restrict__ wave_off,
                                                       const uint32_t *__restrict__ wave_words, uint64_t wf_base, WinList wl,
                                                       DevStatus *st) {
    constexpr bool LIST = false;
    const uint32_t *const list = nullptr, *const n_list = nullptr;
#include "drx_windows_lane_body.inc"
}

// The same kernel over the waveforms list[0 .. *n_list) instead of all of them (behind the block form: the list and its length
// are written on the device by the kernel in front; the launch is sized for the whole batch).  Every lane reads its own stream
// through its own ring column, so the lanes of a wavefront may hold any waveforms.  Lane 0 of the launch leaves the list's length
// in the status word for drx_plan_last_windows_listed.
__global__ __launch_bounds__(64) void k_decode_windows_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                            const uint64_t *__restrict__ wave_off,
                                                            const uint32_t *__restrict__ wave_words, uint64_t wf_base, WinList wl,
                                                            DevStatus *st, const uint32_t *__restrict__ list,
                                                            const uint32_t *__restrict__ n_list) {
    constexpr bool LIST = true;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->listed = *n_list;
#include "drx_windows_lane_body.inc"
}

// General prediction filters: serial_frame() (drx_lane_stream.h) to e_g behind the lane's prologue; 2-byte stores, a loop over
// the live windows per sample.
__global__ __launch_bounds__(64) void k_decode_windows_serial(Geom G, const uint32_t *__restrict__ in,
                                                              const uint64_t *__restrict__ wave_off,
                                                              const uint32_t *__restrict__ wave_words, uint64_t wf_base, WinList wl,
                                                              DevStatus *st) {
    uint64_t g = 0;
    uint32_t len = 0, nlive = 0;
    bool sorted;
    serial_frame(
        G, in, wave_off, wave_words, wf_base, (const uint32_t *)nullptr, 0u, st,
        [&](uint64_t g_, const WaveRef &r) __attribute__((always_inline)) {
            g = g_;
            len = r.len;
            return windows_prologue(wl, g, len, nlive, sorted);
        },
        [&](uint32_t i, int16_t y) __attribute__((always_inline)) {
            for (uint32_t p = 0; p < nlive; ++p) {
                const Win w = window_at(wl.at(g, p), wl.width, len);
                if (i >= w.s && i < w.e) wl.row(g, p)[(int64_t)w.pf + ((int64_t)i - (int64_t)w.s)] = y;
            }
        },
        [](uint64_t, const WaveRef &) {});
}

hipError_t launch_decode_windows(const StreamCall &c, void *d_blk, void *d_wtab, const int64_t *d_start, uint64_t start_wave_stride,
                                 uint64_t start_win_stride, const uint32_t *d_count, uint32_t n_win, int64_t offset, uint32_t width,
                                 int16_t pad, int16_t *d_out, uint64_t out_wave_stride, uint64_t out_win_stride, uint32_t *form_out) {
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    const bool blocks = d_wtab != nullptr && blocks_form_batch(G, d_blk, kWindowsForm);
    if (form_out) *form_out = blocks_form_word(G, blocks, kWindowsForm);
    if (G.total_waves == 0) return hipSuccess;
    // ---- the walk (drx_walk.hip): launch_batch_walk()
    hipError_t e = batch_walk_prologue(c);
    if (e != hipSuccess) return e;
    const WinList wl{d_start, start_wave_stride, start_win_stride, d_count, n_win, width, offset, (uint32_t)(uint16_t)pad * 0x10001u,
                     d_out, out_wave_stride, out_win_stride};
    if (blocks) {
        // ---- few long waveforms: the pads, a workgroup per block of a waveform's stream, then a lane per waveform that form lists
        // (the launch is sized from here, at most a lane per waveform of the batch; the list's length is read on the device)
        BlkFallbackList fl;
        if ((e = launch_windows_blocks(c, d_blk, d_wtab, wl, &fl)) != hipSuccess) return e;
        k_decode_windows_list<<<blocks_for(G.total_waves, 64), 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, 0, wl, c.d_status,
                                                                          fl.listed, fl.n_listed);
    } else {
        // ---- the kernel: a wavefront per 64 waveforms
        const bool serial = G.n_taps != 0;
        for_wavefront_slices(G, !serial, [&](uint64_t base, unsigned nb) {
            if (serial)
                k_decode_windows_serial<<<nb, 64, 0, s>>>(G, c.d_in, c.d_wave_off, c.d_wave_words, base, wl, c.d_status);
            else
                k_decode_windows<<<nb, 64, 0, s>>>(G, c.d_in, c.in_words, c.d_wave_off, c.d_wave_words, base, wl, c.d_status);
        });
    }
    mark(c.ev, 2, s);
    mark(c.ev, 3, s);
    return hipGetLastError();
}

}  // namespace drx
