// drx_lane_stream.h -- the stream side of the kernels that read an encoded batch a LANE per waveform without decoding it to
// memory.  Two families use it:
//   the delta filter's tuned kernels, over the shared reader -- the lane's LDS ring and its two extractions, the text of
//     drx_lane_reader.inc included in each kernel's body: k_wave_stats (drx_stats.hip), k_wave_bins (drx_bins.hip),
//     k_decode_window (drx_window.hip), k_decode_windows and k_decode_windows_list (drx_windows.hip), k_find_pulses and
//     k_find_pulses_list (drx_pulses.hip), k_recode_sizes and k_recode_pack (drx_transcode.hip), k_refilter_sizes and
//     k_refilter_pack (drx_refilter.hip; the shared bodies of those four are drx_recode.h);
//   the general prediction filters' serial kernels, over serial_wave(): k_wave_stats_serial, k_decode_windows_serial and
//     k_select_serial (drx_select.hip) inside one frame, serial_frame(); k_wave_bins_serial, k_decode_window_serial,
//     k_find_pulses_serial, k_refilter_sizes_serial and k_refilter_pack_serial with a frame of their own, for the reasons
//     given at serial_frame().
// Here: the reader's constants, which waveform a lane takes (lane_wave()), the packed-pair helpers, the serial parse and its
// frame.  What a kernel does with its samples stays in its own file.  k_decode_lanes (drx_decode_kernels.hip) has a ring of its
// own: it carries the transposition buffer, the start delay and the in-launch walkers.  Not installed.
#ifndef DRX_LANE_STREAM_H
#define DRX_LANE_STREAM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_internal.h"
#include "drx_device.h"

namespace drx {

constexpr int kRW = 64;      // ring words per lane
constexpr int kLW = 32;      // words per stream piece: one 128-byte line
constexpr int kGS = 16;      // samples per group (a refill test per group)
constexpr int kT = 64;       // samples per round (a piece is committed and the next requested per round)
constexpr int kLogRW = 6;
constexpr int kNV = kLW / 4;  // 16-byte loads per piece
constexpr uint32_t kWMask = (1u << 27) - 1u;
constexpr uint32_t kNeedAt = kGS + 2;  // must refill below this many words (16 codes of 25 bits: 12.5 words; a pair reads three)
static_assert(kT % kGS == 0 && kRW - kLW >= kGS + 2, "round length / ring slack");
// row r: word w with kRW - (w mod kRW) == r; row 0 mirrors row kRW and row -1 mirrors row kRW - 1 (a pair reads three
// consecutive words: rows r + 1, r, r - 1).  A lane reads and writes its own column only.  The kernel declares
// __shared__ uint32_t ring_all[kInRingWords] -- all the LDS the reader needs, 16 896 bytes -- and ring = ring_all + 64.
constexpr int kInRingWords = (kRW + 2) * 64;

// A group's samples two to a register (pr[] of LANE_GROUP_PAIRS, drx_lane_reader.inc), as the packed reductions take them
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_pair(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ uint32_t as_word(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
constexpr int32_t kNarrow = 16383;  // sixteen squares of samples within +-kNarrow sum to less than 2^32
static_assert(16ll * kNarrow * kNarrow < (1ll << 32), "a narrow group's sum of squares fits 32 bits");

// Which waveform a lane takes.  Lanes map plainly, g = 64 * wavefront + lane (chunks need no alignment to wavefronts: a
// wavefront's lanes may lie in two chunks, and the short last waveform of a chunk is a lane like any other); a ragged plan that
// has rag_order takes its {chunk, group of 64 waveforms} entries instead, longest WaveformLength first (a lane takes ~60 ns per
// sample, so the wavefronts of the longest waveforms must not start last).  false: the launch has no such wavefront.
struct LaneWave {
    uint64_t g, chunk;
    uint32_t idx, len, n_samples;
    bool active;
};
__device__ __forceinline__ bool lane_wave(const Geom &G, uint64_t wf, int lane, LaneWave &w) {
    w.g = 0; w.chunk = 0; w.idx = 0; w.len = 0; w.n_samples = 0;
    if (!G.uniform && G.rag_order) {
        if (wf >= G.rag_groups) return false;
        const uint2 e = G.rag_order[wf];  // {chunk, group of 64 waveforms inside it}
        const ChunkDesc d = G.chunks[e.x];
        w.idx = e.y * 64u + (uint32_t)lane;
        w.active = w.idx < d.n_waves;
        w.g = d.wave_base + w.idx;
        w.chunk = e.x;
        w.n_samples = d.n_samples;
        if (w.active) w.len = (w.idx + 1 == d.n_waves) ? (d.n_samples - w.idx * d.wave_len) : d.wave_len;
    } else {
        w.g = wf * 64u + (uint32_t)lane;
        w.active = w.g < G.total_waves;
        if (w.active) {
            const WaveRef r = locate(G, w.g);
            w.chunk = r.chunk; w.idx = r.idx; w.len = r.len; w.n_samples = r.n_samples;
        }
    }
    return true;
}

// The same mapping as statements of the kernel's body, for the kernels that need g, active and len alone (k_wave_stats,
// k_decode_window, k_find_pulses): it declares them, and returns from the kernel where the launch has no such wavefront.
// (Through the inlined function these three kernels compile to another block order and register allocation than they had;
// written out they keep their instructions: profiles/lane_stream_refactor_ab.txt.)
#define LANE_WAVE_G_ACTIVE_LEN(G, wf_, lane)                                                                          \
    const uint64_t wf = (wf_);                                                                                        \
    uint64_t g;                                                                                                       \
    bool active;                                                                                                      \
    uint32_t len = 0;                                                                                                 \
    if (!G.uniform && G.rag_order) {                                                                                  \
        if (wf >= G.rag_groups) return;                                                                               \
        const uint2 e_ = G.rag_order[wf]; /* {chunk, group of 64 waveforms inside it} */                             \
        const ChunkDesc d_ = G.chunks[e_.x];                                                                          \
        const uint32_t idx_ = e_.y * 64u + (uint32_t)lane;                                                            \
        active = idx_ < d_.n_waves;                                                                                   \
        g = d_.wave_base + idx_;                                                                                      \
        if (active) len = (idx_ + 1 == d_.n_waves) ? (d_.n_samples - idx_ * d_.wave_len) : d_.wave_len;               \
    } else {                                                                                                          \
        g = wf * 64u + (uint32_t)lane;                                                                                \
        active = g < G.total_waves;                                                                                   \
        if (active) len = locate(G, g).len;                                                                           \
    }

// The serial parse of one waveform: the kernels of the general prediction filters, a lane per waveform, global loads.
// Correct, not tuned.  s: the payload's first word, n: its words, len: the samples to parse (from the waveform's first).
// hist: the lane's own 64 int16 of filter history, `hist_stride` elements apart (an LDS column; general filters only,
// taps <= DRX_MAX_TAPS = 64).  sink(i, y) receives the sample drx_decode writes, in order.  Returns the payload words the
// codes took: a valid waveform's end in its last word, n_i = ceil(bits / 32) (src/deltaRice.c:237-241).
template <typename Sink>
__device__ __forceinline__ uint64_t serial_wave(const Geom &G, const uint32_t *__restrict__ s, uint32_t n, uint32_t len, int16_t *hist,
                                                uint32_t hist_stride, Sink &&sink) {
    const uint32_t k = G.k;
    uint64_t win = 0;
    uint32_t have = 0, wi = 0;
    int32_t acc = 0;
    for (uint32_t i = 0; i < len; ++i) {
        if (have <= 32u) {
            const uint32_t w = wi < n ? s[wi] : 0u;
            ++wi;
            win |= (uint64_t)w << (32u - have);
            have += 32u;
        }
        uint32_t q = (uint32_t)__clzll((long long)win);
        q = q > 8u ? 8u : q;
        const uint32_t pl = (q == 8u) ? 16u : k;
        const uint64_t t = win << (q + 1u);
        const uint32_t rem = pl ? (uint32_t)(t >> (64u - pl)) : 0u;
        const uint32_t z = (q == 8u) ? rem : ((q << k) + rem);
        const int32_t d = (int32_t)(z >> 1) ^ -(int32_t)(z & 1u);  // un-zig-zag (:172-177)
        if (G.n_taps == 0) {
            acc += d;  // running sum (:80-89)
        } else {
            // general inverse (:92-101): y[i] = (int16)((int16)(d[i] - sum_{j>=1} taps[j] y[i-j]) / taps[0])
            uint32_t a = (uint32_t)(int32_t)(int16_t)d;
            for (uint32_t j = 1; j < G.n_taps && j <= i; ++j) a -= (uint32_t)(int32_t)hist[((i - j) & 63u) * hist_stride] * (uint32_t)G.taps[j];
            acc = (int32_t)(int16_t)(uint16_t)a / G.taps[0];
            hist[(i & 63u) * hist_stride] = (int16_t)acc;
        }
        sink(i, (int16_t)acc);
        const uint32_t used = q + 1u + pl;
        win <<= used;
        have -= used;
    }
    return (32ull * wi - have + 31u) >> 5;
}

// The frame of a serial kernel: everything round serial_wave() but what the call does with a sample.  Lane j = 64 * (wf_base +
// workgroup) + lane of the launch takes waveform g = j, or g = list[j], j < n_list, where the launch has a list (the waveforms
// a block form lists; a caller's selection).  Nothing is followed into the stream once st->err is set -- whatever a walker
// reported, the tables of a batch that failed validation are not valid -- and no table is indexed with a g outside the batch.
// The filter's history, the last 64 outputs of every lane, is an LDS column here (8192 bytes; taps <= DRX_MAX_TAPS = 64).
// What the call supplies:
//   begin(g, r)   in front of the parse -- pads, empty rows, the lane's state; returns e, the samples to parse from the
//                 waveform's first.  e == 0: the lane parses nothing, reads no header table entry and makes no verdict.
//   sample(i, y)  the sample drx_decode writes, for i = 0 .. e - 1 in order
//   end(g, r)     behind the parse and the verdict: the row or count store, a run still open closed at r.len
// The verdict, once: a valid waveform's codes end inside its last payload word, so a lane that parsed to its waveform's end
// asks words == n_i; one that stopped early asks only that its codes lay inside the payload, words <= n_i (nothing behind
// its last code is looked at).
// Not on this frame: k_refilter_sizes_serial (its lanes without a waveform stay for the wavefront's sums, and its sink reads the
// history column) and k_refilter_pack_serial (no verdict of its own -- the sizes pass has made it -- and an OutRing beside the
// column); k_wave_bins_serial, k_decode_window_serial and k_find_pulses_serial, which fit it and were measured 0.4, 0.9 and
// 2.8 % slower through it (profiles/serial_frame_refactor_ab.txt: the same loop instructions at other addresses), so they
// keep the bodies they had.  A new serial kernel starts on the frame.
template <typename T, typename Begin, typename Sample, typename End>
__device__ __forceinline__ void serial_frame(const Geom &G, const uint32_t *__restrict__ in, const uint64_t *__restrict__ wave_off,
                                             const uint32_t *__restrict__ wave_words, uint64_t wf_base, const T *__restrict__ list,
                                             uint64_t n_list, DevStatus *st, Begin &&begin, Sample &&sample, End &&end) {
    __shared__ int16_t hist[64][64];  // [sample mod 64][lane]
    const uint32_t lane = threadIdx.x;
    uint64_t g = (wf_base + blockIdx.x) * 64u + lane;
    if (st->err) return;
    if (list) {
        if (g >= n_list) return;
        g = list[g];
    }
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    const uint32_t e = begin(g, r);
    if (e) {
        const uint32_t n = wave_words[g];
        const uint64_t words = serial_wave(G, in + wave_off[g] + 1, n, e, &hist[0][lane], 64u, sample);
        if (e == r.len ? words != n : words > n) atomicOr(&st->err, kErrCorrupt);
    }
    end(g, r);
}

}  // namespace drx
#endif
