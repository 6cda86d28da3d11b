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
#include "drx_recode.h"

namespace drx {

// The bodies are recode_sizes() and recode_pack() of drx_recode.h over the residuals as they are (SameValue); each has two
// instantiations here, over the whole batch and over a list.
template <bool ALLK>
__global__ __launch_bounds__(64) void k_recode_sizes(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                     const uint64_t *__restrict__ wave_off,
                                                     const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                     DevStatus *st, uint32_t *__restrict__ new_words,
                                                     uint32_t *__restrict__ out_wave_words,
                                                     unsigned long long *__restrict__ est) {
    recode_sizes<ALLK, false>(G, in, in_words, wave_off, wave_words, wf_base, k2, st, new_words, out_wave_words, est, nullptr, nullptr, SameValue{});
}
template <bool ALLK>
__global__ __launch_bounds__(64) void k_recode_sizes_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                          const uint64_t *__restrict__ wave_off,
                                                          const uint32_t *__restrict__ wave_words, uint32_t k2, DevStatus *st,
                                                          uint32_t *__restrict__ new_words, uint32_t *__restrict__ out_wave_words,
                                                          unsigned long long *__restrict__ est, const uint32_t *__restrict__ list,
                                                          const uint32_t *__restrict__ n_list) {
    recode_sizes<ALLK, true>(G, in, in_words, wave_off, wave_words, 0u, k2, st, new_words, out_wave_words, est, list, n_list, SameValue{});
}

__global__ __launch_bounds__(64) void k_recode_pack(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                    const uint64_t *__restrict__ wave_off,
                                                    const uint32_t *__restrict__ wave_words, uint64_t wf_base, uint32_t k2,
                                                    const DevStatus *st, const uint32_t *__restrict__ new_words,
                                                    const uint32_t *__restrict__ new_rel,
                                                    const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out) {
    recode_pack<false>(G, in, in_words, wave_off, wave_words, wf_base, k2, st, new_words, new_rel, out_chunk_off, out, nullptr, nullptr, SameValue{});
}
__global__ __launch_bounds__(64) void k_recode_pack_list(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                         const uint64_t *__restrict__ wave_off,
                                                         const uint32_t *__restrict__ wave_words, uint32_t k2, const DevStatus *st,
                                                         const uint32_t *__restrict__ new_words, const uint32_t *__restrict__ new_rel,
                                                         const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out,
                                                         const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    recode_pack<true>(G, in, in_words, wave_off, wave_words, 0u, k2, st, new_words, new_rel, out_chunk_off, out, list, n_list, SameValue{});
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
