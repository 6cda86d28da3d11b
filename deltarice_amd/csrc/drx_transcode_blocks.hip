// drx_transcode_blocks.hip -- drx_transcode and drx_estimate_words_encoded for few long waveforms: a WORKGROUP per block of a
// waveform's stream.
//
// A lane per waveform (k_recode_sizes / k_recode_pack, drx_transcode.hip) parses twice and emits once at a lane's pace whatever
// else runs; the reference's default options (one waveform per chunk) keep a few dozen of the chip's 98 304 lane slots busy.  The
// batches that drx_decode gives to the block decoder (blocks_batch(), drx_blocks.hip) take this form instead, under EVERY
// prediction filter the plan accepts: the parse of a re-code is on residuals (RESID) and has no filter arithmetic.
//
//   k_trc_blocks, sizes      the block decoder's phase 1, look-back and flags, word for word (drx_blocks_body.inc).  Phase 2
//                            (drx_blocks_trc.inc): a lane adds the code lengths of its residuals at the new parameter -- from the
//                            int16 pairs phase 1 staged, or, where some lane holds more codes than its share, from a second parse --
//                            and the block leaves its bit count in its slot of a table, with what its second run starts from:
//                            where its first code starts, its first sample's index, its sample count.  ALLK (the estimate):
//                            sixteen counts per lane into the waveform's [16] accumulators by 64-bit integer atomics.
//   k_trc_blocks_finish      a thread per waveform.  A waveform that is flagged, suspect or has samples and no payload word goes
//                            on the list of the lane kernels (every one under DRX_DBG_TRANSCODE_ALL_FALLBACK); for every other
//                            one the exclusive scan of its blocks' bit counts replaces them in the table and n_i' = ceil(bits / 32)
//                            goes to the result's tables -- or, the estimate, 1 + ceil(bits / 32) words and a word per chunk go to
//                            est[k], as k_recode_sizes<true> counts them.
//   (k_recode_sizes over the list for the listed waveforms' n_i' or sums and for their VERDICT, then the scan of
//   launch_chunk_offsets(): every kErrCorrupt and kErrCapacity is raised before any kernel touches d_out)
//   k_trc_blocks_layout      a thread per block slot, gated on the status word: the headers n_i' and N_c of the waveforms the
//                            blocks keep, and a zero in every word of the result that two blocks share -- the word a block's first
//                            bit lies in where that bit is not a word's first, likewise behind its last bit.  All inside the
//                            waveform's own n_i' words.
//   k_trc_blocks, pack       the scheme again with every look-back, spin and flag switched off: a run's first block takes its
//                            start, its first sample's index and its bit offset from its slot, so the result does not depend on
//                            which waveforms a launch happened to flag.  A scan of the lanes' bits places every lane's first code;
//                            the lanes parse their codes again and OR whole words into the cleared staging buffer, which is drained
//                            in passes (a block is a fixed number of INPUT bits; at a small new parameter its output is many times
//                            that).  The staging buffer is the one the decoder has, so as many workgroups are resident.  Interior
//                            words go out once, by 16-byte stores where four lie inside; the block's first and last word, where
//                            shared, by atomic OR into the words the layout kernel cleared.
//   (k_recode_pack over the list writes the listed waveforms, every word of their regions by plain stores)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_blocks.h"

namespace drx {

template <int NT, int SW, class TA>
__global__ __launch_bounds__(NT) void k_trc_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                   const uint64_t *__restrict__ wave_off,
                                                   const uint32_t *__restrict__ wave_words,
                                                   const uint32_t *__restrict__ info, uint32_t slots_per_wave,
                                                   uint32_t run_len, uint64_t *__restrict__ state,
                                                   uint32_t *__restrict__ ends, uint32_t *__restrict__ ticket,
                                                   uint32_t *__restrict__ fail, uint32_t *__restrict__ suspect,
                                                   DevStatus *st, TA ta_, uint32_t n_list, const uint32_t *__restrict__ wave_list) {
    constexpr bool RESID = true, FUSE = false, STATS = false, PULSES = false, WINDOWS = false, TRANSCODE = true, BINS = false;
    // what the decoder's phase 2 and its fused inverse filter take: not used here
    int16_t *const out = nullptr;
    const uint32_t *const itab = nullptr;
    uint64_t *const xstate = nullptr;
    const BlkStatsArgs sa{0u, nullptr};
    const BlkPulseArgs pa{};
    const BlkWindowArgs wa{};
    const TA ta = ta_;
    const BlkBinsArgs ba{};
    // whatever a walker reported, and (the pack launch) kErrCorrupt or kErrCapacity: then no word of the result is written
    if (st->err) return;
#include "drx_blocks_body.inc"
}

// A thread per waveform behind the sizes launch (see the head comment).  est != nullptr: the estimate.
__global__ __launch_bounds__(256) void k_trc_blocks_finish(Geom G, const uint32_t *__restrict__ wave_words, const uint32_t *__restrict__ fail,
                                                           const uint32_t *__restrict__ suspect, uint32_t all_listed,
                                                           uint32_t *__restrict__ n_listed, uint32_t *__restrict__ listed,
                                                           uint32_t *__restrict__ keep, const uint32_t *__restrict__ n_blocks,
                                                           uint32_t *__restrict__ slots, uint32_t slots_per_wave,
                                                           const unsigned long long *__restrict__ acc16, const DevStatus *st,
                                                           uint32_t *__restrict__ new_words, uint32_t *__restrict__ out_wave_words,
                                                           unsigned long long *__restrict__ est) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (st->err) return;  // (as k_trc_blocks)
    if (g >= G.total_waves) return;
    const WaveRef r = locate(G, g);
    if (blk_listed(all_listed, fail, suspect, g, [&]() { return r.len != 0u && wave_words[g] == 0u; })) {
        keep[g] = 0u;
        blk_list_append(n_listed, listed, (uint32_t)g);
        return;
    }
    keep[g] = 1u;
    if (est) {
        for (int j = 0; j < 16; ++j)
            atomicAdd(est + j, (unsigned long long)(1u + ((acc16[16u * g + (uint32_t)j] + 31u) >> 5) + (r.idx == 0u ? 1u : 0u)));
        return;
    }
    uint64_t off = 0;
    uint32_t *sl = slots + g * slots_per_wave * (uint64_t)kTrcSlotWords;
    for (uint32_t b = 0, nb = n_blocks[g]; b < nb; ++b, sl += kTrcSlotWords) {
        const uint32_t bits = sl[2];
        sl[0] = (uint32_t)off;
        sl[1] = (uint32_t)(off >> 32);
        off += bits;
    }
    const uint32_t nw = (uint32_t)((off + 31u) >> 5);
    new_words[g] = nw;
    if (out_wave_words) out_wave_words[g] = nw;
}

// A thread per block slot in front of the pack launch (see the head comment).  Nothing is written where the status word holds an
// error; what is written lies inside the n_i' words of a waveform the blocks keep, or is its header (the chunk's: its first waveform's)
__global__ __launch_bounds__(256) void k_trc_blocks_layout(Geom G, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ n_blocks,
                                                           const uint32_t *__restrict__ slots, uint32_t slots_per_wave, const DevStatus *st,
                                                           const uint32_t *__restrict__ new_words, const uint32_t *__restrict__ new_rel,
                                                           const uint64_t *__restrict__ out_chunk_off, uint32_t *__restrict__ out) {
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (st->err) return;
    const uint64_t g = u / slots_per_wave;
    const uint32_t b = (uint32_t)(u - g * slots_per_wave);
    if (g >= G.total_waves || !keep[g]) return;
    const WaveRef r = locate(G, g);
    const uint64_t pos = out_chunk_off[r.chunk] + new_rel[g];
    if (b == 0u) {
        out[pos] = new_words[g];                     // :379
        if (r.idx == 0u) out[pos - 1u] = r.n_samples;  // chunk header, :415
    }
    if (b >= n_blocks[g]) return;
    const uint32_t *sl = slots + u * kTrcSlotWords;
    const uint64_t o = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
    const uint32_t bits = sl[2];
    if (bits == 0u) return;
    if (o & 31u) out[pos + 1u + (o >> 5)] = 0u;
    if ((o + bits) & 31u) out[pos + 1u + ((o + bits) >> 5)] = 0u;
}

// the plan's scratch of this form: u64 acc16[W][16] | u32 n_blocks[W] | u32 keep[W] | the fallback list | u32 slots[block slots][kTrcSlotWords]
struct TrcBlkScratch {
    unsigned long long *acc16;
    uint32_t *n_blocks, *keep, *slots;
    BlkFallbackList list;
    uint64_t reset_bytes, bytes;  // reset per call: the accumulators and the block counts
};
static TrcBlkScratch trc_blocks_layout(const Geom &G, void *base) {
    const uint64_t W = G.total_waves;
    TrcBlkScratch L;
    L.acc16 = reinterpret_cast<unsigned long long *>(base);
    L.n_blocks = reinterpret_cast<uint32_t *>(L.acc16 + 16u * W);
    L.keep = L.n_blocks + W;
    L.list = BlkFallbackList::at(L.keep + W + (W & 1u));
    L.slots = L.list.listed + W;
    L.reset_bytes = 128u * W + 4u * W;
    L.bytes = 128u * W + 4u * (2u * W + (W & 1u)) + BlkFallbackList::bytes(W) + 4ull * kTrcSlotWords * blocks_total_slots(G);
    return L;
}
uint64_t trc_blocks_scratch_bytes(const Geom &G) { return trc_blocks_layout(G, nullptr).bytes; }

hipError_t launch_trc_blocks_sizes(const StreamCall &call, void *d_blk, void *d_tb, uint32_t k2, const TrcScratch &t, uint32_t *d_out_wave_words,
                                   unsigned long long *d_est, BlkFallbackList *list_out) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    const TrcBlkScratch A = trc_blocks_layout(G, d_tb);
    hipError_t e = hipMemsetAsync(A.acc16, 0, A.reset_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(A.list.n_listed, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    BlkTables T;
    BlkClassLaunch cls[kBlkMaxClasses];
    uint32_t n_cls = 0;
    if ((e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls)) != hipSuccess) return e;
    uint32_t spw = 1;
    for (uint32_t i = 0; i < n_cls; ++i) {
        const BlkClassLaunch &c = cls[i];
        spw = c.spw;
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            auto go = [&](auto ta) {
                ta.k2 = k2; ta.pack = 0u; ta.slots = A.slots; ta.n_blocks = A.n_blocks; ta.acc16 = A.acc16;
                ta.keep = nullptr; ta.new_rel = nullptr; ta.out_chunk_off = nullptr; ta.outw = nullptr;
                k_trc_blocks<NT, SW, decltype(ta)><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw,
                                                                         c.run_len, T.state, T.ends, c.info + 2, T.fail, T.suspect, call.d_status, ta,
                                                                         c.n_waves, c.list);
            };
            if (d_est) go(BlkTrcAllKArgs{});
            else go(BlkTrcArgs{});
        });
    }
    k_trc_blocks_finish<<<blocks_for(G.total_waves, 256), 256, 0, s>>>(G, call.d_wave_words, T.fail, T.suspect,
                                                                        (G.dbg & kTranscodeForm.all_fallback_flag) ? 1u : 0u, A.list.n_listed,
                                                                        A.list.listed, A.keep, A.n_blocks, A.slots, spw, A.acc16, call.d_status, t.words,
                                                                        d_out_wave_words, d_est);
    *list_out = A.list;
    return hipGetLastError();
}

hipError_t launch_trc_blocks_pack(const StreamCall &call, void *d_blk, void *d_tb, uint32_t k2, const TrcScratch &t, const EncOut &out) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    const TrcBlkScratch A = trc_blocks_layout(G, d_tb);
    // the launches of the scheme again: the decoder's scratch is reset (tickets; the pack launch reads nothing else of it)
    BlkTables T;
    BlkClassLaunch cls[kBlkMaxClasses];
    uint32_t n_cls = 0;
    const hipError_t e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls);
    if (e != hipSuccess) return e;
    const uint32_t spw = n_cls ? cls[0].spw : 1u;
    k_trc_blocks_layout<<<blocks_for(G.total_waves * spw, 256), 256, 0, s>>>(G, A.keep, A.n_blocks, A.slots, spw, call.d_status, t.words, t.rel,
                                                                            out.d_chunk_word_off, out.d_out);
    for (uint32_t i = 0; i < n_cls; ++i) {
        const BlkClassLaunch &c = cls[i];
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            BlkTrcArgs ta{};
            ta.k2 = k2; ta.pack = 1u; ta.slots = A.slots; ta.n_blocks = A.n_blocks; ta.acc16 = nullptr;
            ta.keep = A.keep; ta.new_rel = t.rel; ta.out_chunk_off = out.d_chunk_word_off; ta.outw = out.d_out;
            k_trc_blocks<NT, SW, BlkTrcArgs><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw, c.run_len,
                                                                   T.state, T.ends, c.info + 2, T.fail, T.suspect, call.d_status, ta, c.n_waves, c.list);
        });
    }
    return hipGetLastError();
}

}  // namespace drx
