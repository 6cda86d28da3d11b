// drx_pulses_blocks.hip -- drx_find_pulses for few long waveforms: a WORKGROUP per block of a waveform's stream.
//
// A lane per waveform (k_find_pulses, drx_pulses.hip) takes 50-60 ns per sample whatever else runs; a long trace that holds many
// events is the shape the call is for and the one on which a lane per waveform leaves the chip idle.  The batches that
// drx_wave_stats gives to its block form (blocks_form_batch() under kPulsesForm) take this form:
//
//   k_pulses_blocks   the block decoder's phase 1, look-back and flags, word for word (drx_blocks_body.inc), and a third phase 2
//                     (`if constexpr (PULSES)` there): a fast reject -- no lane of the block holds an over sample, which on
//                     ordinary data is nearly every block -- or a summary per lane (drx_pulse_runs.h), a scan over the lanes
//                     with pulse_combine(), and a second pass over the staged values that stores the pulses closing inside the
//                     block to the block's staging slots under block-relative numbers.  A run does not stop at a block's
//                     border, and a block knows neither what is open in front of it nor how many pulses its waveform has had:
//                     the run that touches its first sample and the run still open at its last one are not emitted but
//                     published, with the number of its own pulses, in the block's summary -- kPulseTabWords uint64 per block
//                     slot, of which pulse_seg_pack() (drx_pulse_runs.h) fills the first kPulseSegWords; plain stores.
//                     Blocks wait for nothing new: the summaries are read behind the kernel's end.
//   k_pulses_stitch   a thread per waveform walks its blocks' summaries in order (pulse_stitch()): joins the runs across the
//                     borders, numbers the pulses by their start, writes the records it put together and copies the staged ones
//                     to their slots, and the count; it leaves every block the number of its first pulse in the table's last
//                     word.  A waveform that is flagged or suspect is appended to a list on the device instead, and nothing
//                     of it is written.
// Listed waveforms are computed again, and JUDGED, by k_find_pulses_list (drx_pulses.hip): the delta filter's lane kernel over
// that list, 48 ns per sample and lane -- a pass that lasts as long as its longest waveform however few lanes run.  Noise and
// quiet data are never flagged.
//
// Staging.  A block stages its first C = min(max_pulses, kPulseStageCap) pulses, C records of DRX_PULSE_COLS int64 per block
// slot; the buffer belongs to the plan and grows when a call needs more.  The cap is DRX_PULSES_STAGE_CAP = 8: at the
// look-back's worst case of 25 bits per sample 2048 waveforms of 500 000 samples have 348 160 block slots, 111 MB of staging at
// the cap beside a decoded batch of 2 GB (DESIGN.md section 4.2i has the measurements at 8, 16 and 32).  Where a block holds
// more than C pulses AND more than C of them are among its waveform's first max_pulses, the stitch cannot fill the slots.  It
// still knows the count and every block's first pulse number, and puts the waveform on a REDO list: launch_pulses_blocks()
// runs k_pulses_blocks a second time over those lists alone (BlkPulseArgs::n_redo), where a block publishes nothing and stores
// pulse r straight to slot first + r of the caller's records, and k_pulses_redo_check behind it counts them for
// drx_plan_last_pulses_redone (and lists one that was flagged this time).  With max_pulses <= 8 that cannot happen and the
// second launch is not made; the counting form (max_pulses = 0) stages nothing.
// Delta filter only, as the block decoder's phase 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drx_blocks.h"

namespace drx {

static_assert(DRX_PULSE_COLS == kPulseRecCols && DRX_PULSE_START == 0 && DRX_PULSE_WIDTH == 1 && DRX_PULSE_PEAK == 2 && DRX_PULSE_ARGPEAK == 3 &&
                  DRX_PULSE_SUM == 4,
              "pulse_record() writes the columns of include/deltarice_hip.h");

constexpr uint32_t kPulseStageCap = DRX_PULSES_STAGE_CAP;

template <int NT, int SW>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void k_pulses_blocks(Geom G, const uint32_t *__restrict__ in, uint64_t in_words,
                                                      const uint64_t *__restrict__ wave_off,
                                                      const uint32_t *__restrict__ wave_words,
                                                      const uint32_t *__restrict__ info, uint32_t slots_per_wave,
                                                      uint32_t run_len, uint64_t *__restrict__ state,
                                                      uint32_t *__restrict__ ends, uint32_t *__restrict__ ticket,
                                                      uint32_t *__restrict__ fail, uint32_t *__restrict__ suspect,
                                                      DevStatus *st, BlkPulseArgs pa, uint32_t n_list,
                                                      const uint32_t *__restrict__ wave_list) {
    constexpr bool RESID = false, FUSE = false, STATS = false, PULSES = true, WINDOWS = false, TRANSCODE = false, BINS = false;
    // what the decoder's phase 2, its fused inverse filter and the statistics form take: not used here
    int16_t *const out = nullptr;
    const uint32_t *const itab = nullptr;
    uint64_t *const xstate = nullptr;
    const BlkStatsArgs sa{0u, nullptr};
    const BlkWindowArgs wa{};
    const BlkTrcArgs ta{};
    const BlkBinsArgs ba{};
    // whatever a walker reported: the tables of a batch that failed validation are not followed into the stream
    if (st->err) return;
#include "drx_blocks_body.inc"
}

// A thread per waveform of the launch (all of the batch, or one length class of a ragged one: the blocks of a class are
// words_per_block payload words each).  all_listed: DRX_DBG_PULSES_ALL_FALLBACK.
__global__ __launch_bounds__(64) void k_pulses_stitch(Geom G, const uint32_t *__restrict__ wave_words, uint32_t n_waves,
                                                      const uint32_t *__restrict__ wave_list, uint32_t words_per_block,
                                                      uint32_t slots_per_wave, uint64_t *__restrict__ table,
                                                      const int64_t *__restrict__ staging, uint32_t cap, uint32_t neg,
                                                      uint32_t min_width, uint32_t max_pulses, const uint32_t *__restrict__ fail,
                                                      const uint32_t *__restrict__ suspect, uint32_t all_listed,
                                                      uint32_t *__restrict__ n_listed, uint32_t *__restrict__ listed,
                                                      uint32_t *__restrict__ n_redo, uint32_t *__restrict__ redo,
                                                      const DevStatus *st, uint32_t *__restrict__ count_out,
                                                      int64_t *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (st->err) return;  // (as k_pulses_blocks)
    if (j >= n_waves) return;
    const uint64_t g = wave_list ? wave_list[j] : j;
    const uint32_t n = wave_words[g];
    const uint32_t n_blocks = (n + words_per_block - 1u) / words_per_block;
    // (a waveform with samples and no payload word has had no block to judge it: the lane kernel does)
    if (blk_listed(all_listed, fail, suspect, g, [&G, g, n_blocks] { return n_blocks == 0u && locate(G, g).len != 0u; })) {
        blk_list_append(n_listed, listed, (uint32_t)g);
        return;
    }
    const uint64_t slot0 = g * (uint64_t)slots_per_wave;
    int64_t *const rows = out + g * (uint64_t)max_pulses * (uint64_t)kPulseRecCols;  // (never followed where max_pulses == 0)
    uint32_t count = 0;
    const bool complete = pulse_stitch(
        n_blocks, min_width, max_pulses, cap,
        [&](uint32_t b) { return pulse_seg_unpack(table + (slot0 + b) * kPulseTabWords); },
        [&](uint32_t p, uint32_t s, uint32_t w, int64_t key, int64_t sum) { pulse_record(rows + (uint64_t)p * kPulseRecCols, s, w, key, sum, neg != 0u); },
        [&](uint32_t b, uint32_t r, uint32_t p) {
            const int64_t *src = staging + ((slot0 + b) * cap + r) * (uint64_t)kPulseRecCols;
            int64_t *dst = rows + (uint64_t)p * kPulseRecCols;
#pragma unroll
            for (int c = 0; c < kPulseRecCols; ++c) dst[c] = src[c];
        },
        [&](uint32_t b, uint32_t first) { table[(slot0 + b) * kPulseTabWords + kPulseSegWords] = (uint64_t)first; },  // (for the second launch)
        &count);
    // a block did not stage a record this waveform needs: the launch's second kernel runs the waveform's blocks again, and they
    // write their pulses to the slots numbered here (the count, and the slots written so far, are exact)
    if (!complete) redo[atomicAdd(n_redo, 1u)] = (uint32_t)g;
    count_out[g] = count;
}

// Behind the second launch, a thread per class of waveforms: how many were run again, for drx_plan_last_pulses_redone; and a
// thread per such waveform: one that the block parse flagged THIS time (its first run was clean: a flag is a matter of timing
// between blocks) joins the list of the lane kernel after all.
__global__ __launch_bounds__(64) void k_pulses_redo_check(uint32_t n_classes, const uint32_t *__restrict__ n_redo,
                                                          const uint32_t *__restrict__ redo, uint32_t class_off, uint32_t cls,
                                                          const uint32_t *__restrict__ fail, const uint32_t *__restrict__ suspect,
                                                          uint32_t *__restrict__ n_listed, uint32_t *__restrict__ listed, DevStatus *st) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (st->err) return;
    if (j == 0u && cls == 0u) {
        uint32_t t = 0;
        for (uint32_t c = 0; c < n_classes; ++c) t += n_redo[c];
        st->redone = t;
    }
    if (j >= n_redo[cls]) return;
    const uint32_t g = redo[class_off + j];
    if (blk_listed(0u, fail, suspect, g)) blk_list_append(n_listed, listed, g);
}

// the plan's scratch of this form: u64 table[block slots][kPulseTabWords] | the fallback list | u32 n_redo[kBlkMaxClasses] |
// u32 redo[W] (class by class, as the launches' own lists lie); the staging buffer is another (it depends on max_pulses)
struct PulseBlkScratch {
    uint64_t *table;
    BlkFallbackList list;
    uint32_t *n_redo, *redo;
    uint64_t bytes;
};
static PulseBlkScratch pulses_blocks_layout(const Geom &G, void *base) {
    const uint64_t slots = blocks_total_slots(G);
    PulseBlkScratch L;
    L.table = reinterpret_cast<uint64_t *>(base);
    L.list = BlkFallbackList::at(L.table + slots * kPulseTabWords);
    L.n_redo = L.list.listed + G.total_waves;
    L.redo = L.n_redo + kBlkMaxClasses;
    L.bytes = slots * kPulseTabWords * 8u + BlkFallbackList::bytes(G.total_waves) + 4u * (G.total_waves + kBlkMaxClasses);
    return L;
}
uint64_t pulses_blocks_scratch_bytes(const Geom &G) { return pulses_blocks_layout(G, nullptr).bytes; }
static uint32_t stage_cap(uint32_t max_pulses) { return max_pulses < kPulseStageCap ? max_pulses : kPulseStageCap; }
uint64_t pulses_blocks_staging_bytes(const Geom &G, uint32_t max_pulses) {
    return blocks_total_slots(G) * stage_cap(max_pulses) * (uint64_t)kPulseRecCols * sizeof(int64_t);
}

// k_pulses_blocks and k_pulses_stitch per launch of the block scheme.  The block decoder's scratch is used as the decoder uses it
// (calls on a plan are ordered on one stream) and reset on the stream first.
hipError_t launch_pulses_blocks(const StreamCall &call, void *d_blk, void *d_ptab, void *d_pstage, const int64_t *d_thr, uint64_t thr_stride,
                                int64_t thr, bool neg, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count, int64_t *d_out,
                                BlkFallbackList *list_out) {
    const Geom &G = *call.G;
    const hipStream_t s = call.s;
    const PulseBlkScratch A = pulses_blocks_layout(G, d_ptab);
    hipError_t e = hipMemsetAsync(A.list.n_listed, 0, 8, s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(A.n_redo, 0, 4u * kBlkMaxClasses, s)) != hipSuccess) return e;
    BlkTables T;
    BlkClassLaunch cls[kBlkMaxClasses];
    uint32_t n_cls = 0;
    if ((e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls)) != hipSuccess) return e;
    const BlkPulseArgs pa{d_thr, thr_stride, thr, neg ? 1u : 0u, min_width, stage_cap(max_pulses), A.table, reinterpret_cast<int64_t *>(d_pstage),
                          nullptr, max_pulses, d_out};
    // the waveforms of a class's launch lie at the same place in the redo list as in the plan's own list
    auto class_off = [&](const BlkClassLaunch &c) { return c.list ? (uint32_t)(c.list - G.rag_blk_list) : 0u; };
    // one launch of the blocks per class: over the class's waveforms, or (again = true) over those of them the stitch put on the redo list
    auto blocks = [&](uint32_t i, bool again) {
        const BlkClassLaunch &c = cls[i];
        BlkPulseArgs a = pa;
        if (again) a.n_redo = A.n_redo + i;
        const uint32_t *list = again ? A.redo + class_off(c) : c.list;
        blk_dispatch(c.nt, c.sw, [&](auto nt_tag, auto sw_tag) {
            constexpr int NT = decltype(nt_tag)::value, SW = decltype(sw_tag)::value;
            k_pulses_blocks<NT, SW><<<c.grid, NT, 0, s>>>(G, call.d_in, call.in_words, call.d_wave_off, call.d_wave_words, c.info, c.spw, c.run_len,
                                                          T.state, T.ends, c.info + 2, T.fail, T.suspect, call.d_status, a, c.n_waves, list);
        });
    };
    for (uint32_t i = 0; i < n_cls; ++i) blocks(i, false);
    for (uint32_t i = 0; i < n_cls; ++i) {
        const BlkClassLaunch &c = cls[i];
        k_pulses_stitch<<<blocks_for(c.n_waves, 64), 64, 0, s>>>(G, call.d_wave_words, c.n_waves, c.list, (uint32_t)c.nt * (uint32_t)c.sw, c.spw, A.table,
                                                                pa.staging, pa.cap, pa.neg, min_width, max_pulses, T.fail, T.suspect,
                                                                (G.dbg & kPulsesForm.all_fallback_flag) ? 1u : 0u, A.list.n_listed, A.list.listed, A.n_redo + i,
                                                                A.redo + class_off(c), call.d_status, d_count, d_out);
    }
    // The second launch, where a block can have staged too few records at all (max_pulses above the cap): the block scheme's
    // scratch reset as for the first, the blocks over the redo lists (a launch whose list is empty ends at its first ticket),
    // and the check behind them.
    if (max_pulses > pa.cap) {
        if ((e = blocks_prepare(G, call.in_words, call.d_wave_words, d_blk, s, &T, cls, &n_cls)) != hipSuccess) return e;
        for (uint32_t i = 0; i < n_cls; ++i) blocks(i, true);
        for (uint32_t i = 0; i < n_cls; ++i)
            k_pulses_redo_check<<<blocks_for(cls[i].n_waves, 64), 64, 0, s>>>(n_cls, A.n_redo, A.redo, class_off(cls[i]), i, T.fail, T.suspect, A.list.n_listed,
                                                                             A.list.listed, call.d_status);
    }
    *list_out = A.list;
    return hipGetLastError();
}

}  // namespace drx
