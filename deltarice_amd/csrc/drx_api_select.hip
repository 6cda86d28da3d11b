// drx_api_select.hip -- C ABI glue (drx_api.h): the calls that take a list of waveforms, drx_decode_select (drx_select.hip) and
// drx_gather_encoded (drx_gather.hip).  What the list asks of the batch is drx_sel_survey.h's arithmetic.  Host code only.
#include <algorithm>
#include <new>

#include "drx_api.h"
#include "drx_sel_survey.h"

using namespace drx;

// sel_survey() over the plan's geometry and, for a ragged plan, the host's chunk table.  An entry that is no waveform of the
// batch is refused here; what per_entry refuses comes back as its own value, the entry's number in *at.
template <typename F>
static int plan_survey(drx_plan *p, const char *who, const uint64_t *wave_idx, uint64_t n_sel, bool sideband,
                       std::vector<uint32_t> &lists, uint32_t n_class[3], uint64_t *at, F &&per_entry) {
    const Geom &G = p->G;
    const SelGeom S{G.uniform != 0, G.n_chunks, G.total_waves, G.u_n_samples, G.u_wave_len, G.u_n_waves};
    const int r = sel_survey(S, p->host_chunks.data(), wave_idx, n_sel, sideband, select_walk_class, lists, n_class, at, per_entry);
    if (r == kSelBadIndex)
        (void)fail(p->ctx, DRX_ERR_ARG, "%s: entry %llu is waveform %llu of %llu", who, (unsigned long long)*at,
                   (unsigned long long)wave_idx[*at], (unsigned long long)G.total_waves);
    return r;
}

// The selection's scratch: pinned staging and device copy of `bytes` each, the walk's flags.  A call that needs more replaces
// them (Buffers::reserve(); should the second allocation fail, the first stays grown, which is harmless).
static drx_status sel_scratch(drx_plan *p, size_t bytes) {
    drx_ctx *ctx = p->ctx;
    drx_plan::Selection &S = p->sel;
    if (!S.copied) DRX_HIP(ctx, hipEventCreateWithFlags(&S.copied, hipEventDisableTiming));
    DRX_HIP(ctx, p->mem.once(&S.d_fail, p->G.n_chunks * sizeof(uint32_t)));
    DRX_HIP(ctx, p->mem.reserve(S.h, bytes, 4, true, Buffers::KeepOld, ctx->stream));
    const hipError_t e = p->mem.reserve(S.d, bytes, 4, false, Buffers::KeepOld, ctx->stream);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_NOMEM, "selection scratch of %zu bytes: %s", Buffers::size(bytes, 4), hipGetErrorString(e));
    return DRX_OK;
}

// The gather's device-only scratch beside the selection's (gather_scratch_view(), drx_internal.h); grown like the selection's.
static drx_status gather_scratch(drx_plan *p, size_t bytes) {
    const hipError_t e = p->mem.reserve(p->gat.d, bytes, 4, false, Buffers::KeepOld, p->ctx->stream);
    if (e != hipSuccess) return fail(p->ctx, DRX_ERR_NOMEM, "gather scratch of %zu bytes: %s", Buffers::size(bytes, 4), hipGetErrorString(e));
    return DRX_OK;
}

// The front end of both selection calls.  The staging buffer: uint64 sel[n_sel] | uint32 chunk_n[n_out] (the gather's output
// chunks; decode_select has none) | uint32 chunk lists[touched]; sel_staged() is its device copy's view.  sel_stage() grows the
// scratch (gather_bytes != 0: the gather's too), waits until the last call's copy has left the staging buffer, fills it and sends
// it across.  sel_walk(): the walk over the chunks the selection touches, between the call's events 0 and 1.
struct SelStaged {
    const uint64_t *d_sel;
    const uint32_t *d_chunk_n, *d_lists;
};
static SelStaged sel_staged(const drx_plan *p, uint64_t n_sel, uint64_t n_out) {
    const uint32_t *d_chunk_n = (const uint32_t *)((const char *)p->sel.d.ptr + n_sel * sizeof(uint64_t));
    return SelStaged{(const uint64_t *)p->sel.d.ptr, d_chunk_n, d_chunk_n + n_out};
}
static drx_status sel_stage(drx_plan *p, const uint64_t *wave_idx, uint64_t n_sel, const std::vector<uint32_t> &chunk_n,
                            const std::vector<uint32_t> &lists, size_t gather_bytes) {
    drx_ctx *ctx = p->ctx;
    const size_t sel_bytes = n_sel * sizeof(uint64_t), cn_bytes = chunk_n.size() * sizeof(uint32_t), ls_bytes = lists.size() * sizeof(uint32_t);
    if (const drx_status st = sel_scratch(p, sel_bytes + cn_bytes + ls_bytes)) return st;
    if (gather_bytes)
        if (const drx_status st = gather_scratch(p, gather_bytes)) return st;
    char *h_sel = (char *)p->sel.h.ptr;
    DRX_HIP(ctx, hipEventSynchronize(p->sel.copied));  // (the last call's copy out of the staging buffer)
    memcpy(h_sel, wave_idx, sel_bytes);
    if (cn_bytes) memcpy(h_sel + sel_bytes, chunk_n.data(), cn_bytes);
    memcpy(h_sel + sel_bytes + cn_bytes, lists.data(), ls_bytes);
    DRX_HIP(ctx, hipMemcpyAsync(p->sel.d.ptr, h_sel, sel_bytes + cn_bytes + ls_bytes, hipMemcpyHostToDevice, ctx->stream));
    DRX_HIP(ctx, hipEventRecord(p->sel.copied, ctx->stream));
    return DRX_OK;
}
static drx_status sel_walk(drx_plan *p, const StreamCall &c, const uint32_t *d_sideband, const uint32_t *d_lists, size_t n_lists,
                           const uint32_t n_class[3]) {
    drx_ctx *ctx = p->ctx;
    mark(c.ev, 0, c.s);
    if (d_sideband)
        DRX_HIP(ctx, launch_sideband_tables(c, d_sideband, d_lists, (uint32_t)n_lists));
    else
        DRX_HIP(ctx, launch_select_walk(c, d_lists, n_class[0], n_class[1], n_class[2], p->sel.d_fail));
    mark(c.ev, 1, c.s);
    return DRX_OK;
}

// A call's host-side lists (the survey's vectors) may not fit in host memory: f() under the one handler for that
template <typename F> static drx_status list_call(drx_plan *p, const char *who, uint64_t n_sel, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) { return fail(p->ctx, DRX_ERR_NOMEM, "%s: host memory for a list of %llu entries", who, (unsigned long long)n_sel); }
}

static drx_status decode_select(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                const uint32_t *d_sideband, bool sideband, const uint64_t *wave_idx, uint64_t n_sel,
                                int16_t *d_out, uint64_t stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (n_sel == 0) return DRX_OK;
    if (!d_in || !d_chunk_word_off || !wave_idx || !d_out || (sideband && !d_sideband)) return fail(ctx, DRX_ERR_ARG, "decode_select: null pointer");
    if (sideband && d_sideband == p->d_wave_words) return fail(ctx, DRX_ERR_ARG, "the side-band table must not be the plan's own (copy it first)");
    if (n_sel >= (1ull << 32)) return fail(ctx, DRX_ERR_ARG, "decode_select: %llu entries (at most 2^32 - 1)", (unsigned long long)n_sel);
    uint32_t longest = 0;
    uint32_t n_class[3];
    uint64_t at;
    std::vector<uint32_t> lists;
    if (plan_survey(p, "decode_select", wave_idx, n_sel, sideband, lists, n_class, &at, [&](uint64_t, uint64_t, uint32_t len) {
            longest = std::max(longest, len);
            return 0;
        }))
        return DRX_ERR_ARG;
    p->gat.last.valid = false;
    if (stride < longest) return fail(ctx, DRX_ERR_ARG, "decode_select: row stride %llu below the longest selected waveform (%u)", (unsigned long long)stride, longest);
    DRX_ON_DEVICE(ctx);
    if (const drx_status st = sel_stage(p, wave_idx, n_sel, {}, lists, 0)) return st;
    const SelStaged S = sel_staged(p, n_sel, 0);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, nullptr, false, &c)) return st;
    if (const drx_status st = sel_walk(p, c, sideband ? d_sideband : nullptr, S.d_lists, lists.size(), n_class)) return st;
    DRX_HIP(ctx, launch_decode_select(c, S.d_sel, n_sel, d_out, stride));
    mark(c.ev, 2, c.s);
    mark(c.ev, 3, c.s);
    return call_end(p, DRX_PATH_SELECT);
}

// selected waveforms into a new encoded batch (drx_gather.hip)
// mean words per entry from which the copy is a wavefront per entry; below, a workgroup per run of entries
constexpr uint64_t kGatherWavesFromWords = 192;

static drx_status gather_encoded(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                 const uint32_t *d_sideband, bool sideband, const uint64_t *wave_idx, uint64_t n_sel,
                                 uint64_t cw, uint32_t *d_out, uint64_t out_cap, uint64_t *d_out_off, uint32_t *d_out_wave_words) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (cw == 0) return fail(ctx, DRX_ERR_ARG, "gather_encoded: out_chunk_waves is 0");
    if (n_sel == 0) return DRX_OK;
    if (!d_in || !d_chunk_word_off || !wave_idx || !d_out_off || (sideband && !d_sideband)) return fail(ctx, DRX_ERR_ARG, "gather_encoded: null pointer");
    if (!d_out && out_cap) return fail(ctx, DRX_ERR_ARG, "gather_encoded: no output buffer but a capacity of %llu words", (unsigned long long)out_cap);
    if (sideband && (d_sideband == p->d_wave_words || d_out_wave_words == d_sideband))
        return fail(ctx, DRX_ERR_ARG, "the side-band table must be neither the plan's own nor the output's (copy it first)");
    if (n_sel >= (1ull << 32)) return fail(ctx, DRX_ERR_ARG, "gather_encoded: %llu entries (at most 2^32 - 1)", (unsigned long long)n_sel);
    const Geom &G = p->G;
    const uint64_t n_out = (n_sel + cw - 1) / cw;
    const EncOut out{d_out, out_cap, d_out_off, d_out_wave_words};
    // the copy's form by the batch's mean code length (in_words may be a capacity: a speed matter only, like the grid's shape)
    const uint64_t mean_words = in_words / G.total_waves;
    const bool tiles = (mean_words < kGatherWavesFromWords) != ((ctx->debug_flags & DRX_DBG_GATHER_OTHER_COPY) != 0);
    // The call behind a SIZING call: the same stream, tables and list as the plan's last call, which wrote no output.  The scalar
    // key first, then the list word for word against the staged one (only then: 8 MB at 10^6 entries); the walk and the sizes are
    // not repeated.  One resume per sizing call: a call that has copied is never a source of tables.  The key is dropped HERE,
    // before sel_stage() may regrow the buffers it describes: a valid key always fits them.
    const drx_plan::Gather::Key K = p->gat.last;
    p->gat.last.valid = false;
    if (K.valid && d_out && K.d_in == d_in && K.in_words == in_words && K.d_off == d_chunk_word_off && K.d_sideband == (sideband ? d_sideband : nullptr) &&
        K.n_sel == n_sel && K.cw == cw && memcmp(p->sel.h.ptr, wave_idx, n_sel * sizeof(uint64_t)) == 0) {
        DRX_ON_DEVICE(ctx);
        StreamCall c;
        if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, nullptr, true, &c)) return st;
        const SelStaged S = sel_staged(p, n_sel, n_out);
        mark(c.ev, 0, c.s);
        mark(c.ev, 1, c.s);
        DRX_HIP(ctx, launch_gather(c, S.d_sel, n_sel, cw, S.d_chunk_n, out, gather_scratch_view(p->gat.d.ptr, n_sel), tiles, mean_words, /*resume*/ true));
        mark(c.ev, 3, c.s);
        return call_end(p, DRX_PATH_GATHER);
    }
    // the output chunks by GatherChunks' rule (drx_sel_survey.h); chunk_n[c] = output chunk c's sample count N_c
    std::vector<uint32_t> chunk_n(n_out);
    GatherChunks rule{cw, chunk_n.data()};
    uint32_t n_class[3], refused_len = 0;
    uint64_t at;
    std::vector<uint32_t> lists;
    const int refused = plan_survey(p, "gather_encoded", wave_idx, n_sel, sideband, lists, n_class, &at, [&](uint64_t i, uint64_t, uint32_t len) {
        refused_len = len;
        return (int)rule.add(i, len);
    });
    const unsigned long long entry = rule.entry, oc = rule.oc;
    switch (refused) {
    case 0: break;
    case GatherChunks::kShorterNotLast:
        return fail(ctx, DRX_ERR_ARG, "gather_encoded: entry %llu is shorter than output chunk %llu's first (%u samples) and not its last", entry, oc, rule.first);
    case GatherChunks::kLonger:
        return fail(ctx, DRX_ERR_ARG, "gather_encoded: entry %llu has %u samples, output chunk %llu's first has %u", entry, refused_len, oc, rule.first);
    case GatherChunks::kTooLong:
        return fail(ctx, DRX_ERR_ARG, "gather_encoded: output chunk %llu reaches 2^31 samples at entry %llu", oc, entry);
    default: return DRX_ERR_ARG;  // (kSelBadIndex: plan_survey() has said which entry)
    }
    DRX_ON_DEVICE(ctx);
    if (const drx_status st = sel_stage(p, wave_idx, n_sel, chunk_n, lists, gather_scratch_view(nullptr, n_sel).bytes)) return st;
    const SelStaged S = sel_staged(p, n_sel, n_out);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, nullptr, false, &c)) return st;
    if (const drx_status st = sel_walk(p, c, sideband ? d_sideband : nullptr, S.d_lists, lists.size(), n_class)) return st;
    DRX_HIP(ctx, launch_gather(c, S.d_sel, n_sel, cw, S.d_chunk_n, out, gather_scratch_view(p->gat.d.ptr, n_sel), tiles, mean_words, /*resume*/ false));
    mark(c.ev, 3, c.s);
    p->gat.last = drx_plan::Gather::Key{d_out == nullptr, d_in, sideband ? d_sideband : nullptr, d_chunk_word_off, in_words, n_sel, cw};
    return call_end(p, DRX_PATH_GATHER);
}

extern "C" {

drx_status drx_decode_select(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint64_t *wave_idx, uint64_t n_sel, int16_t *d_out, uint64_t out_stride_samples) {
    return list_call(p, "decode_select", n_sel, [&] {
        return decode_select(p, d_in, in_words, d_chunk_word_off, nullptr, false, wave_idx, n_sel, d_out, out_stride_samples);
    });
}

drx_status drx_decode_select_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                             const uint32_t *d_wave_words, const uint64_t *wave_idx, uint64_t n_sel,
                                             int16_t *d_out, uint64_t out_stride_samples) {
    return list_call(p, "decode_select", n_sel, [&] {
        return decode_select(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, wave_idx, n_sel, d_out, out_stride_samples);
    });
}

drx_status drx_gather_encoded(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const uint64_t *wave_idx, uint64_t n_sel, uint64_t out_chunk_waves, uint32_t *d_out,
                              uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return list_call(p, "gather_encoded", n_sel, [&] {
        return gather_encoded(p, d_in, in_words, d_chunk_word_off, nullptr, false, wave_idx, n_sel, out_chunk_waves, d_out, out_cap_words,
                              d_out_chunk_word_off, d_out_wave_words);
    });
}

drx_status drx_gather_encoded_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                              const uint32_t *d_wave_words, const uint64_t *wave_idx, uint64_t n_sel,
                                              uint64_t out_chunk_waves, uint32_t *d_out, uint64_t out_cap_words,
                                              uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return list_call(p, "gather_encoded", n_sel, [&] {
        return gather_encoded(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, wave_idx, n_sel, out_chunk_waves, d_out, out_cap_words,
                              d_out_chunk_word_off, d_out_wave_words);
    });
}

}  // extern "C"
