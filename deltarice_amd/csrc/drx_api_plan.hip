// drx_api_plan.hip -- C ABI (include/deltarice_hip.h) over the gfx950 kernels: contexts, plans, the prediction filter, what a plan
// reports of its last call, and the begin and end of every call (drx_api.h).
//
// The drx_api_*.hip files are host-side glue only: option parsing, batch geometry, workspace ownership, launches.  There is
// deliberately no CPU implementation of the codec in them: every entry point either runs the HIP kernels or returns an error.
//   drx_api_plan.hip    this file
//   drx_api_encode.hip  how an encode is routed, drx_encode, drx_estimate_words
//   drx_api_select.hip  drx_decode_select, drx_gather_encoded
//   drx_api_stream.hip  the calls that read an encoded batch: decode, wave_stats, wave_bins, decode_window(s), find_pulses, transcode
//   drx_api_host.hip    one chunk through host memory (the H5Z callback's body)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "drx_api.h"

using namespace drx;

drx_status drx::fail(drx_ctx *ctx, drx_status st, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->err_mu);
        ctx->last_error = buf;
    }
    return st;
}

drx_status drx::call_begin(drx_plan *p) {
    drx_ctx *ctx = p->ctx;
    p->gat.last.valid = false;
    DRX_HIP(ctx, hipMemsetAsync(p->d_status, 0, sizeof(DevStatus), ctx->stream));
    p->G.dbg = ctx->debug_flags;
    return DRX_OK;
}
drx_status drx::stream_call_begin(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                  const uint32_t *d_sideband, bool tables_ready, StreamCall *c) {
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = call_begin(p)) return st;
    // (d_pw was allocated with the plan; a plan whose filter was set to general taps afterwards simply does not take those paths)
    *c = StreamCall{&p->G, d_in, in_words, d_chunk_word_off, p->d_wave_off, p->d_wave_words, tables_ready || d_sideband, p->dec.d_pw,
                    p->d_status, ctx->profile ? p->prof.ev : nullptr, ctx->stream};
    if (d_sideband)  // header positions from the caller's n_i table, checked against the stream (k_sideband_tables)
        DRX_HIP(ctx, launch_sideband_tables(*c, d_sideband));
    return DRX_OK;
}
drx_status drx::call_end(drx_plan *p, uint32_t path, bool encode) {
    (encode ? p->enc.last_path : p->dec.last_path) = path;
    p->prof.valid = p->ctx->profile != 0;
    p->last_was_encode = encode;
    return DRX_OK;
}
drx_status drx::stream_call_args(drx_plan *p, const char *who, bool have_pointers, const uint32_t *d_sideband, bool sideband) {
    if (!have_pointers || (sideband && !d_sideband)) return fail(p->ctx, DRX_ERR_ARG, "%s: null pointer", who);
    if (sideband && d_sideband == p->d_wave_words) return fail(p->ctx, DRX_ERR_ARG, "the side-band table must not be the plan's own (copy it first)");
    return DRX_OK;
}

// n entries of a host table into the plan's device copy *view, allocated by the first upload (the same n every time);
// n = 0 leaves *view as it is (a planner's empty table: nullptr, the path is not taken)
template <typename T> static hipError_t upload(drx_plan *p, const T *host, size_t n, const T **view) {
    if (!n) return hipSuccess;
    T *d = const_cast<T *>(*view);
    const hipError_t e = p->mem.once(&d, n * sizeof(T));
    if (e != hipSuccess) return e;
    *view = d;
    return hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
}
template <typename T> static hipError_t upload(drx_plan *p, const std::vector<T> &tab, const T **view) {
    return upload(p, tab.data(), tab.size(), view);
}

void drx::plan_free(drx_plan *p) {
    if (!p) return;
    DeviceGuard guard(p->ctx->device);
    for (hipEvent_t e : p->prof.ev) if (e) (void)hipEventDestroy(e);
    if (p->sel.copied) (void)hipEventDestroy(p->sel.copied);
    delete p;  // (and its buffers)
}

// the segment encoder's bits and bit positions per unit: both or neither
hipError_t drx::seg_scratch(drx_plan *p) {
    drx_plan::Encoders &E = p->enc;
    if (E.d_seg_bits) return hipSuccess;
    const uint64_t units = long_batch_units(p->G);
    hipError_t e = p->mem.once(&E.d_seg_bits, units * sizeof(uint32_t));
    if (e == hipSuccess && (e = p->mem.once(&E.d_seg_pos, units * sizeof(uint64_t))) != hipSuccess) {
        p->mem.release(E.d_seg_bits);
        E.d_seg_bits = nullptr;
    }
    return e;
}

// Buffers of every plan
static drx_status plan_alloc(drx_plan *p) {
    drx_ctx *ctx = p->ctx;
    Geom &G = p->G;
    const uint64_t W = G.total_waves ? G.total_waves : 1;
    DRX_HIP(ctx, p->mem.alloc(&p->d_wave_words, W * sizeof(uint32_t)));
    DRX_HIP(ctx, p->mem.alloc(&p->d_wave_rel, W * sizeof(uint32_t)));
    DRX_HIP(ctx, p->mem.alloc(&p->d_wave_off, W * sizeof(uint64_t)));
    DRX_HIP(ctx, p->mem.alloc(&p->d_chunk_words, (G.n_chunks + 1) * sizeof(uint64_t)));
    // (every user clears what it reads on the stream before its launch.  k_encode_stream: size[W] | place[W] | control; its
    // segment form, where it is the default choice: size[T] | place[2 T] | control with T tickets at the shortest segments)
    uint64_t words = 2 * W + 192;
    if (stream_segs_admits(G) && G.u_wave_len >= kEsSegsFromLen) words = std::max(words, segs_scan_words(G, kEsSegMinLen));
    DRX_HIP(ctx, p->mem.reserve(p->enc.scan, words * sizeof(uint64_t), 0, false, Buffers::KeepOld, ctx->stream));
    DRX_HIP(ctx, p->mem.alloc(&p->d_status, sizeof(DevStatus)));
    DRX_HIP(ctx, hipMemset(p->d_status, 0, sizeof(DevStatus)));  // (drx_plan_finish before any launch, or behind an empty selection: no error)
    DRX_HIP(ctx, p->mem.alloc(&p->h_status, sizeof(DevStatus), true));
    memset(p->h_status, 0, sizeof(DevStatus));
    DRX_HIP(ctx, p->mem.alloc(&G.host_words, sizeof(uint64_t), true));  // (pinned host memory is device-visible at the same address)
    *G.host_words = 0;
    for (hipEvent_t &e : p->prof.ev) DRX_HIP(ctx, hipEventCreate(&e));
    return DRX_OK;
}

// Ragged plans: the chunk table, and each path's tables as its planner decided them from the host's copy
static drx_status plan_ragged(drx_plan *p, const std::vector<ChunkDesc> &desc) {
    Geom &G = p->G;
    const ChunkDesc *d = desc.data();
    const std::vector<uint32_t> walk_lists = walk_plan_ragged(G, d);
    const std::vector<uint2> order = decode_plan_ragged(G, d);
    const std::vector<uint64_t> unit_base = segments_plan_ragged(G, d);
    const std::vector<uint32_t> wg_base = pieces_plan_ragged(G, d);
    p->enc.pc_wgs = wg_base.empty() ? 0 : wg_base.back();
    // few long waveforms: the block-parallel decoder and, behind it, the in-place inverse of a general filter
    const std::vector<uint32_t> blk_list = blocks_plan_ragged(G, d);
    std::vector<uint64_t> tile_base;
    if (!blk_list.empty()) {
        tile_base.resize(G.n_chunks + 1);
        G.iir_n_tiles = iir_tiles(G, d, tile_base.data());
    }
    hipError_t e = upload(p, desc, &G.chunks);
    if (e == hipSuccess) e = upload(p, walk_lists, &G.walk_short);
    if (e == hipSuccess) e = upload(p, order, &G.rag_order);
    if (e == hipSuccess) e = upload(p, unit_base, &G.seg_unit_base);
    if (e == hipSuccess) e = upload(p, wg_base, &G.pc_wg_base);
    if (e == hipSuccess) e = upload(p, blk_list, &G.rag_blk_list);
    if (e == hipSuccess) e = upload(p, tile_base, &G.iir_chunk_tile_base);
    if (e != hipSuccess) return fail(p->ctx, DRX_ERR_DEVICE, "chunk table upload failed: %s", hipGetErrorString(e));
    G.walk_long = G.walk_short + G.n_short;
    return DRX_OK;
}

// Scratch of the paths the plan's geometry takes by default (segment and pieces encoders, parallel header walks, block decoder
// and the inverse filter behind it).  A route that a debug flag forces gets what it lacks from drx_encode (route_scratch()).
static drx_status plan_alloc_scratch(drx_plan *p) {
    drx_ctx *ctx = p->ctx;
    Geom &G = p->G;
    if (long_batch(G)) DRX_HIP(ctx, seg_scratch(p));
    if (const uint64_t nb = walk_scratch_bytes(G)) DRX_HIP(ctx, p->mem.alloc(&p->dec.d_pw, nb));
    if (const uint64_t nb = blocks_scratch_bytes(G)) {
        DRX_HIP(ctx, p->mem.alloc(&p->dec.d_blk, nb));
        // ... and, should the plan get a general prediction filter, the look-back state of the in-place inverse filter
        if (G.uniform) G.iir_n_tiles = iir_tiles(G, nullptr, nullptr);
        DRX_HIP(ctx, p->mem.alloc(&G.iir_state, (G.iir_n_tiles + 1) * sizeof(uint64_t)));
    }
    if (G.uniform && pieces_admits(G)) p->enc.pc_wgs = pieces_workgroups(G);  // (ragged: pieces_plan_ragged())
    if (p->enc.pc_wgs) DRX_HIP(ctx, p->mem.alloc(&p->enc.d_pc_scan, pieces_scan_words(G, p->enc.pc_wgs) * sizeof(uint64_t)));
    return DRX_OK;
}

// One chunk of a plan: N samples (< 2^31: int totalNumber, src/deltaRice.c:389) in waveforms of wave_len (0: the whole chunk)
static drx_status chunk_desc(drx_ctx *ctx, uint64_t c, uint32_t N, uint32_t wave_len, ChunkDesc *out) {
    if (N == 0 || N > 0x7fffffffu) return fail(ctx, DRX_ERR_ARG, "chunk %llu: bad sample count %u", (unsigned long long)c, N);
    const uint32_t L = wave_len ? wave_len : N;
    if (L > 0x7fffffffu) return fail(ctx, DRX_ERR_ARG, "chunk %llu: bad waveform length", (unsigned long long)c);
    *out = ChunkDesc{0, 0, N, L, (uint32_t)(((uint64_t)N + L - 1) / L), 0};
    return DRX_OK;
}

// The one plan builder behind drx_plan_create (per_chunk: an entry of each array per chunk) and drx_plan_create_uniform (the
// first entries hold every chunk's).  A batch whose chunks are all equal is uniform; a ragged one has the host's chunk table.
static drx_status plan_create(drx_ctx *ctx, uint64_t n_chunks, const uint32_t *chunk_samples, const uint32_t *chunk_wave_len,
                              bool per_chunk, uint32_t rice_k, drx_plan **out) {
    if (!ctx || !out || !n_chunks || !chunk_samples || !chunk_wave_len) return DRX_ERR_ARG;
    *out = nullptr;
    if (rice_k > 15) return fail(ctx, DRX_ERR_ARG, "rice_k %u out of range 0..15", rice_k);
    if (n_chunks > 0xffffffffull) return fail(ctx, DRX_ERR_ARG, "too many chunks");
    ChunkDesc first;
    if (const drx_status st = chunk_desc(ctx, 0, chunk_samples[0], chunk_wave_len[0], &first)) return st;
    std::vector<ChunkDesc> desc;
    bool uniform = true;
    if (per_chunk) {
        desc.resize(n_chunks);
        uint64_t soff = 0, wbase = 0;
        for (uint64_t c = 0; c < n_chunks; ++c) {
            if (const drx_status st = chunk_desc(ctx, c, chunk_samples[c], chunk_wave_len[c], &desc[c])) return st;
            desc[c].sample_off = soff;
            desc[c].wave_base = wbase;
            uniform = uniform && desc[c].n_samples == first.n_samples && desc[c].wave_len == first.wave_len;
            soff += desc[c].n_samples;
            wbase += desc[c].n_waves;
        }
        if (uniform) desc.clear();
    }
    DRX_ON_DEVICE(ctx);  // every allocation and table upload below lands on the context's device
    drx_plan *p = new (std::nothrow) drx_plan;
    if (!p) return DRX_ERR_NOMEM;
    p->ctx = ctx;
    Geom &G = p->G;
    G.n_chunks = n_chunks;
    G.uniform = uniform ? 1u : 0u;
    G.u_n_samples = first.n_samples;
    G.u_wave_len = first.wave_len;
    G.u_n_waves = first.n_waves;
    G.k = rice_k;
    if (uniform) {
        G.total_samples = n_chunks * first.n_samples;
        G.total_waves = n_chunks * first.n_waves;
        p->max_words = n_chunks * chunk_max_words(first.n_samples, first.n_waves);
    } else {
        G.total_samples = desc.back().sample_off + desc.back().n_samples;
        G.total_waves = desc.back().wave_base + desc.back().n_waves;
        for (const ChunkDesc &d : desc) p->max_words += chunk_max_words(d.n_samples, d.n_waves);
    }
    drx_status st = plan_alloc(p);
    if (st == DRX_OK && !uniform) st = plan_ragged(p, desc);
    if (st == DRX_OK && !uniform) p->host_chunks = std::move(desc);
    if (st == DRX_OK) st = plan_alloc_scratch(p);
    if (st != DRX_OK) { plan_free(p); return st; }
    *out = p;
    return DRX_OK;
}

extern "C" {

const char *drx_version(void) { return "deltarice-hip 0.1 (gfx950)"; }

const char *drx_status_str(drx_status s) {
    switch (s) {
        case DRX_OK: return "ok";
        case DRX_ERR_ARG: return "invalid argument or compression_opts";
        case DRX_ERR_DEVICE: return "HIP device/runtime error";
        case DRX_ERR_CAPACITY: return "output capacity too small";
        case DRX_ERR_CORRUPT: return "corrupt encoded chunk";
        case DRX_ERR_UNSUPPORTED: return "not supported on the device path";
        case DRX_ERR_NOMEM: return "out of memory";
    }
    return "unknown";
}

int drx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// cd_values -> options; the meaning of each slot is the reference's (src/deltaRice.c:248-291).
drx_status drx_parse_cd_values(size_t cd_nelmts, const unsigned *cd_values, drx_opts *out) {
    if (!out || (cd_nelmts && !cd_values)) return DRX_ERR_ARG;
    long long m = 8;
    out->wave_len = -1;
    out->n_taps = 2;
    memset(out->taps, 0, sizeof out->taps);
    out->taps[0] = 1;
    out->taps[1] = -1;
    if (cd_nelmts >= 1) m = (int)cd_values[0];
    if (cd_nelmts >= 2) out->wave_len = (int)cd_values[1];
    if (cd_nelmts >= 3) {
        const long long nt = (int)cd_values[2];
        if (nt <= 0 || nt > DRX_MAX_TAPS || (size_t)nt + 3 > cd_nelmts) return DRX_ERR_ARG;
        out->n_taps = (uint32_t)nt;
        for (long long j = 0; j < nt; ++j) out->taps[j] = (int)cd_values[3 + j];
        if (out->taps[0] == 0) return DRX_ERR_ARG;
    }
    // M must be a power of two (src/deltaRice.c:114-136); 1 <= M <= 32768 is the range in
    // which the reference itself is well defined.
    if (m <= 0 || (m & (m - 1)) != 0 || m > 32768) return DRX_ERR_ARG;
    uint32_t k = 0;
    while ((1ll << k) != m) ++k;
    out->rice_k = k;
    if (out->wave_len == 0 || out->wave_len < -1) return DRX_ERR_ARG;
    return DRX_OK;
}

drx_status drx_ctx_create(int device, void *hip_stream, drx_ctx **out) {
    if (!out) return DRX_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return DRX_ERR_DEVICE;
    drx_ctx *c = new (std::nothrow) drx_ctx;
    if (!c) return DRX_ERR_NOMEM;
    c->device = device;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) { delete c; return DRX_ERR_DEVICE; }
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return DRX_ERR_DEVICE; }
        c->own_stream = true;
    }
    // the side stream is an optimisation: a context without one runs everything on its stream
    if (hipStreamCreateWithFlags(&c->side.s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->side.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->side.join, hipEventDisableTiming) != hipSuccess) {
        if (c->side.s) (void)hipStreamDestroy(c->side.s);
        if (c->side.fork) (void)hipEventDestroy(c->side.fork);
        c->side = SideStream{nullptr, nullptr, nullptr};
        (void)hipGetLastError();
    }
    *out = c;
    return DRX_OK;
}

void drx_ctx_destroy(drx_ctx *c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->host.plan) plan_free(c->host.plan);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    if (c->side.s) (void)hipStreamDestroy(c->side.s);
    if (c->side.fork) (void)hipEventDestroy(c->side.fork);
    if (c->side.join) (void)hipEventDestroy(c->side.join);
    delete c;  // (and its buffers)
}

drx_status drx_ctx_synchronize(drx_ctx *c) {
    if (!c) return DRX_ERR_ARG;
    DRX_ON_DEVICE(c);
    DRX_HIP(c, hipStreamSynchronize(c->stream));
    return DRX_OK;
}

const char *drx_ctx_last_error(const drx_ctx *c) { return c ? c->last_error.c_str() : ""; }
void *drx_ctx_stream(const drx_ctx *c) { return c ? (void *)c->stream : nullptr; }
drx_status drx_ctx_host_staging(drx_ctx *ctx, size_t bytes, void **host_out) {
    if (!ctx || !host_out) return DRX_ERR_ARG;
    DRX_ON_DEVICE(ctx);
    const hipError_t e = ctx->mem.reserve(ctx->h_stage, bytes, 8, true, Buffers::ReleaseFirst, ctx->stream);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_NOMEM, "pinned staging buffer of %zu bytes: %s", Buffers::size(bytes, 8), hipGetErrorString(e));
    *host_out = ctx->h_stage.ptr;
    return DRX_OK;
}
int drx_ctx_device(const drx_ctx *c) { return c ? c->device : -1; }

drx_status drx_ctx_set_option(drx_ctx *c, const char *key, int64_t value) {
    if (!c || !key) return DRX_ERR_ARG;
    if (!strcmp(key, "decode_impl")) {
        if (value != 0 && value != 7 && value != 8) return DRX_ERR_ARG;
        c->decode_impl = (int)value;
        return DRX_OK;
    }
    if (!strcmp(key, "encode_impl")) {
        if (value < 0 || value > 2) return DRX_ERR_ARG;
        c->encode_impl = (int)value;
        return DRX_OK;
    }
    if (!strcmp(key, "bins_impl")) {
        if (value != 0 && value != 1) return DRX_ERR_ARG;
        c->bins_impl = (int)value;
        return DRX_OK;
    }
    if (!strcmp(key, "stack_workgroups")) {
        if (value < 0 || value > 0xffffffffll) return DRX_ERR_ARG;
        c->stack_workgroups = (uint32_t)value;
        return DRX_OK;
    }
    if (!strcmp(key, "debug_flags")) {
        c->debug_flags = (uint32_t)value;
        return DRX_OK;
    }
    if (!strcmp(key, "profile")) {
        c->profile = value != 0;
        return DRX_OK;
    }
    return DRX_ERR_ARG;
}

drx_status drx_plan_create(drx_ctx *ctx, uint64_t n_chunks, const uint32_t *chunk_samples,
                           const uint32_t *chunk_wave_len, uint32_t rice_k, drx_plan **out) {
    return plan_create(ctx, n_chunks, chunk_samples, chunk_wave_len, true, rice_k, out);
}

drx_status drx_plan_create_uniform(drx_ctx *ctx, uint64_t n_chunks, uint32_t chunk_samples,
                                   uint32_t wave_len, uint32_t rice_k, drx_plan **out) {
    return plan_create(ctx, n_chunks, &chunk_samples, &wave_len, false, rice_k, out);
}

drx_status drx_plan_set_filter(drx_plan *p, uint32_t n_taps, const int32_t *taps) {
    if (!p || !taps || n_taps == 0 || n_taps > DRX_MAX_TAPS) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (taps[0] == 0) return fail(ctx, DRX_ERR_ARG, "taps[0] must not be 0 (the inverse filter divides by it)");
    DRX_ON_DEVICE(ctx);
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Geom &G = p->G;
    p->enc.words_per_wave = 0;  // (another filter, another code length: what the last encode measured no longer applies)
    p->gat.last.valid = false;
    *G.host_words = 0;
    G.fast_taps = 0;
    G.enc_fast = 0;
    const bool delta = n_taps == 2 && taps[0] == 1 && taps[1] == -1;  // checkIfDeltaFilter, src/deltaRice.c:38-46
    if (!delta && n_taps <= 4) {
        G.enc_fast = 1;
        for (uint32_t j = 0; j < 4; ++j) G.enc_t[j] = (j < n_taps) ? (uint32_t)taps[j] & 0xffffu : 0u;
    }
    if (!delta && n_taps <= 4 && (taps[0] == 1 || taps[0] == -1)) {
        G.fast_taps = 1;
        G.fast_t0neg = taps[0] == -1;
        for (uint32_t j = 1; j < 4; ++j) G.fast_nt[j - 1] = (j < n_taps) ? 0u - (uint32_t)taps[j] : 0u;
    }
    // the device copies of the filter: kept for the plan's next filter, freed when this one has no use for them
    if (G.fast_taps && G.iir_state) {  // the block decoder's geometry: the inverse filter's matrix tables
        const uint32_t words = kIirTabWords + blocks_iir_tab_words();  // k_iir_tiles' tables, then the block decoder's own
        std::vector<uint32_t> tab(words);
        iir_tables(G.fast_nt, G.fast_t0neg, tab.data());
        blocks_iir_tables(G.fast_nt, G.fast_t0neg, tab.data() + kIirTabWords);
        DRX_HIP(ctx, upload(p, tab, &G.iir_tab));
        G.blk_iir_tab = G.iir_tab + kIirTabWords;
    } else {
        p->mem.release(G.iir_tab);
        G.iir_tab = G.blk_iir_tab = nullptr;
    }
    if (delta) {
        p->mem.release(G.taps);
        G.n_taps = 0;
        G.taps = nullptr;
        return DRX_OK;
    }
    int32_t t[DRX_MAX_TAPS] = {0};
    memcpy(t, taps, n_taps * sizeof(int32_t));
    DRX_HIP(ctx, upload(p, t, DRX_MAX_TAPS, &G.taps));
    G.n_taps = n_taps;
    return DRX_OK;
}

void drx_plan_destroy(drx_plan *p) { plan_free(p); }
uint64_t drx_plan_n_chunks(const drx_plan *p) { return p ? p->G.n_chunks : 0; }
uint64_t drx_plan_total_samples(const drx_plan *p) { return p ? p->G.total_samples : 0; }
uint64_t drx_plan_total_waves(const drx_plan *p) { return p ? p->G.total_waves : 0; }
uint64_t drx_plan_max_encoded_words(const drx_plan *p) { return p ? p->max_words : 0; }
const uint32_t *drx_plan_wave_words(const drx_plan *p) { return p ? p->d_wave_words : nullptr; }
const uint64_t *drx_plan_wave_word_off(const drx_plan *p) { return p ? p->d_wave_off : nullptr; }
uint32_t drx_plan_last_decode_path(const drx_plan *p) { return p ? p->dec.last_path : 0u; }
uint32_t drx_plan_last_encode_path(const drx_plan *p) { return p ? p->enc.last_path : 0u; }
uint32_t drx_plan_last_stats_form(const drx_plan *p) { return p ? p->stats.last_form : 0u; }
uint32_t drx_plan_last_pulses_form(const drx_plan *p) { return p ? p->pulses.last_form : 0u; }
uint32_t drx_plan_last_windows_form(const drx_plan *p) { return p ? p->windows.last_form : 0u; }
uint32_t drx_plan_last_transcode_form(const drx_plan *p) { return p ? p->trc.blocks.last_form : 0u; }
uint32_t drx_plan_last_transcode_listed(const drx_plan *p) { return (p && p->h_status && p->dec.last_path == DRX_PATH_TRANSCODE) ? p->h_status->listed : 0u; }
uint32_t drx_plan_last_pulses_redone(const drx_plan *p) { return (p && p->h_status && p->dec.last_path == DRX_PATH_PULSES) ? p->h_status->redone : 0u; }
uint32_t drx_plan_last_pulses_listed(const drx_plan *p) { return (p && p->h_status && p->dec.last_path == DRX_PATH_PULSES) ? p->h_status->listed : 0u; }
uint32_t drx_plan_last_bins_form(const drx_plan *p) { return p ? p->bins.last_form : 0u; }
uint32_t drx_plan_last_bins_listed(const drx_plan *p) { return (p && p->h_status && p->dec.last_path == DRX_PATH_BINS) ? p->h_status->listed : 0u; }
uint32_t drx_plan_last_windows_listed(const drx_plan *p) { return (p && p->h_status && p->dec.last_path == DRX_PATH_WINDOWS) ? p->h_status->listed : 0u; }

drx_status drx_plan_read_wave_words(drx_plan *p, uint32_t *host_out) {
    if (!p || !host_out) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    DRX_HIP(ctx, hipMemcpyAsync(host_out, p->d_wave_words, p->G.total_waves * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, ctx->stream));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DRX_OK;
}

drx_status drx_plan_last_timings(drx_plan *p, float ms[4]) {
    if (!p || !ms) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (!p->prof.valid) return fail(ctx, DRX_ERR_ARG, "set the context option \"profile\" before the call to be timed");
    DRX_ON_DEVICE(ctx);
    hipEvent_t *ev = p->prof.ev;
    DRX_HIP(ctx, hipEventSynchronize(ev[3]));
    for (int i = 0; i < 3; ++i) DRX_HIP(ctx, hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    DRX_HIP(ctx, hipEventElapsedTime(&ms[3], ev[0], ev[3]));
    return DRX_OK;
}

drx_status drx_plan_finish(drx_plan *p, uint64_t *total_words) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    DRX_HIP(ctx, hipMemcpyAsync(p->h_status, p->d_status, sizeof(DevStatus), hipMemcpyDeviceToHost, ctx->stream));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (total_words) *total_words = p->h_status->total_words;
    // what an encode measured decides the next encode's kernel (stream_encoder_suits())
    if (p->last_was_encode && !p->h_status->err && p->G.total_waves) p->enc.words_per_wave = p->h_status->total_words / p->G.total_waves;
    if (p->h_status->err & kErrInternal) return fail(ctx, DRX_ERR_DEVICE, "encoder look-back timed out (internal error)");
    if (p->h_status->err & kErrCorrupt) return fail(ctx, DRX_ERR_CORRUPT, "encoded input failed header-chain validation");
    if (p->h_status->err & kErrCapacity)
        return fail(ctx, DRX_ERR_CAPACITY, "encoded batch needs %llu words", (unsigned long long)p->h_status->total_words);
    return DRX_OK;
}

}  // extern "C"
