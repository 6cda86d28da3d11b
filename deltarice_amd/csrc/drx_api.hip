// drx_api.hip -- C ABI (include/deltarice_hip.h) over the gfx950 kernels.
//
// Host-side glue only: option parsing, batch geometry, workspace ownership, launches.
// There is deliberately no CPU implementation of the codec here: every entry point
// either runs the HIP kernels or returns an error.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/deltarice_hip.h"
#include "drx_internal.h"

using namespace drx;

// Device and pinned host memory of a context or a plan: every buffer of either is allocated here and freed by the destructor,
// which runs with the owner's device current (drx_ctx_destroy() and plan_free() hold a DeviceGuard).
class Buffers {
    struct Buf { void *ptr; bool pinned; };
    std::vector<Buf> bufs_;
    static void free_buf(const Buf &b) {
        if (b.pinned) (void)hipHostFree(b.ptr);
        else (void)hipFree(b.ptr);
    }

  public:
    Buffers() = default;
    Buffers(const Buffers &) = delete;
    Buffers &operator=(const Buffers &) = delete;
    ~Buffers() { for (const Buf &b : bufs_) free_buf(b); }
    template <typename T> hipError_t alloc(T **out, size_t bytes, bool pinned = false) {
        void *ptr = nullptr;
        const hipError_t e = pinned ? hipHostMalloc(&ptr, bytes, hipHostMallocDefault) : hipMalloc(&ptr, bytes);
        if (e != hipSuccess) return e;
        bufs_.push_back(Buf{ptr, pinned});
        *out = static_cast<T *>(ptr);
        return hipSuccess;
    }
    void release(const void *ptr) {  // frees one buffer now (nullptr: none)
        if (!ptr) return;
        for (size_t i = 0; i < bufs_.size(); ++i)
            if (bufs_[i].ptr == ptr) {
                free_buf(bufs_[i]);
                bufs_.erase(bufs_.begin() + i);
                return;
            }
    }
};

struct drx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    SideStream side{nullptr, nullptr, nullptr};  // independent kernels of one call (launch_decode)
    int decode_impl = 8;   // launch_decode(): 8 = walk fused into the staged kernel (default), 7 = the same with a separate
                           // walk kernel, 0 = simple kernel
    int encode_impl = 2;  // 2: single pass, persistent (k_encode_stream) where the standard geometry applies; 1: single pass with
                          // look-back (k_encode_fused) everywhere; 0: size pass + scan + pack pass
    int profile = 0;      // bracket kernels with HIP events (drx_plan_last_timings)
    uint32_t debug_flags = 0;  // Geom::dbg
    std::string last_error;
    Buffers mem;  // owns the buffers below
    // scratch of the one-chunk host path (drx_filter_chunk_host), grown on demand
    void *d_raw = nullptr;   size_t raw_cap = 0;
    void *d_enc = nullptr;   size_t enc_cap = 0;
    uint64_t *d_off = nullptr;
    void *h_pin = nullptr;   size_t pin_cap = 0;
    void *h_stage = nullptr; size_t stage_cap = 0;  // drx_ctx_host_staging(): the direct-chunk HDF5 path's staging buffer
    // the host path's plan is kept between calls: HDF5 calls the filter once per chunk with the same
    // geometry, and creating a plan costs its allocations and frees (about a millisecond)
    drx_plan *host_plan = nullptr;
    uint32_t hp_samples = 0, hp_L = 0, hp_k = 0, hp_ntaps = 0;
    int32_t hp_taps[DRX_MAX_TAPS] = {0};
    std::mutex mu;      // serialises drx_filter_chunk_host callers (HDF5 may call the filter from any thread)
    std::mutex err_mu;  // last_error
};

// Every entry point runs on the context's device and leaves the calling thread's current device as it found it
// (an application that works on another GPU must not find its device switched by an H5Dread).
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = (prev == device) ? hipSuccess : hipSetDevice(device);
        if (prev == device) prev = -1;  // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define DRX_ON_DEVICE(ctx)                                                                         \
    DeviceGuard dev_guard_((ctx)->device);                                                         \
    if (dev_guard_.err != hipSuccess)                                                              \
        return fail((ctx), DRX_ERR_DEVICE, "hipSetDevice(%d) failed: %s", (ctx)->device, hipGetErrorString(dev_guard_.err))

struct drx_plan {
    drx_ctx *ctx = nullptr;
    Geom G{};      // its device tables (chunks, walk lists, taps, ...) and pinned host_words are buffers of mem, held nowhere else
    Buffers mem;   // owns every buffer of the plan
    uint64_t max_words = 0;
    uint32_t *d_wave_words = nullptr;  // n_i
    uint32_t *d_wave_rel = nullptr;    // encode: header position relative to chunk start
    uint64_t *d_wave_off = nullptr;    // decode: absolute header position
    uint64_t *d_chunk_words = nullptr;
    uint64_t *d_scan = nullptr;        // look-back state of the single-pass encoders + ticket; the decoder's granules
    size_t scan_bytes = 0;             // ... its size
    uint32_t last_enc_path = 0;         // DRX_ENC_* of the last drx_encode
    uint64_t enc_words_per_wave = 0;   // of the plan's last encode (0: none yet)
    uint32_t *d_seg_bits = nullptr;    // segment encoder: bits and bit position of every segment (both or neither:
    uint64_t *d_seg_pos = nullptr;     // seg_scratch())
    uint64_t *d_pc_scan = nullptr;        // pieces encoder: look-back entry per workgroup + ticket
    uint64_t pc_wgs = 0;                  // its workgroups (0: the plan's geometry never takes it)
    void *d_pw = nullptr;              // a handful of chunks: candidate lists of the parallel header walk
    void *d_blk = nullptr;             // few waveforms: unit table, look-back state and flags of the block-parallel decoder
    void *d_sacc = nullptr;            // ... and drx_wave_stats' block form: accumulators and list, allocated by its first call
    uint32_t last_stats_form = 0;      // DRX_STATS_FORM_* of the last drx_wave_stats (0: none yet)
    void *d_ptab = nullptr;            // ... and drx_find_pulses' block form: block summaries and list, allocated by its first call
    void *d_pstage = nullptr;          // ... and the records its blocks stage, grown when a call needs more (pulses_staging())
    size_t pstage_cap = 0;
    uint32_t last_pulses_form = 0;     // DRX_PULSES_FORM_* of the last drx_find_pulses (0: none yet)
    void *d_wtab = nullptr;            // ... and drx_decode_windows' block form: its list, allocated by its first call
    uint32_t last_windows_form = 0;    // DRX_WINDOWS_FORM_* of the last drx_decode_windows (0: none yet)
    DevStatus *d_status = nullptr;
    DevStatus *h_status = nullptr;  // pinned
    bool last_was_encode = false;
    uint32_t last_path = 0;  // DRX_PATH_* of the last decode
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    // drx_decode_select: the host's chunk table (ragged plans; host memory), and the selection's scratch -- allocated by the
    // first select call, grown when a later one needs more (sel_scratch())
    std::vector<ChunkDesc> host_chunks;
    void *h_sel = nullptr, *d_sel = nullptr;  // uint64 sel[n_sel] | uint32 chunk lists[touched]: pinned staging and its device copy
    size_t sel_cap = 0;                       // ... bytes of each
    uint32_t *d_sel_fail = nullptr;           // uint32[n_chunks]: chunks the chunk-wide walk handed to the scalar walker
    hipEvent_t sel_copied = nullptr;          // the staging buffer has crossed to the device (the next call may fill it again)
    // drx_transcode / drx_estimate_words_encoded: uint64 chunk_words[n_chunks + 1] | uint64 est[16] | uint32 n_i'[W] | uint32
    // header positions[W] of the RESULT (the plan's own tables describe the source); allocated by the first such call
    void *d_trc = nullptr;
    void *d_gat = nullptr;                    // drx_gather_encoded: positions, sizes and scan state (gather_scratch())
    size_t gat_cap = 0;
    // ... and what the plan's last call was asked IF that call was a gather's SIZING call (d_out == NULL: it wrote no output): its
    // list is still in h_sel / d_sel, its tables (the walk's, sizes, scanned block sums, total and verdict) in d_wave_* / d_gat.
    // The gather with the same arguments right behind it resumes from them, once.  `valid` is cleared by every other call on the
    // plan that launches or writes one of those buffers, by a gather that regrows h_sel / d_gat (so a valid key always fits the
    // buffers it describes), and by the resumed call itself: no call that copied anything is ever resumed from
    struct GatherKey {
        bool valid = false;
        const uint32_t *d_in = nullptr, *d_sideband = nullptr;
        const uint64_t *d_off = nullptr;
        uint64_t in_words = 0, n_sel = 0, cw = 0;
    } gat_last;
};

static drx_status fail(drx_ctx *ctx, drx_status st, const char *fmt, ...) {
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

#define DRX_HIP(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((ctx), DRX_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// n entries of a host table into the plan's device copy *view, allocated by the first upload (the same n every time);
// n = 0 leaves *view as it is (a planner's empty table: nullptr, the path is not taken)
template <typename T> static hipError_t upload(drx_plan *p, const T *host, size_t n, const T **view) {
    if (!n) return hipSuccess;
    T *d = const_cast<T *>(*view);
    if (!d) {
        const hipError_t e = p->mem.alloc(&d, n * sizeof(T));
        if (e != hipSuccess) return e;
        *view = d;
    }
    return hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
}
template <typename T> static hipError_t upload(drx_plan *p, const std::vector<T> &tab, const T **view) {
    return upload(p, tab.data(), tab.size(), view);
}

// What a selection asks of the plan: every entry's chunk and length (arithmetic for a uniform plan, a bisection of the host's
// chunk table for a ragged one) handed to per_entry(i, chunk, len), which may refuse the list; and the sorted set of chunks the
// selection touches as the walk takes them -- three lists, each sorted (select_walk_class()); the side-band takes them as one.
template <typename F>
static drx_status sel_survey(drx_plan *p, const char *who, const uint64_t *wave_idx, uint64_t n_sel, bool sideband,
                             std::vector<uint32_t> &lists, uint32_t n_class[3], F &&per_entry) {
    drx_ctx *ctx = p->ctx;
    const Geom &G = p->G;
    const bool small = G.total_waves <= 0xffffffffull;
    auto chunk_of = [&](uint64_t g, uint32_t *len) -> uint64_t {
        uint64_t c, idx;
        uint32_t W, L, N;
        if (G.uniform) {
            c = small ? (uint32_t)g / G.u_n_waves : g / G.u_n_waves;  // (a million entries: the 32-bit division is a third of the loop)
            idx = g - c * G.u_n_waves;
            W = G.u_n_waves; L = G.u_wave_len; N = G.u_n_samples;
        } else {
            uint64_t lo = 0, hi = G.n_chunks;  // invariant: wave_base[lo] <= g < wave_base[hi]
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (p->host_chunks[mid].wave_base <= g) lo = mid; else hi = mid;
            }
            const ChunkDesc &d = p->host_chunks[c = lo];
            idx = g - d.wave_base; W = d.n_waves; L = d.wave_len; N = d.n_samples;
        }
        *len = idx + 1 == W ? N - (uint32_t)idx * L : L;
        return c;
    };
    // a flag per chunk for large selections, sort + unique for small ones
    std::vector<uint32_t> touched;
    std::vector<uint8_t> flag;
    const bool by_flag = n_sel > G.n_chunks / 8u;
    if (by_flag) flag.assign(G.n_chunks, 0);
    else touched.reserve(n_sel);
    for (uint64_t i = 0; i < n_sel; ++i) {
        if (wave_idx[i] >= G.total_waves)
            return fail(ctx, DRX_ERR_ARG, "%s: entry %llu is waveform %llu of %llu", who, (unsigned long long)i,
                        (unsigned long long)wave_idx[i], (unsigned long long)G.total_waves);
        uint32_t len;
        const uint64_t c = chunk_of(wave_idx[i], &len);
        if (const drx_status st = per_entry(i, c, len)) return st;
        if (by_flag) flag[c] = 1;
        else touched.push_back((uint32_t)c);
    }
    if (by_flag) {
        for (uint64_t c = 0; c < G.n_chunks; ++c) if (flag[c]) touched.push_back((uint32_t)c);
    } else {
        std::sort(touched.begin(), touched.end());
        touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    }
    n_class[0] = n_class[1] = n_class[2] = 0;
    lists.assign(touched.size(), 0);
    if (sideband) {
        lists = touched;
    } else {
        auto cls = [&](uint32_t c) { return G.uniform ? select_walk_class(G.u_n_waves, G.u_wave_len)
                                                      : select_walk_class(p->host_chunks[c].n_waves, p->host_chunks[c].wave_len); };
        for (uint32_t c : touched) ++n_class[cls(c)];
        uint32_t at[3] = {0, n_class[0], n_class[0] + n_class[1]};
        for (uint32_t c : touched) lists[at[cls(c)]++] = c;
    }
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

static void plan_free(drx_plan *p);

void drx_ctx_destroy(drx_ctx *c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->host_plan) plan_free(c->host_plan);
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
    if (ctx->stage_cap < bytes) {
        if (ctx->h_stage) { (void)hipStreamSynchronize(ctx->stream); ctx->mem.release(ctx->h_stage); ctx->h_stage = nullptr; ctx->stage_cap = 0; }
        const size_t want = bytes + bytes / 8 + 4096;
        const hipError_t e = ctx->mem.alloc(&ctx->h_stage, want, true);
        if (e != hipSuccess) return fail(ctx, DRX_ERR_NOMEM, "pinned staging buffer of %zu bytes: %s", want, hipGetErrorString(e));
        ctx->stage_cap = want;
    }
    *host_out = ctx->h_stage;
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

// the context's host-path buffers: a call that needs more replaces the buffer (freeing the old one first: every call grows
// them again before use)
static drx_status grow(drx_ctx *ctx, void **ptr, size_t *cap, size_t need, bool pinned) {
    if (*cap >= need) return DRX_OK;
    size_t want = need + need / 4 + 4096;
    ctx->mem.release(*ptr);
    *ptr = nullptr;
    *cap = 0;
    hipError_t e = ctx->mem.alloc(ptr, want, pinned);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_DEVICE, "allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
    *cap = want;
    return DRX_OK;
}

static void plan_free(drx_plan *p) {
    if (!p) return;
    DeviceGuard guard(p->ctx->device);
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    if (p->sel_copied) (void)hipEventDestroy(p->sel_copied);
    delete p;  // (and its buffers)
}

// the segment encoder's bits and bit positions per unit: both or neither
static hipError_t seg_scratch(drx_plan *p) {
    const uint64_t units = long_batch_units(p->G);
    uint32_t *bits = nullptr;
    uint64_t *pos = nullptr;
    hipError_t e = p->mem.alloc(&bits, units * sizeof(uint32_t));
    if (e == hipSuccess && (e = p->mem.alloc(&pos, units * sizeof(uint64_t))) != hipSuccess) p->mem.release(bits);
    if (e != hipSuccess) return e;
    p->d_seg_bits = bits;
    p->d_seg_pos = pos;
    return hipSuccess;
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
    DRX_HIP(ctx, p->mem.alloc(&p->d_scan, p->scan_bytes = words * sizeof(uint64_t)));
    DRX_HIP(ctx, p->mem.alloc(&p->d_status, sizeof(DevStatus)));
    DRX_HIP(ctx, hipMemset(p->d_status, 0, sizeof(DevStatus)));  // (drx_plan_finish before any launch, or behind an empty selection: no error)
    DRX_HIP(ctx, p->mem.alloc(&p->h_status, sizeof(DevStatus), true));
    memset(p->h_status, 0, sizeof(DevStatus));
    DRX_HIP(ctx, p->mem.alloc(&G.host_words, sizeof(uint64_t), true));  // (pinned host memory is device-visible at the same address)
    *G.host_words = 0;
    for (hipEvent_t &e : p->ev) DRX_HIP(ctx, hipEventCreate(&e));
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
    p->pc_wgs = wg_base.empty() ? 0 : wg_base.back();
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
    if (const uint64_t nb = walk_scratch_bytes(G)) DRX_HIP(ctx, p->mem.alloc(&p->d_pw, nb));
    if (const uint64_t nb = blocks_scratch_bytes(G)) {
        DRX_HIP(ctx, p->mem.alloc(&p->d_blk, nb));
        // ... and, should the plan get a general prediction filter, the look-back state of the in-place inverse filter
        if (G.uniform) G.iir_n_tiles = iir_tiles(G, nullptr, nullptr);
        DRX_HIP(ctx, p->mem.alloc(&G.iir_state, (G.iir_n_tiles + 1) * sizeof(uint64_t)));
    }
    if (G.uniform && pieces_admits(G)) p->pc_wgs = pieces_workgroups(G);  // (ragged: pieces_plan_ragged())
    if (p->pc_wgs) DRX_HIP(ctx, p->mem.alloc(&p->d_pc_scan, pieces_scan_words(G, p->pc_wgs) * sizeof(uint64_t)));
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
    p->enc_words_per_wave = 0;  // (another filter, another code length: what the last encode measured no longer applies)
    p->gat_last.valid = false;
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
uint32_t drx_plan_last_decode_path(const drx_plan *p) { return p ? p->last_path : 0u; }
uint32_t drx_plan_last_encode_path(const drx_plan *p) { return p ? p->last_enc_path : 0u; }
uint32_t drx_plan_last_stats_form(const drx_plan *p) { return p ? p->last_stats_form : 0u; }
uint32_t drx_plan_last_pulses_form(const drx_plan *p) { return p ? p->last_pulses_form : 0u; }
uint32_t drx_plan_last_windows_form(const drx_plan *p) { return p ? p->last_windows_form : 0u; }
uint32_t drx_plan_last_pulses_redone(const drx_plan *p) { return (p && p->h_status && p->last_path == DRX_PATH_PULSES) ? p->h_status->redone : 0u; }
uint32_t drx_plan_last_pulses_listed(const drx_plan *p) { return (p && p->h_status && p->last_path == DRX_PATH_PULSES) ? p->h_status->listed : 0u; }
uint32_t drx_plan_last_windows_listed(const drx_plan *p) { return (p && p->h_status && p->last_path == DRX_PATH_WINDOWS) ? p->h_status->listed : 0u; }

drx_status drx_plan_read_wave_words(drx_plan *p, uint32_t *host_out) {
    if (!p || !host_out) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    DRX_HIP(ctx, hipMemcpyAsync(host_out, p->d_wave_words, p->G.total_waves * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, ctx->stream));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DRX_OK;
}

// k_encode_stream or k_encode_fused?  The persistent form wins where a wavefront's ring (kEsRingWords) holds a waveform's
// code AND most of the next one's (the next is coded while the first waits for its place), and where the batch feeds its
// 4096 wavefronts a few waveforms each -- measured (profiles/r04_notes.md section 1e), stream / fused: 100 chunks of 14 M
// samples at WaveformLength 3600 ... 8192 (1060-1660 words per waveform) 1.02-1.70 / 1.09-1.97 ms, at 10000 (2020 words: the
// next waveform cannot start) 1.72 / 1.25; AR(1) under m = 4 (1740 words, 11 % escapes) 6.44 / 5.70; one chunk of 2000
// waveforms 0.031 / 0.023, ten chunks 0.126 / 0.137.  A waveform's words are not known before it is coded: the plan's last
// encode says (the same data shape comes again), and before that k + 3.5 bits per sample (the RiceParameter that suits).
static bool stream_encoder_suits(const drx_plan *p, int wide) {
    const Geom &G = p->G;
    if (wide != 0 || G.total_waves < kEsMinUnits) return false;
    const uint64_t L = G.uniform ? G.u_wave_len : G.max_wave_len64 / 64u;
    const uint64_t words = p->enc_words_per_wave ? p->enc_words_per_wave : (L * (2u * G.k + 7u)) / 64u;
    return words <= (uint64_t)kEsRingWords * 67u / 100u;
}

// k_encode_stream_segs or k_encode_pieces?  Long waveforms in a batch that feeds the persistent grid's 4096 wavefronts a few
// segments each; returns the segment length to aim at (0: not this encoder) -- what leaves a ring room for most of the next
// segment (57 % of it, as a 7000-sample waveform of the headline does), from the bits per sample of the plan's last encode or,
// before that, k + 3.5.
static uint32_t stream_segs_target(const drx_plan *p) {
    const Geom &G = p->G;
    const uint64_t L = G.u_wave_len;
    if (L < kEsSegsFromLen) return 0u;
    const uint64_t bps16 = p->enc_words_per_wave ? (p->enc_words_per_wave * 512u) / L : 16u * G.k + 56u;  // bits per sample x 16
    uint64_t t = ((uint64_t)kEsRingWords * 32u * 57u / 100u) * 16u / (bps16 ? bps16 : 1u);
    t = t > kEsSegMaxLen ? kEsSegMaxLen : (t < kEsSegMinLen ? kEsSegMinLen : t);
    const EsSegShape sh = es_seg_shape((uint32_t)L, (uint32_t)t);
    if (G.total_waves * sh.nseg < kEsMinUnits) return 0u;
    return (uint32_t)t;
}

// ---------------------------------------------------------------------------
// How an encode call is routed: ONE table, first matching row wins (route_encode()).  An encoder admits the batches it can run
// (geometry, filter, encode_impl); its default row takes those it is the best choice for.
//   encoder     | admits                                               | default choice
//   ------------+------------------------------------------------------+-------------------------------------------------------
//   STREAM_SEGS | impl 2, stream_segs_admits()                         | L >= kEsSegsFromLen, kEsMinUnits segments (stream_segs_target())
//   PIECES      | impl >= 1, pieces_admits()                           | pieces_batch(): runs of short / segments of long waveforms
//   SEGMENTS    | impl >= 1, long_batch_admits()                       | long_batch(): short, long or few long waveforms
//   STREAM      | impl 2, delta or fast filter, tickets fit 32 bits    | stream_encoder_suits(): >= kEsMinUnits waveforms, code fits a ring
//   FUSED       | impl >= 1, delta or fast filter, <= kMaxWavefrontWaves | always (fused_wide(): larger buffers for m above 8)
//   TWO_PASS    | always (launched in slices)                          | always
// A launch carries fewer than 2^32 threads: the encoders that give every waveform (segment slot) a wavefront of ONE launch admit
// batches of at most kMaxWavefrontWaves of them, k_encode_pieces fewer than 2^23 workgroups (include/deltarice_hip.h).
// Forced rows come first, in this order: DRX_DBG_FORCE_STREAM_SEGS (segments of kEsSegMinLen samples), FORCE_SEGMENTS,
// FORCE_PIECES, FORCE_STREAM take their encoder wherever it admits the batch.  Exclusions: NO_PIECES drops the default
// PIECES and STREAM_SEGS rows, NO_LONG_PATHS the default SEGMENTS and STREAM_SEGS rows; NO_WIDE_FUSED sets fused_wide to 0.
// ---------------------------------------------------------------------------
struct EncodeRoute { uint32_t enc, seg_target; int wide; };  // DRX_ENC_*, STREAM_SEGS: segment length to aim at, FUSED: fused_wide()

static EncodeRoute route_encode(const drx_plan *p, int impl, uint32_t dbg) {
    const Geom &G = p->G;
    const int wide = (dbg & DRX_DBG_NO_WIDE_FUSED) ? 0 : fused_wide(G);
    const bool fast = G.n_taps == 0 || G.enc_fast, single = impl >= 1;
    const bool segs_in = impl == 2 && stream_segs_admits(G), pieces_in = single && pieces_admits(G);
    const bool long_in = single && long_batch_admits(G), stream_in = impl == 2 && fast && G.total_waves < 0xffff0000ull;
    const bool fused_in = single && fast && G.total_waves <= kMaxWavefrontWaves;
    if ((dbg & DRX_DBG_FORCE_STREAM_SEGS) && segs_in) return {DRX_ENC_STREAM_SEGS, kEsSegMinLen, wide};
    if ((dbg & DRX_DBG_FORCE_SEGMENTS) && long_in) return {DRX_ENC_SEGMENTS, 0, wide};
    if ((dbg & DRX_DBG_FORCE_PIECES) && pieces_in) return {DRX_ENC_PIECES, 0, wide};
    if ((dbg & DRX_DBG_FORCE_STREAM) && stream_in) return {DRX_ENC_STREAM, 0, wide};
    if (segs_in && !(dbg & (DRX_DBG_NO_PIECES | DRX_DBG_NO_LONG_PATHS)))
        if (const uint32_t t = stream_segs_target(p)) return {DRX_ENC_STREAM_SEGS, t, wide};
    if (pieces_in && !(dbg & DRX_DBG_NO_PIECES) && pieces_batch(G, wide)) return {DRX_ENC_PIECES, 0, wide};
    if (long_in && !(dbg & DRX_DBG_NO_LONG_PATHS) && long_batch(G)) return {DRX_ENC_SEGMENTS, 0, wide};
    if (stream_in && stream_encoder_suits(p, wide)) return {DRX_ENC_STREAM, 0, wide};
    return {fused_in ? DRX_ENC_FUSED : DRX_ENC_TWO_PASS, 0, wide};
}

// Scratch of a route beyond what the plan was sized for, which only a route that a debug flag forces needs: the segment
// form's look-back state for shorter segments, the segment encoder's where its default row would not take the batch
static drx_status route_scratch(drx_plan *p, const EncodeRoute &R) {
    drx_ctx *ctx = p->ctx;
    if (R.enc == DRX_ENC_STREAM_SEGS) {
        const size_t need = segs_scan_words(p->G, R.seg_target) * sizeof(uint64_t);
        if (p->scan_bytes < need) {
            // the larger buffer first: should that fail, the plan keeps the one its default routes were sized for
            const size_t want = need + need / 4 + 4096;
            uint64_t *scan = nullptr;
            DRX_HIP(ctx, p->mem.alloc(&scan, want));
            p->mem.release(p->d_scan);  // (waits for the device)
            p->d_scan = scan;
            p->scan_bytes = want;
        }
    }
    if (R.enc == DRX_ENC_SEGMENTS && !p->d_seg_bits) DRX_HIP(ctx, seg_scratch(p));
    return DRX_OK;
}

// ---------------------------------------------------------------------------
// Every call that launches opens with call_begin(), on the context's device: the resume key dropped (a no-op for the selection
// calls, which drop it earlier -- before the early returns their argument checks leave them), the plan's status word cleared on
// the stream, the debug flags copied.  The frame a call hands its launchers (drx_internal.h) is built from the plan behind it:
// stream_call_begin() for the calls on an encoded batch, whose side-band form (d_sideband: the WHOLE batch's table) gets its
// header tables here.  call_end(): what the plan remembers of its last call.
// ---------------------------------------------------------------------------
static drx_status call_begin(drx_plan *p) {
    drx_ctx *ctx = p->ctx;
    p->gat_last.valid = false;
    DRX_HIP(ctx, hipMemsetAsync(p->d_status, 0, sizeof(DevStatus), ctx->stream));
    p->G.dbg = ctx->debug_flags;
    return DRX_OK;
}
static drx_status stream_call_begin(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                    const uint32_t *d_sideband, bool tables_ready, StreamCall *c) {
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = call_begin(p)) return st;
    // (d_pw was allocated with the plan; a plan whose filter was set to general taps afterwards simply does not take those paths)
    *c = StreamCall{&p->G, d_in, in_words, d_chunk_word_off, p->d_wave_off, p->d_wave_words, tables_ready || d_sideband, p->d_pw,
                    p->d_status, ctx->profile ? p->ev : nullptr, ctx->stream};
    if (d_sideband)  // header positions from the caller's n_i table, checked against the stream (k_sideband_tables)
        DRX_HIP(ctx, launch_sideband_tables(*c, d_sideband));
    return DRX_OK;
}
static drx_status call_end(drx_plan *p, uint32_t path, bool encode = false) {
    (encode ? p->last_enc_path : p->last_path) = path;
    p->ev_valid = p->ctx->profile != 0;
    p->last_was_encode = encode;
    return DRX_OK;
}

drx_status drx_encode(drx_plan *p, const int16_t *d_in, uint32_t *d_out, uint64_t out_cap_words,
                      uint64_t *d_chunk_word_off) {
    if (!p || !d_in || !d_out || !d_chunk_word_off) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    if (const drx_status st = call_begin(p)) return st;
    // what the plan's last encode measured decides this one's kernel -- read from the word the encoders write to pinned host
    // memory, so that callers that never wait for an encode (bench.py's steps) are covered without a copy or an event
    if (const uint64_t w = *(volatile uint64_t *)p->G.host_words) p->enc_words_per_wave = p->G.total_waves ? w / p->G.total_waves : 0;
    const EncodeRoute R = route_encode(p, ctx->encode_impl, ctx->debug_flags);
    if (const drx_status st = route_scratch(p, R)) return st;
    const EncodeCall c{&p->G, d_in, EncOut{d_out, out_cap_words, d_chunk_word_off, p->d_wave_words}, p->d_status,
                       ctx->profile ? p->ev : nullptr, ctx->stream};
    switch (R.enc) {
    case DRX_ENC_STREAM_SEGS: DRX_HIP(ctx, launch_encode_stream_segs(c, R.seg_target, p->d_scan)); break;
    case DRX_ENC_PIECES: DRX_HIP(ctx, launch_encode_pieces(c, p->G.total_samples, p->d_pc_scan, p->pc_wgs)); break;
    case DRX_ENC_SEGMENTS: DRX_HIP(ctx, launch_encode_long(c, p->d_wave_rel, p->d_chunk_words, p->d_seg_bits, p->d_seg_pos)); break;
    case DRX_ENC_STREAM: DRX_HIP(ctx, launch_encode_stream(c, p->d_scan)); break;
    case DRX_ENC_FUSED: DRX_HIP(ctx, launch_encode_fused(c, R.wide, p->d_scan)); break;
    default: DRX_HIP(ctx, launch_encode(c, p->d_wave_rel, p->d_chunk_words));
    }
    return call_end(p, R.enc, /*encode*/ true);
}

static drx_status decode_launch(drx_plan *p, const uint32_t *d_in, uint64_t in_words,
                                const uint64_t *d_chunk_word_off, int16_t *d_out, bool tables_ready,
                                const uint32_t *d_sideband = nullptr) {
    if (!p || !d_in || !d_chunk_word_off || !d_out) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    // (in_words says nothing about how long a waveform's code is -- it may be, and in bench.py IS, the buffer's capacity; round 4
    // took it for the stream's length for a while and sent the headline batch to k_encode_fused)
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, tables_ready, &c)) return st;
    // (d_blk was allocated with the plan, like d_pw)
    DRX_HIP(ctx, launch_decode(c, d_out, p->d_scan, ctx->decode_impl, p->d_blk, ctx->side.s ? &ctx->side : nullptr, &p->last_path));
    return call_end(p, p->last_path);
}

drx_status drx_decode(drx_plan *p, const uint32_t *d_in, uint64_t in_words,
                      const uint64_t *d_chunk_word_off, int16_t *d_out) {
    return decode_launch(p, d_in, in_words, d_chunk_word_off, d_out, false);
}

drx_status drx_decode_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                      const uint32_t *d_wave_words, int16_t *d_out) {
    if (!d_wave_words) return DRX_ERR_ARG;
    if (p && d_wave_words == p->d_wave_words) return fail(p->ctx, DRX_ERR_ARG, "the side-band table must not be the plan's own (copy it first)");
    return decode_launch(p, d_in, in_words, d_chunk_word_off, d_out, false, d_wave_words);
}

// ---------------------------------------------------------------------------
// selected waveforms (drx_select.hip)
// ---------------------------------------------------------------------------
// The selection's scratch: pinned staging and device copy of `bytes` each, the walk's flags.  A call that needs more
// replaces the pair (the larger ones first: should that fail, the plan keeps what it had).
static drx_status sel_scratch(drx_plan *p, size_t bytes) {
    drx_ctx *ctx = p->ctx;
    if (!p->sel_copied) DRX_HIP(ctx, hipEventCreateWithFlags(&p->sel_copied, hipEventDisableTiming));
    if (!p->d_sel_fail) DRX_HIP(ctx, p->mem.alloc(&p->d_sel_fail, p->G.n_chunks * sizeof(uint32_t)));
    if (p->sel_cap >= bytes) return DRX_OK;
    const size_t want = bytes + bytes / 4 + 4096;
    void *h = nullptr, *d = nullptr;
    DRX_HIP(ctx, p->mem.alloc(&h, want, true));
    const hipError_t e = p->mem.alloc(&d, want);
    if (e != hipSuccess) {
        p->mem.release(h);
        return fail(ctx, DRX_ERR_NOMEM, "selection scratch of %zu bytes: %s", want, hipGetErrorString(e));
    }
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier select call may still read the old pair)
    p->mem.release(p->h_sel);
    p->mem.release(p->d_sel);
    p->h_sel = h;
    p->d_sel = d;
    p->sel_cap = want;
    return DRX_OK;
}

// The gather's device-only scratch beside the selection's (gather_scratch_view(), drx_internal.h); grown like the selection's.
static drx_status gather_scratch(drx_plan *p, size_t bytes) {
    drx_ctx *ctx = p->ctx;
    if (p->gat_cap >= bytes) return DRX_OK;
    const size_t want = bytes + bytes / 4 + 4096;
    void *d = nullptr;
    const hipError_t e = p->mem.alloc(&d, want);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_NOMEM, "gather scratch of %zu bytes: %s", want, hipGetErrorString(e));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier gather may still use the old one)
    p->mem.release(p->d_gat);
    p->d_gat = d;
    p->gat_cap = want;
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
    const uint32_t *d_chunk_n = (const uint32_t *)((const char *)p->d_sel + n_sel * sizeof(uint64_t));
    return SelStaged{(const uint64_t *)p->d_sel, d_chunk_n, d_chunk_n + n_out};
}
static drx_status sel_stage(drx_plan *p, const uint64_t *wave_idx, uint64_t n_sel, const std::vector<uint32_t> &chunk_n,
                            const std::vector<uint32_t> &lists, size_t gather_bytes) {
    drx_ctx *ctx = p->ctx;
    const size_t sel_bytes = n_sel * sizeof(uint64_t), cn_bytes = chunk_n.size() * sizeof(uint32_t), ls_bytes = lists.size() * sizeof(uint32_t);
    if (const drx_status st = sel_scratch(p, sel_bytes + cn_bytes + ls_bytes)) return st;
    if (gather_bytes)
        if (const drx_status st = gather_scratch(p, gather_bytes)) return st;
    DRX_HIP(ctx, hipEventSynchronize(p->sel_copied));  // (the last call's copy out of the staging buffer)
    memcpy(p->h_sel, wave_idx, sel_bytes);
    if (cn_bytes) memcpy((char *)p->h_sel + sel_bytes, chunk_n.data(), cn_bytes);
    memcpy((char *)p->h_sel + sel_bytes + cn_bytes, lists.data(), ls_bytes);
    DRX_HIP(ctx, hipMemcpyAsync(p->d_sel, p->h_sel, sel_bytes + cn_bytes + ls_bytes, hipMemcpyHostToDevice, ctx->stream));
    DRX_HIP(ctx, hipEventRecord(p->sel_copied, ctx->stream));
    return DRX_OK;
}
static drx_status sel_walk(drx_plan *p, const StreamCall &c, const uint32_t *d_sideband, const uint32_t *d_lists, size_t n_lists,
                           const uint32_t n_class[3]) {
    drx_ctx *ctx = p->ctx;
    mark(c.ev, 0, c.s);
    if (d_sideband)
        DRX_HIP(ctx, launch_sideband_tables(c, d_sideband, d_lists, (uint32_t)n_lists));
    else
        DRX_HIP(ctx, launch_select_walk(c, d_lists, n_class[0], n_class[1], n_class[2], p->d_sel_fail));
    mark(c.ev, 1, c.s);
    return DRX_OK;
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
    std::vector<uint32_t> lists;
    if (const drx_status st = sel_survey(p, "decode_select", wave_idx, n_sel, sideband, lists, n_class, [&](uint64_t, uint64_t, uint32_t len) {
            longest = std::max(longest, len);
            return DRX_OK;
        }))
        return st;
    p->gat_last.valid = false;
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

drx_status drx_decode_select(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint64_t *wave_idx, uint64_t n_sel, int16_t *d_out, uint64_t out_stride_samples) {
    try {
        return decode_select(p, d_in, in_words, d_chunk_word_off, nullptr, false, wave_idx, n_sel, d_out, out_stride_samples);
    } catch (const std::bad_alloc &) { return fail(p->ctx, DRX_ERR_NOMEM, "decode_select: host memory for a list of %llu entries", (unsigned long long)n_sel); }
}

drx_status drx_decode_select_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                             const uint32_t *d_wave_words, const uint64_t *wave_idx, uint64_t n_sel,
                                             int16_t *d_out, uint64_t out_stride_samples) {
    try {
        return decode_select(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, wave_idx, n_sel, d_out, out_stride_samples);
    } catch (const std::bad_alloc &) { return fail(p->ctx, DRX_ERR_NOMEM, "decode_select: host memory for a list of %llu entries", (unsigned long long)n_sel); }
}

// ---------------------------------------------------------------------------
// selected waveforms into a new encoded batch (drx_gather.hip)
// ---------------------------------------------------------------------------
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
    // not repeated.  One resume per sizing call: a call that has copied is never a source of tables.
    const drx_plan::GatherKey K = p->gat_last;
    p->gat_last.valid = false;
    if (K.valid && d_out && K.d_in == d_in && K.in_words == in_words && K.d_off == d_chunk_word_off && K.d_sideband == (sideband ? d_sideband : nullptr) &&
        K.n_sel == n_sel && K.cw == cw && memcmp(p->h_sel, wave_idx, n_sel * sizeof(uint64_t)) == 0) {
        DRX_ON_DEVICE(ctx);
        StreamCall c;
        if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, nullptr, true, &c)) return st;
        const SelStaged S = sel_staged(p, n_sel, n_out);
        mark(c.ev, 0, c.s);
        mark(c.ev, 1, c.s);
        DRX_HIP(ctx, launch_gather(c, S.d_sel, n_sel, cw, S.d_chunk_n, out, gather_scratch_view(p->d_gat, n_sel), tiles, mean_words, /*resume*/ true));
        mark(c.ev, 3, c.s);
        return call_end(p, DRX_PATH_GATHER);
    }
    // every output chunk is a chunk under ONE WaveformLength (its first entry's; only its last entry may be shorter) of fewer
    // than 2^31 samples (src/deltaRice.c:389); chunk_n[c] = its sample count N_c
    std::vector<uint32_t> chunk_n(n_out);
    uint32_t first = 0, n_class[3];
    uint64_t left = 0, sum = 0, oc = ~0ull;  // entries left in the current output chunk, its samples so far, its number
    bool closed = false;         // a shorter entry has been seen: it must be the chunk's last
    std::vector<uint32_t> lists;
    if (const drx_status st = sel_survey(p, "gather_encoded", wave_idx, n_sel, sideband, lists, n_class, [&](uint64_t i, uint64_t, uint32_t len) {
            if (left == 0) { left = cw; first = len; sum = 0; closed = false; ++oc; }
            if (closed)
                return fail(ctx, DRX_ERR_ARG, "gather_encoded: entry %llu is shorter than output chunk %llu's first (%u samples) and not its last",
                            (unsigned long long)(i - 1), (unsigned long long)oc, first);
            if (len > first)
                return fail(ctx, DRX_ERR_ARG, "gather_encoded: entry %llu has %u samples, output chunk %llu's first has %u",
                            (unsigned long long)i, len, (unsigned long long)oc, first);
            closed = len < first;
            sum += len;
            if (sum >= (1ull << 31))
                return fail(ctx, DRX_ERR_ARG, "gather_encoded: output chunk %llu reaches 2^31 samples at entry %llu", (unsigned long long)oc,
                            (unsigned long long)i);
            chunk_n[oc] = (uint32_t)sum;
            --left;
            return DRX_OK;
        }))
        return st;
    DRX_ON_DEVICE(ctx);
    if (const drx_status st = sel_stage(p, wave_idx, n_sel, chunk_n, lists, gather_scratch_view(nullptr, n_sel).bytes)) return st;
    const SelStaged S = sel_staged(p, n_sel, n_out);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, nullptr, false, &c)) return st;
    if (const drx_status st = sel_walk(p, c, sideband ? d_sideband : nullptr, S.d_lists, lists.size(), n_class)) return st;
    DRX_HIP(ctx, launch_gather(c, S.d_sel, n_sel, cw, S.d_chunk_n, out, gather_scratch_view(p->d_gat, n_sel), tiles, mean_words, /*resume*/ false));
    mark(c.ev, 3, c.s);
    p->gat_last.valid = d_out == nullptr;
    p->gat_last.d_in = d_in; p->gat_last.in_words = in_words; p->gat_last.d_off = d_chunk_word_off;
    p->gat_last.d_sideband = sideband ? d_sideband : nullptr; p->gat_last.n_sel = n_sel; p->gat_last.cw = cw;
    return call_end(p, DRX_PATH_GATHER);
}

drx_status drx_gather_encoded(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const uint64_t *wave_idx, uint64_t n_sel, uint64_t out_chunk_waves, uint32_t *d_out,
                              uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    try {
        return gather_encoded(p, d_in, in_words, d_chunk_word_off, nullptr, false, wave_idx, n_sel, out_chunk_waves, d_out, out_cap_words,
                              d_out_chunk_word_off, d_out_wave_words);
    } catch (const std::bad_alloc &) { return fail(p->ctx, DRX_ERR_NOMEM, "gather_encoded: host memory for a list of %llu entries", (unsigned long long)n_sel); }
}

drx_status drx_gather_encoded_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                              const uint32_t *d_wave_words, const uint64_t *wave_idx, uint64_t n_sel,
                                              uint64_t out_chunk_waves, uint32_t *d_out, uint64_t out_cap_words,
                                              uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    try {
        return gather_encoded(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, wave_idx, n_sel, out_chunk_waves, d_out, out_cap_words,
                              d_out_chunk_word_off, d_out_wave_words);
    } catch (const std::bad_alloc &) { return fail(p->ctx, DRX_ERR_NOMEM, "gather_encoded: host memory for a list of %llu entries", (unsigned long long)n_sel); }
}

// ---------------------------------------------------------------------------
// The calls that read the whole batch from the encoded stream without decoding it -- wave_stats, decode_window(s), find_pulses,
// transcode, estimate_words_encoded -- open with stream_call_begin() and close with call_end() (above).  stream_call_args(): the
// pointers every one of them takes (have_pointers: the caller's own included; who: its name in the message).
// ---------------------------------------------------------------------------
static drx_status stream_call_args(drx_plan *p, const char *who, bool have_pointers, const uint32_t *d_sideband, bool sideband) {
    if (!have_pointers || (sideband && !d_sideband)) return fail(p->ctx, DRX_ERR_ARG, "%s: null pointer", who);
    if (sideband && d_sideband == p->d_wave_words) return fail(p->ctx, DRX_ERR_ARG, "the side-band table must not be the plan's own (copy it first)");
    return DRX_OK;
}
// A block form's scratch (*d) belongs to the plan and is allocated by the first call that takes that form (BlkFormRule, drx_internal.h)
static hipError_t form_scratch(drx_plan *p, const BlkFormRule &r, void **d, uint64_t (*bytes)(const Geom &)) {
    return (!*d && blocks_form_batch(p->G, p->d_blk, r)) ? p->mem.alloc(d, bytes(p->G)) : hipSuccess;
}

// ---------------------------------------------------------------------------
// per-waveform statistics from the encoded stream (drx_stats.hip)
// ---------------------------------------------------------------------------
static drx_status wave_stats(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint32_t *d_sideband, bool sideband, uint32_t head_len, int64_t *d_out) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "wave_stats", d_in && d_chunk_word_off && d_out, d_sideband, sideband)) return st;
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kStatsForm, &p->d_sacc, stats_blocks_scratch_bytes));  // accumulators and list
    DRX_HIP(ctx, launch_wave_stats(c, p->d_blk, p->d_sacc, head_len, d_out, &p->last_stats_form));
    return call_end(p, DRX_PATH_STATS);
}

drx_status drx_wave_stats(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, uint32_t head_len,
                          int64_t *d_out) {
    return wave_stats(p, d_in, in_words, d_chunk_word_off, nullptr, false, head_len, d_out);
}

drx_status drx_wave_stats_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                          const uint32_t *d_wave_words, uint32_t head_len, int64_t *d_out) {
    return wave_stats(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, head_len, d_out);
}

// ---------------------------------------------------------------------------
// a window of every waveform, at per-waveform offsets (drx_window.hip)
// ---------------------------------------------------------------------------
static drx_status decode_window(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                const uint32_t *d_sideband, bool sideband, const int64_t *d_start, uint64_t start_stride,
                                int64_t offset, uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "decode_window", d_in && d_chunk_word_off && d_out, d_sideband, sideband)) return st;
    if (out_stride < width)
        return fail(ctx, DRX_ERR_ARG, "decode_window: rows %llu samples apart do not hold %u", (unsigned long long)out_stride, width);
    if (d_start && start_stride == 0) return fail(ctx, DRX_ERR_ARG, "decode_window: start_stride 0");
    if (width == 0) return DRX_OK;  // (no row receives a sample: nothing to launch)
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, launch_decode_window(c, d_start, start_stride, offset, width, pad, d_out, out_stride));
    return call_end(p, DRX_PATH_WINDOW);
}

drx_status drx_decode_window(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const int64_t *d_start, uint64_t start_stride, int64_t offset, uint32_t width, int16_t pad,
                             int16_t *d_out, uint64_t out_stride_samples) {
    return decode_window(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_start, start_stride, offset, width, pad, d_out,
                         out_stride_samples);
}

drx_status drx_decode_window_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                             const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_stride,
                                             int64_t offset, uint32_t width, int16_t pad, int16_t *d_out,
                                             uint64_t out_stride_samples) {
    return decode_window(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_start, start_stride, offset, width, pad, d_out,
                         out_stride_samples);
}

// ---------------------------------------------------------------------------
// several windows of every waveform, at per-window starts (drx_windows.hip)
// ---------------------------------------------------------------------------
static drx_status decode_windows(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                 const uint32_t *d_sideband, bool sideband, const int64_t *d_start, uint64_t start_wave_stride,
                                 uint64_t start_win_stride, const uint32_t *d_count, uint32_t n_win, int64_t offset, uint32_t width,
                                 int16_t pad, int16_t *d_out, uint64_t out_wave_stride, uint64_t out_win_stride) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "decode_windows", d_in && d_chunk_word_off && d_start && d_out, d_sideband, sideband)) return st;
    if (start_wave_stride == 0 || start_win_stride == 0) return fail(ctx, DRX_ERR_ARG, "decode_windows: a start stride of 0");
    if (out_win_stride < width)
        return fail(ctx, DRX_ERR_ARG, "decode_windows: rows %llu samples apart do not hold %u", (unsigned long long)out_win_stride, width);
    // a waveform's rows must end in front of the next one's: (n_win - 1) * out_win_stride + width samples, in 128 bits
    if (n_win && (unsigned __int128)(n_win - 1u) * out_win_stride + width > (unsigned __int128)out_wave_stride)
        return fail(ctx, DRX_ERR_ARG, "decode_windows: waveforms %llu samples apart do not hold %u rows %llu apart",
                    (unsigned long long)out_wave_stride, n_win, (unsigned long long)out_win_stride);
    if (width == 0 || n_win == 0) return DRX_OK;  // (no row receives a sample: nothing to launch)
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kWindowsForm, &p->d_wtab, windows_blocks_scratch_bytes));  // the list
    DRX_HIP(ctx, launch_decode_windows(c, p->d_blk, p->d_wtab, d_start, start_wave_stride, start_win_stride, d_count, n_win, offset, width, pad,
                                       d_out, out_wave_stride, out_win_stride, &p->last_windows_form));
    return call_end(p, DRX_PATH_WINDOWS);
}

drx_status drx_decode_windows(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const int64_t *d_start, uint64_t start_wave_stride, uint64_t start_win_stride, const uint32_t *d_count,
                              uint32_t n_win, int64_t offset, uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_wave_stride,
                              uint64_t out_win_stride) {
    return decode_windows(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_start, start_wave_stride, start_win_stride, d_count, n_win,
                          offset, width, pad, d_out, out_wave_stride, out_win_stride);
}

drx_status drx_decode_windows_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                              const uint32_t *d_wave_words, const int64_t *d_start, uint64_t start_wave_stride,
                                              uint64_t start_win_stride, const uint32_t *d_count, uint32_t n_win, int64_t offset,
                                              uint32_t width, int16_t pad, int16_t *d_out, uint64_t out_wave_stride,
                                              uint64_t out_win_stride) {
    return decode_windows(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_start, start_wave_stride, start_win_stride, d_count,
                          n_win, offset, width, pad, d_out, out_wave_stride, out_win_stride);
}

// ---------------------------------------------------------------------------
// every pulse of every waveform: threshold discrimination (drx_pulses.hip)
// ---------------------------------------------------------------------------
// The block form's staging buffer (pulses_blocks_staging_bytes()); grown like the gather's scratch.
static drx_status pulses_staging(drx_plan *p, size_t bytes) {
    drx_ctx *ctx = p->ctx;
    if (p->pstage_cap >= bytes) return DRX_OK;
    void *d = nullptr;
    const hipError_t e = p->mem.alloc(&d, bytes);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_NOMEM, "find_pulses: staging of %zu bytes: %s", bytes, hipGetErrorString(e));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier call may still use the old one)
    p->mem.release(p->d_pstage);
    p->d_pstage = d;
    p->pstage_cap = bytes;
    return DRX_OK;
}

static drx_status find_pulses(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                              const uint32_t *d_sideband, bool sideband, const int64_t *d_thr, uint64_t thr_stride, int64_t thr,
                              int32_t polarity, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count, int64_t *d_out) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (const drx_status st = stream_call_args(p, "find_pulses", d_in && d_chunk_word_off && d_count, d_sideband, sideband)) return st;
    if (max_pulses && !d_out) return fail(ctx, DRX_ERR_ARG, "find_pulses: no output for %u pulses per waveform", max_pulses);
    if (polarity == 0) return fail(ctx, DRX_ERR_ARG, "find_pulses: polarity 0");
    if (min_width == 0) return fail(ctx, DRX_ERR_ARG, "find_pulses: min_width 0");
    if (d_thr && thr_stride == 0) return fail(ctx, DRX_ERR_ARG, "find_pulses: thr_stride 0");
    DRX_ON_DEVICE(ctx);
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, form_scratch(p, kPulsesForm, &p->d_ptab, pulses_blocks_scratch_bytes));  // summaries and lists
    // ... and the records its blocks stage: as many as this call needs
    if (blocks_form_batch(p->G, p->d_blk, kPulsesForm))
        if (const drx_status st = pulses_staging(p, pulses_blocks_staging_bytes(p->G, max_pulses))) return st;
    DRX_HIP(ctx, launch_find_pulses(c, p->d_blk, p->d_ptab, p->d_pstage, d_thr, thr_stride, thr, polarity < 0, min_width, max_pulses, d_count,
                                    d_out, &p->last_pulses_form));
    return call_end(p, DRX_PATH_PULSES);
}

drx_status drx_find_pulses(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                           const int64_t *d_thr, uint64_t thr_stride, int64_t thr, int32_t polarity, uint32_t min_width,
                           uint32_t max_pulses, uint32_t *d_count, int64_t *d_out) {
    return find_pulses(p, d_in, in_words, d_chunk_word_off, nullptr, false, d_thr, thr_stride, thr, polarity, min_width, max_pulses,
                       d_count, d_out);
}

drx_status drx_find_pulses_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                           const uint32_t *d_wave_words, const int64_t *d_thr, uint64_t thr_stride, int64_t thr,
                                           int32_t polarity, uint32_t min_width, uint32_t max_pulses, uint32_t *d_count,
                                           int64_t *d_out) {
    return find_pulses(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, d_thr, thr_stride, thr, polarity, min_width,
                       max_pulses, d_count, d_out);
}

// ---------------------------------------------------------------------------
// re-coding to another RiceParameter, and the sizes at every one, from the encoded stream (drx_transcode.hip)
// ---------------------------------------------------------------------------
static drx_status trc_scratch(drx_plan *p, TrcScratch *t) {  // (trc_scratch_view(), drx_internal.h; allocated by the first such call)
    if (!p->d_trc) {
        const hipError_t e = p->mem.alloc(&p->d_trc, trc_scratch_view(p->G, nullptr).bytes);
        if (e != hipSuccess) return fail(p->ctx, DRX_ERR_NOMEM, "transcode scratch: %s", hipGetErrorString(e));
    }
    *t = trc_scratch_view(p->G, p->d_trc);
    return DRX_OK;
}

static drx_status transcode(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                            const uint32_t *d_sideband, bool sideband, uint32_t new_k, uint32_t *d_out, uint64_t out_cap,
                            uint64_t *d_out_off, uint32_t *d_out_wave_words) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (new_k > 15u) return fail(ctx, DRX_ERR_ARG, "transcode: new_rice_k %u (0..15)", new_k);
    if (!d_in || !d_chunk_word_off || !d_out_off || (sideband && !d_sideband)) return fail(ctx, DRX_ERR_ARG, "transcode: null pointer");
    if (!d_out && out_cap) return fail(ctx, DRX_ERR_ARG, "transcode: no output buffer but a capacity of %llu words", (unsigned long long)out_cap);
    if (sideband && (d_sideband == p->d_wave_words || d_out_wave_words == d_sideband))
        return fail(ctx, DRX_ERR_ARG, "the side-band table must be neither the plan's own nor the output's (copy it first)");
    DRX_ON_DEVICE(ctx);
    TrcScratch t;
    if (const drx_status st = trc_scratch(p, &t)) return st;
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_sideband, false, &c)) return st;
    DRX_HIP(ctx, launch_transcode(c, new_k, t, EncOut{d_out, out_cap, d_out_off, d_out_wave_words}));
    return call_end(p, DRX_PATH_TRANSCODE);
}

drx_status drx_transcode(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, uint32_t new_rice_k,
                         uint32_t *d_out, uint64_t out_cap_words, uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return transcode(p, d_in, in_words, d_chunk_word_off, nullptr, false, new_rice_k, d_out, out_cap_words, d_out_chunk_word_off,
                     d_out_wave_words);
}

drx_status drx_transcode_with_wave_words(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                         const uint32_t *d_wave_words, uint32_t new_rice_k, uint32_t *d_out, uint64_t out_cap_words,
                                         uint64_t *d_out_chunk_word_off, uint32_t *d_out_wave_words) {
    return transcode(p, d_in, in_words, d_chunk_word_off, d_wave_words, true, new_rice_k, d_out, out_cap_words, d_out_chunk_word_off,
                     d_out_wave_words);
}

drx_status drx_estimate_words_encoded(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                                      const uint32_t *d_wave_words, uint64_t words_out[16]) {
    if (!p) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    const bool sideband = d_wave_words != nullptr;
    if (const drx_status st = stream_call_args(p, "estimate_words_encoded", d_in && d_chunk_word_off && words_out, d_wave_words, sideband)) return st;
    DRX_ON_DEVICE(ctx);
    TrcScratch t;
    if (const drx_status st = trc_scratch(p, &t)) return st;
    StreamCall c;
    if (const drx_status st = stream_call_begin(p, d_in, in_words, d_chunk_word_off, d_wave_words, false, &c)) return st;
    DRX_HIP(ctx, launch_estimate_words_encoded(c, t.est));
    (void)call_end(p, DRX_PATH_TRANSCODE);
    DRX_HIP(ctx, hipMemcpyAsync(words_out, t.est, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return drx_plan_finish(p, nullptr);  // (waits; a stream that failed validation: DRX_ERR_CORRUPT, words_out undefined)
}

// Header chain of ONE encoded chunk in host memory (src/deltaRice.c:320-325), with the validation the device
// walk does: sample count, every n_i between 1 + k and 25 bits per sample, the chain ends exactly at the chunk end.
static bool walk_chunk_host(const uint32_t *w, uint64_t n_words, uint32_t n_samples, uint32_t wave_len, uint32_t k,
                            uint64_t *wave_off, uint32_t *wave_words) {
    if (n_words < 2 || w[0] != n_samples) return false;
    const uint32_t L = wave_len ? wave_len : n_samples;
    const uint64_t W = ((uint64_t)n_samples + L - 1) / L;
    uint64_t at = 1;
    for (uint64_t i = 0; i < W; ++i) {
        if (at >= n_words) return false;
        const uint32_t n = w[at];
        const uint64_t len = (i + 1 == W) ? (uint64_t)n_samples - i * L : L;
        if (n > ((len * 25u + 31u) >> 5) || n < ((len * (k + 1u) + 31u) >> 5) || at + 1u + n > n_words) return false;
        wave_off[i] = at;
        wave_words[i] = n;
        at += (uint64_t)n + 1u;
    }
    return at == n_words;
}

drx_status drx_estimate_words(drx_plan *p, const int16_t *d_in, uint64_t words_out[16]) {
    if (!p || !d_in || !words_out) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    // the look-back scratch is idle outside drx_encode/drx_decode: its first 16 words hold the sums
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DRX_HIP(ctx, launch_estimate_words(p->G, d_in, (unsigned long long *)p->d_scan, ctx->stream));
    DRX_HIP(ctx, hipMemcpyAsync(words_out, p->d_scan, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DRX_OK;
}

drx_status drx_plan_last_timings(drx_plan *p, float ms[4]) {
    if (!p || !ms) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    if (!p->ev_valid) return fail(ctx, DRX_ERR_ARG, "set the context option \"profile\" before the call to be timed");
    DRX_ON_DEVICE(ctx);
    DRX_HIP(ctx, hipEventSynchronize(p->ev[3]));
    for (int i = 0; i < 3; ++i) DRX_HIP(ctx, hipEventElapsedTime(&ms[i], p->ev[i], p->ev[i + 1]));
    DRX_HIP(ctx, hipEventElapsedTime(&ms[3], p->ev[0], p->ev[3]));
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
    if (p->last_was_encode && !p->h_status->err && p->G.total_waves) p->enc_words_per_wave = p->h_status->total_words / p->G.total_waves;
    if (p->h_status->err & kErrInternal) return fail(ctx, DRX_ERR_DEVICE, "encoder look-back timed out (internal error)");
    if (p->h_status->err & kErrCorrupt) return fail(ctx, DRX_ERR_CORRUPT, "encoded input failed header-chain validation");
    if (p->h_status->err & kErrCapacity)
        return fail(ctx, DRX_ERR_CAPACITY, "encoded batch needs %llu words", (unsigned long long)p->h_status->total_words);
    return DRX_OK;
}

// ---------------------------------------------------------------------------
// one chunk through host memory: the body of the H5Z callback
// ---------------------------------------------------------------------------
drx_status drx_filter_chunk_host(drx_ctx *ctx, int reverse, size_t cd_nelmts, const unsigned *cd_values,
                                 const void *in, size_t nbytes, void **out, size_t *out_bytes) {
    if (!ctx || !in || !out || !out_bytes) return DRX_ERR_ARG;
    drx_opts o;
    if (drx_parse_cd_values(cd_nelmts, cd_values, &o) != DRX_OK)
        return fail(ctx, DRX_ERR_ARG, "invalid compression_opts");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DRX_ON_DEVICE(ctx);
    if (!ctx->d_off) DRX_HIP(ctx, ctx->mem.alloc(&ctx->d_off, 2 * sizeof(uint64_t)));

    uint32_t n_samples;
    if (!reverse) {
        // nbytes must be a whole number of int16 (src/deltaRice.c:394-397) and < 2^31 samples (:389)
        if (nbytes == 0 || (nbytes & 1u) || nbytes / 2 > 0x7fffffffull) return fail(ctx, DRX_ERR_ARG, "bad chunk size %zu", nbytes);
        n_samples = (uint32_t)(nbytes / 2);
    } else {
        if (nbytes < 8 || (nbytes & 3u)) return fail(ctx, DRX_ERR_CORRUPT, "encoded chunk of %zu bytes", nbytes);
        memcpy(&n_samples, in, 4);  // totalNumberPoints (:306)
        if (n_samples == 0 || n_samples > 0x7fffffffu) return fail(ctx, DRX_ERR_CORRUPT, "bad sample count in header");
        // the header is untrusted and sizes every allocation below: a code has at least 1 + k bits (:215-222), so a
        // chunk of nbytes cannot hold more than 8 * (nbytes - 8) / (1 + k) samples
        if ((uint64_t)(nbytes - 8) * 8u < (uint64_t)n_samples * (o.rice_k + 1u))
            return fail(ctx, DRX_ERR_CORRUPT, "header claims %u samples, %zu bytes cannot hold them", n_samples, nbytes);
    }
    const uint32_t L = (o.wave_len < 0) ? 0u : (uint32_t)o.wave_len;
    drx_status st = DRX_OK;
    if (!ctx->host_plan || ctx->hp_samples != n_samples || ctx->hp_L != L || ctx->hp_k != o.rice_k ||
        ctx->hp_ntaps != o.n_taps || memcmp(ctx->hp_taps, o.taps, o.n_taps * sizeof(int32_t)) != 0) {
        if (ctx->host_plan) { plan_free(ctx->host_plan); ctx->host_plan = nullptr; }
        drx_plan *np = nullptr;
        if ((st = drx_plan_create_uniform(ctx, 1, n_samples, L, o.rice_k, &np)) != DRX_OK) return st;
        if ((st = drx_plan_set_filter(np, o.n_taps, o.taps)) != DRX_OK) { plan_free(np); return st; }
        ctx->host_plan = np;
        ctx->hp_samples = n_samples; ctx->hp_L = L; ctx->hp_k = o.rice_k; ctx->hp_ntaps = o.n_taps;
        memcpy(ctx->hp_taps, o.taps, sizeof ctx->hp_taps);
    }
    drx_plan *plan = ctx->host_plan;
    const size_t raw_bytes = (size_t)n_samples * 2;
    const size_t enc_cap_bytes = (size_t)plan->max_words * 4;
    void *result = nullptr;
    do {
        if ((st = grow(ctx, &ctx->d_raw, &ctx->raw_cap, raw_bytes, false)) != DRX_OK) break;
        if ((st = grow(ctx, &ctx->d_enc, &ctx->enc_cap, reverse ? nbytes : enc_cap_bytes, false)) != DRX_OK) break;
        hipError_t e;
        if (!reverse) {
            e = hipMemcpyAsync(ctx->d_raw, in, raw_bytes, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) { st = fail(ctx, DRX_ERR_DEVICE, "H2D failed: %s", hipGetErrorString(e)); break; }
            if ((st = drx_encode(plan, (const int16_t *)ctx->d_raw, (uint32_t *)ctx->d_enc, plan->max_words, ctx->d_off)) != DRX_OK) break;
            uint64_t words = 0;
            if ((st = drx_plan_finish(plan, &words)) != DRX_OK) break;
            const size_t nb = (size_t)words * 4;
            result = malloc(nb);
            if (!result) { st = DRX_ERR_NOMEM; break; }
            e = hipMemcpyAsync(result, ctx->d_enc, nb, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { st = fail(ctx, DRX_ERR_DEVICE, "D2H failed: %s", hipGetErrorString(e)); break; }
            *out_bytes = nb;
        } else {
            // The device finds the headers of a large chunk (parallel walk: 0.14 ms for 2000 waveforms; the CPU takes 0.28 ms).
            const uint64_t W = plan->G.total_waves;
            // A chunk of a few hundred waveforms is walked on the CPU as well: ~0.14 us per hop out of host memory against
            // ~1 us per dependent load on the device (20 waveforms: 19 us) or the 60 us of the parallel walk's three launches.
            const bool device_walk = W > 512u;
            const size_t tab_bytes = 16 + (device_walk ? 0 : (size_t)W * (sizeof(uint64_t) + sizeof(uint32_t)));
            if ((st = grow(ctx, &ctx->h_pin, &ctx->pin_cap, tab_bytes, true)) != DRX_OK) break;
            uint64_t *h_off = (uint64_t *)ctx->h_pin;              // [2] chunk table, then [W] wave_off
            uint32_t *h_words = (uint32_t *)(h_off + 2 + W);       // [W] wave_words
            h_off[0] = 0;
            h_off[1] = (uint64_t)(nbytes / 4);
            e = hipMemcpyAsync(ctx->d_enc, in, nbytes, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_off, h_off, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
            if (!device_walk) {
                if (!walk_chunk_host((const uint32_t *)in, nbytes / 4, n_samples, L, o.rice_k, h_off + 2, h_words)) {
                    (void)hipStreamSynchronize(ctx->stream);
                    st = fail(ctx, DRX_ERR_CORRUPT, "encoded chunk failed header-chain validation");
                    break;
                }
                if (e == hipSuccess) e = hipMemcpyAsync(plan->d_wave_off, h_off + 2, W * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(plan->d_wave_words, h_words, W * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
            }
            // (no wait here: the pinned table is not touched again before this call's final synchronisation)
            if (e != hipSuccess) { st = fail(ctx, DRX_ERR_DEVICE, "H2D failed: %s", hipGetErrorString(e)); break; }
            if ((st = decode_launch(plan, (const uint32_t *)ctx->d_enc, nbytes / 4, ctx->d_off, (int16_t *)ctx->d_raw, !device_walk)) != DRX_OK) break;
            if ((st = drx_plan_finish(plan, nullptr)) != DRX_OK) break;
            result = malloc(raw_bytes);
            if (!result) { st = DRX_ERR_NOMEM; break; }
            e = hipMemcpyAsync(result, ctx->d_raw, raw_bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { st = fail(ctx, DRX_ERR_DEVICE, "D2H failed: %s", hipGetErrorString(e)); break; }
            *out_bytes = raw_bytes;
        }
    } while (0);
    if (st != DRX_OK) { free(result); return st; }
    *out = result;
    return DRX_OK;
}

}  // extern "C"
