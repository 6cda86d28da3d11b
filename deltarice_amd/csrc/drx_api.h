// drx_api.h -- what the C ABI glue (drx_api_*.hip) shares: the context and the plan, the memory they own, the device guard, and
// the begin and end of every call.  Host code only; no translation unit that includes it for these holds device code.
#ifndef DRX_API_H
#define DRX_API_H
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/deltarice_hip.h"
#include "drx_internal.h"

// A buffer that a later call may need larger (Buffers::reserve())
struct Grown {
    void *ptr = nullptr;
    size_t cap = 0;  // bytes
};

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
    // A buffer that the first call that needs it allocates, at a size that never changes
    template <typename T> hipError_t once(T **out, size_t bytes, bool pinned = false) {
        return *out ? hipSuccess : alloc(out, bytes, pinned);
    }

    // The ONE rule by which a buffer grows: b holds at least `need` bytes afterwards, its contents undefined if it was replaced.
    // A replacement allocates need + need / slack + 4096 bytes (slack 0: need), size() below, and waits for `wait` before the old
    // buffer is released (a kernel or copy of an earlier call may still use it).  What differs between the sites, and nothing else:
    //   buffer                     | owner   | memory | order        | slack | a failure is reported as
    //   ---------------------------+---------+--------+--------------+-------+------------------------------------------------------
    //   d_raw, d_enc (host path)   | context | device | ReleaseFirst | 4     | DRX_ERR_DEVICE "allocation of %zu bytes failed: %s"
    //   h_pin (host path)          | context | pinned | ReleaseFirst | 4     | DRX_ERR_DEVICE, the same
    //   h_stage (host_staging)     | context | pinned | ReleaseFirst | 8     | DRX_ERR_NOMEM  "pinned staging buffer of %zu bytes: %s"
    //   enc.scan (forced route)    | plan    | device | KeepOld      | 4     | DRX_ERR_DEVICE (DRX_HIP)
    //   sel.h (selection staging)  | plan    | pinned | KeepOld      | 4     | DRX_ERR_DEVICE (DRX_HIP)
    //   sel.d (its device copy)    | plan    | device | KeepOld      | 4     | DRX_ERR_NOMEM  "selection scratch of %zu bytes: %s"
    //   gat.d (gather)             | plan    | device | KeepOld      | 4     | DRX_ERR_NOMEM  "gather scratch of %zu bytes: %s"
    //   pulses.stage (block form)  | plan    | device | KeepOld      | none  | DRX_ERR_NOMEM  "find_pulses: staging of %zu bytes: %s"
    // KeepOld: the larger buffer first -- should that fail, the plan keeps what it had.  ReleaseFirst: the context's buffers are
    // filled anew by every call and a chunk's can be gigabytes, so the two never exist side by side.  A failed wait is returned
    // like a failed allocation (under KeepOld the owner keeps what it had).
    enum Order { KeepOld, ReleaseFirst };
    static size_t size(size_t need, unsigned slack) { return slack ? need + need / slack + 4096 : need; }
    hipError_t reserve(Grown &b, size_t need, unsigned slack, bool pinned, Order order, hipStream_t wait) {
        if (b.cap >= need) return hipSuccess;
        void *fresh = nullptr;
        hipError_t e = order == KeepOld ? alloc(&fresh, size(need, slack), pinned) : hipSuccess;
        if (e == hipSuccess && b.ptr) e = hipStreamSynchronize(wait);
        if (e != hipSuccess) { release(fresh); return e; }
        release(b.ptr);
        b = Grown{};
        if (order == ReleaseFirst && (e = alloc(&fresh, size(need, slack), pinned)) != hipSuccess) return e;
        b = Grown{fresh, size(need, slack)};
        return hipSuccess;
    }
};

// What the one-chunk host path's cached plan was made for
struct HostPlanKey {
    uint32_t samples = 0, wave_len = 0, k = 0, n_taps = 0;
    int32_t taps[DRX_MAX_TAPS] = {0};  // (zero beyond n_taps: drx_parse_cd_values())
    bool operator==(const HostPlanKey &o) const {
        return samples == o.samples && wave_len == o.wave_len && k == o.k && n_taps == o.n_taps && memcmp(taps, o.taps, sizeof taps) == 0;
    }
};

struct drx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    drx::SideStream side{nullptr, nullptr, nullptr};  // independent kernels of one call (launch_decode)
    int decode_impl = 8;   // launch_decode(): 8 = walk fused into the staged kernel (default), 7 = the same with a separate
                           // walk kernel, 0 = simple kernel
    int encode_impl = 2;  // 2: single pass, persistent (k_encode_stream) where the standard geometry applies; 1: single pass with
                          // look-back (k_encode_fused) everywhere; 0: size pass + scan + pack pass
    int bins_impl = 0;    // launch_wave_bins(): 0 = a lane per waveform whatever the batch (default), 1 = the block form where
                          // blocks_form_batch() admits the batch under kBinsForm (drx_bins_blocks.hip)
    uint32_t stack_workgroups = 0;  // launch_wave_stack(): 0 = the resident grid (default), n = at most n persistent workgroups per tile
    int profile = 0;      // bracket kernels with HIP events (drx_plan_last_timings)
    uint32_t debug_flags = 0;  // Geom::dbg
    std::string last_error;
    Buffers mem;  // owns the buffers below
    // The one-chunk host path (drx_filter_chunk_host): its scratch, grown on demand, and its plan, kept between calls -- HDF5
    // calls the filter once per chunk with the same geometry, and creating a plan costs its allocations and frees (about a
    // millisecond)
    struct HostPath {
        Grown d_raw, d_enc, h_pin;
        uint64_t *d_off = nullptr;  // the chunk's two offsets, allocated by the first call
        drx_plan *plan = nullptr;
        HostPlanKey key;
    } host;
    Grown h_stage;  // drx_ctx_host_staging(): the direct-chunk HDF5 path's staging buffer
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
        return drx::fail((ctx), DRX_ERR_DEVICE, "hipSetDevice(%d) failed: %s", (ctx)->device, hipGetErrorString(dev_guard_.err))

// A plan: the batch's geometry, the tables and status every call uses, and each call's own scratch under that call's name.
// Scratch marked "first call" is allocated by the first call that needs it (Buffers::once()), a Grown by Buffers::reserve().
struct drx_plan {
    drx_ctx *ctx = nullptr;
    drx::Geom G{};  // its device tables (chunks, walk lists, taps, ...) and pinned host_words are buffers of mem, held nowhere else
    Buffers mem;    // owns every buffer of the plan
    uint64_t max_words = 0;
    std::vector<drx::ChunkDesc> host_chunks;  // the host's chunk table (ragged plans): what a selection is surveyed against
    uint32_t *d_wave_words = nullptr;  // n_i
    uint32_t *d_wave_rel = nullptr;    // encode: header position relative to chunk start
    uint64_t *d_wave_off = nullptr;    // decode: absolute header position
    uint64_t *d_chunk_words = nullptr;
    drx::DevStatus *d_status = nullptr;
    drx::DevStatus *h_status = nullptr;  // pinned
    bool last_was_encode = false;
    struct Encoders {
        Grown scan;                      // look-back state of the single-pass encoders + ticket; the decoder's granules
        uint32_t *d_seg_bits = nullptr;  // segment encoder: bits and bit position of every segment (both or neither: seg_scratch())
        uint64_t *d_seg_pos = nullptr;
        uint64_t *d_pc_scan = nullptr;   // pieces encoder: look-back entry per workgroup + ticket
        uint64_t pc_wgs = 0;             // its workgroups (0: the plan's geometry never takes it)
        uint32_t last_path = 0;          // DRX_ENC_* of the last drx_encode
        uint64_t words_per_wave = 0;     // of the plan's last encode (0: none yet)
    } enc;
    struct Decoder {
        void *d_pw = nullptr;    // a handful of chunks: candidate lists of the parallel header walk
        void *d_blk = nullptr;   // few waveforms: unit table, look-back state and flags of the block-parallel decoder
        uint32_t last_path = 0;  // DRX_PATH_* of the last call on an encoded batch
    } dec;
    // The block forms beside the decoder's (BlkFormRule, drx_internal.h): each one's own scratch (first call) and DRX_*_FORM_* of
    // the last call (0: none yet)
    struct BlockForm {
        void *d = nullptr;
        uint32_t last_form = 0;
    };
    BlockForm stats;    // drx_wave_stats: accumulators and list
    BlockForm windows;  // drx_decode_windows: its list
    BlockForm bins;     // drx_wave_bins: its list (allocated under bins_impl 1 only)
    struct Pulses : BlockForm {  // drx_find_pulses: block summaries and list ...
        Grown stage;             // ... and the records its blocks stage: as many as the call needs (pulses_blocks_staging_bytes())
    } pulses;
    // drx_transcode / drx_estimate_words_encoded: uint64 chunk_words[n_chunks + 1] | uint64 est[16] | uint32 n_i'[W] | uint32
    // header positions[W] of the RESULT (the plan's own tables describe the source); first call
    // ... and the block form's own scratch and form word (trc_blocks_scratch_bytes(): accumulators, list, block-slot table)
    struct Transcode { void *d = nullptr; BlockForm blocks; } trc;
    void *stack_list = nullptr;  // drx_wave_stack under a selection: the listed waveforms (stack_list_bytes(), drx_internal.h); first call
    // drx_decode_select and the gather's front end
    struct Selection {
        Grown h, d;  // uint64 sel[n_sel] | uint32 chunk_n[n_out] | uint32 chunk lists[touched]: pinned staging and its device copy
        uint32_t *d_fail = nullptr;   // uint32[n_chunks]: chunks the chunk-wide walk handed to the scalar walker; first call
        hipEvent_t copied = nullptr;  // the staging buffer has crossed to the device (the next call may fill it again); first call
    } sel;
    // drx_gather_encoded: positions, sizes and scan state (gather_scratch_view(), drx_internal.h) ...
    struct Gather {
        Grown d;
        // ... and what the plan's last call was asked IF that call was a gather's SIZING call (d_out == NULL: it wrote no output):
        // its list is still in sel.h / sel.d, its tables (the walk's, sizes, scanned block sums, total and verdict) in d_wave_* /
        // d.  The gather with the same arguments right behind it resumes from them, once.  `valid` is cleared by every other call
        // on the plan that launches or writes one of those buffers, by a gather that regrows sel.h / d (so a valid key always fits
        // the buffers it describes), and by the resumed call itself: no call that copied anything is ever resumed from
        struct Key {
            bool valid = false;
            const uint32_t *d_in = nullptr, *d_sideband = nullptr;
            const uint64_t *d_off = nullptr;
            uint64_t in_words = 0, n_sel = 0, cw = 0;
        } last;
    } gat;
    struct Profiling {
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        bool valid = false;  // the last call recorded them
    } prof;
};

namespace drx {

drx_status fail(drx_ctx *ctx, drx_status st, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

#define DRX_HIP(ctx, expr)                                                                           \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return drx::fail((ctx), DRX_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

void plan_free(drx_plan *p);
hipError_t seg_scratch(drx_plan *p);  // the segment encoder's scratch, if the plan has none yet

// ---------------------------------------------------------------------------
// Every call that launches opens with call_begin(), on the context's device: the resume key dropped (a no-op for the selection
// calls, which drop it earlier -- before the early returns their argument checks leave them), the plan's status word cleared on
// the stream, the debug flags copied.  The frame a call hands its launchers (drx_internal.h) is built from the plan behind it:
// stream_call_begin() for the calls on an encoded batch, whose side-band form (d_sideband: the WHOLE batch's table) gets its
// header tables here.  call_end(): what the plan remembers of its last call.  stream_call_args(): the pointers every call on an
// encoded batch takes (have_pointers: the caller's own included; who: its name in the message).
// ---------------------------------------------------------------------------
drx_status call_begin(drx_plan *p);
drx_status stream_call_begin(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off,
                             const uint32_t *d_sideband, bool tables_ready, StreamCall *c);
drx_status call_end(drx_plan *p, uint32_t path, bool encode = false);
drx_status stream_call_args(drx_plan *p, const char *who, bool have_pointers, const uint32_t *d_sideband, bool sideband);

// drx_decode behind its argument checks (the one-chunk host path comes with its header tables ready)
drx_status decode_launch(drx_plan *p, const uint32_t *d_in, uint64_t in_words, const uint64_t *d_chunk_word_off, int16_t *d_out,
                         bool tables_ready, const uint32_t *d_sideband = nullptr);

}  // namespace drx
#endif
