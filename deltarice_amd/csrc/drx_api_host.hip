// drx_api_host.hip -- C ABI glue (drx_api.h): one chunk through host memory, the body of the H5Z callback.  Host code only.
#include <cstdlib>

#include "drx_api.h"
#include "drx_device.h"

using namespace drx;

// Header chain of ONE encoded chunk in host memory (src/deltaRice.c:320-325), with the validation the device
// walk does: sample count, every n_i between 1 + k and 25 bits per sample, the chain ends exactly at the chunk end.
static bool walk_chunk_host(const uint32_t *w, uint64_t n_words, uint32_t n_samples, uint32_t wave_len, uint32_t k,
                            uint64_t *wave_off, uint32_t *wave_words) {
    if (n_words < 2 || w[0] != n_samples) return false;
    const uint32_t L = wave_len ? wave_len : n_samples;
    const uint64_t W = ((uint64_t)n_samples + L - 1) / L;  // (< 2^31: n_samples is)
    const HeaderBounds hb = header_bounds(L, n_samples, (uint32_t)W, k);
    uint64_t at = 1;
    for (uint64_t i = 0; i < W; ++i) {
        if (at >= n_words) return false;
        const uint32_t n = w[at];
        if (!hb.ok(n, i + 1 == W) || at + 1u + n > n_words) return false;
        wave_off[i] = at;
        wave_words[i] = n;
        at += (uint64_t)n + 1u;
    }
    return at == n_words;
}

// the context's host-path buffers: a call that needs more replaces the buffer (Buffers::reserve(): the old one goes first)
static drx_status grow(drx_ctx *ctx, Grown &b, size_t need, bool pinned) {
    const hipError_t e = ctx->mem.reserve(b, need, 4, pinned, Buffers::ReleaseFirst, ctx->stream);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_DEVICE, "allocation of %zu bytes failed: %s", Buffers::size(need, 4), hipGetErrorString(e));
    return DRX_OK;
}

// What both directions share: the chunk's sample count -- the input's size forward, the untrusted header's in reverse -- and
// the plan for it, the one kept from the last call if that was made for the same chunk shape and options
static drx_status host_chunk_plan(drx_ctx *ctx, bool reverse, const drx_opts &o, const void *in, size_t nbytes, drx_plan **plan) {
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
    drx_ctx::HostPath &H = ctx->host;
    HostPlanKey key{n_samples, (o.wave_len < 0) ? 0u : (uint32_t)o.wave_len, o.rice_k, o.n_taps};
    memcpy(key.taps, o.taps, sizeof key.taps);
    if (!H.plan || !(H.key == key)) {
        if (H.plan) { plan_free(H.plan); H.plan = nullptr; }
        drx_plan *np = nullptr;
        if (const drx_status st = drx_plan_create_uniform(ctx, 1, n_samples, key.wave_len, o.rice_k, &np)) return st;
        if (const drx_status st = drx_plan_set_filter(np, o.n_taps, o.taps)) { plan_free(np); return st; }
        H.plan = np;
        H.key = key;
    }
    *plan = H.plan;
    return DRX_OK;
}

// the copy of the result that the caller receives: `bytes` of d_src, behind everything on the stream
static drx_status host_result(drx_ctx *ctx, const void *d_src, size_t bytes, void **out, size_t *out_bytes) {
    void *result = malloc(bytes);
    if (!result) return DRX_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(result, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { free(result); return fail(ctx, DRX_ERR_DEVICE, "D2H failed: %s", hipGetErrorString(e)); }
    *out_bytes = bytes;
    *out = result;
    return DRX_OK;
}

static drx_status host_forward(drx_ctx *ctx, drx_plan *plan, const void *in, void **out, size_t *out_bytes) {
    drx_ctx::HostPath &H = ctx->host;
    const size_t raw_bytes = (size_t)plan->G.total_samples * 2;
    if (const drx_status st = grow(ctx, H.d_raw, raw_bytes, false)) return st;
    if (const drx_status st = grow(ctx, H.d_enc, (size_t)plan->max_words * 4, false)) return st;
    const hipError_t e = hipMemcpyAsync(H.d_raw.ptr, in, raw_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(ctx, DRX_ERR_DEVICE, "H2D failed: %s", hipGetErrorString(e));
    if (const drx_status st = drx_encode(plan, (const int16_t *)H.d_raw.ptr, (uint32_t *)H.d_enc.ptr, plan->max_words, H.d_off)) return st;
    uint64_t words = 0;
    if (const drx_status st = drx_plan_finish(plan, &words)) return st;
    return host_result(ctx, H.d_enc.ptr, (size_t)words * 4, out, out_bytes);
}

static drx_status host_reverse(drx_ctx *ctx, drx_plan *plan, const void *in, size_t nbytes, void **out, size_t *out_bytes) {
    drx_ctx::HostPath &H = ctx->host;
    const size_t raw_bytes = (size_t)plan->G.total_samples * 2;
    if (const drx_status st = grow(ctx, H.d_raw, raw_bytes, false)) return st;
    if (const drx_status st = grow(ctx, H.d_enc, nbytes, false)) return st;
    // The device finds the headers of a large chunk (parallel walk: 0.14 ms for 2000 waveforms; the CPU takes 0.28 ms).
    const uint64_t W = plan->G.total_waves;
    // A chunk of a few hundred waveforms is walked on the CPU as well: ~0.14 us per hop out of host memory against
    // ~1 us per dependent load on the device (20 waveforms: 19 us) or the 60 us of the parallel walk's three launches.
    const bool device_walk = W > 512u;
    const size_t tab_bytes = 16 + (device_walk ? 0 : (size_t)W * (sizeof(uint64_t) + sizeof(uint32_t)));
    if (const drx_status st = grow(ctx, H.h_pin, tab_bytes, true)) return st;
    uint64_t *h_off = (uint64_t *)H.h_pin.ptr;        // [2] chunk table, then [W] wave_off
    uint32_t *h_words = (uint32_t *)(h_off + 2 + W);  // [W] wave_words
    h_off[0] = 0;
    h_off[1] = (uint64_t)(nbytes / 4);
    hipError_t e = hipMemcpyAsync(H.d_enc.ptr, in, nbytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(H.d_off, h_off, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
    if (!device_walk) {
        if (!walk_chunk_host((const uint32_t *)in, nbytes / 4, plan->G.u_n_samples, plan->G.u_wave_len, plan->G.k, h_off + 2, h_words)) {
            (void)hipStreamSynchronize(ctx->stream);
            return fail(ctx, DRX_ERR_CORRUPT, "encoded chunk failed header-chain validation");
        }
        if (e == hipSuccess) e = hipMemcpyAsync(plan->d_wave_off, h_off + 2, W * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(plan->d_wave_words, h_words, W * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    }
    // (no wait here: the pinned table is not touched again before this call's final synchronisation)
    if (e != hipSuccess) return fail(ctx, DRX_ERR_DEVICE, "H2D failed: %s", hipGetErrorString(e));
    if (const drx_status st = decode_launch(plan, (const uint32_t *)H.d_enc.ptr, nbytes / 4, H.d_off, (int16_t *)H.d_raw.ptr, !device_walk)) return st;
    if (const drx_status st = drx_plan_finish(plan, nullptr)) return st;
    return host_result(ctx, H.d_raw.ptr, raw_bytes, out, out_bytes);
}

extern "C" drx_status drx_filter_chunk_host(drx_ctx *ctx, int reverse, size_t cd_nelmts, const unsigned *cd_values,
                                            const void *in, size_t nbytes, void **out, size_t *out_bytes) {
    if (!ctx || !in || !out || !out_bytes) return DRX_ERR_ARG;
    drx_opts o;
    if (drx_parse_cd_values(cd_nelmts, cd_values, &o) != DRX_OK)
        return fail(ctx, DRX_ERR_ARG, "invalid compression_opts");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DRX_ON_DEVICE(ctx);
    DRX_HIP(ctx, ctx->mem.once(&ctx->host.d_off, 2 * sizeof(uint64_t)));
    drx_plan *plan;
    if (const drx_status st = host_chunk_plan(ctx, reverse != 0, o, in, nbytes, &plan)) return st;
    return reverse ? host_reverse(ctx, plan, in, nbytes, out, out_bytes) : host_forward(ctx, plan, in, out, out_bytes);
}
