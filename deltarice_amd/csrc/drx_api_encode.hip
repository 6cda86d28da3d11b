// drx_api_encode.hip -- C ABI glue (drx_api.h): which encoder a drx_encode call takes, its scratch, the call itself, and
// drx_estimate_words.  Host code only.
#include "drx_api.h"

using namespace drx;

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
    const uint64_t words = p->enc.words_per_wave ? p->enc.words_per_wave : (L * (2u * G.k + 7u)) / 64u;
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
    const uint64_t bps16 = p->enc.words_per_wave ? (p->enc.words_per_wave * 512u) / L : 16u * G.k + 56u;  // bits per sample x 16
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
    if (R.enc == DRX_ENC_STREAM_SEGS)
        DRX_HIP(ctx, p->mem.reserve(p->enc.scan, segs_scan_words(p->G, R.seg_target) * sizeof(uint64_t), 4, false, Buffers::KeepOld, ctx->stream));
    if (R.enc == DRX_ENC_SEGMENTS) DRX_HIP(ctx, seg_scratch(p));
    return DRX_OK;
}

extern "C" {

drx_status drx_encode(drx_plan *p, const int16_t *d_in, uint32_t *d_out, uint64_t out_cap_words,
                      uint64_t *d_chunk_word_off) {
    if (!p || !d_in || !d_out || !d_chunk_word_off) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    if (const drx_status st = call_begin(p)) return st;
    // what the plan's last encode measured decides this one's kernel -- read from the word the encoders write to pinned host
    // memory, so that callers that never wait for an encode (bench.py's steps) are covered without a copy or an event
    if (const uint64_t w = *(volatile uint64_t *)p->G.host_words) p->enc.words_per_wave = p->G.total_waves ? w / p->G.total_waves : 0;
    const EncodeRoute R = route_encode(p, ctx->encode_impl, ctx->debug_flags);
    if (const drx_status st = route_scratch(p, R)) return st;
    const EncodeCall c{&p->G, d_in, EncOut{d_out, out_cap_words, d_chunk_word_off, p->d_wave_words}, p->d_status,
                       ctx->profile ? p->prof.ev : nullptr, ctx->stream};
    const drx_plan::Encoders &E = p->enc;
    uint64_t *d_scan = (uint64_t *)E.scan.ptr;
    switch (R.enc) {
    case DRX_ENC_STREAM_SEGS: DRX_HIP(ctx, launch_encode_stream_segs(c, R.seg_target, d_scan)); break;
    case DRX_ENC_PIECES: DRX_HIP(ctx, launch_encode_pieces(c, p->G.total_samples, E.d_pc_scan, E.pc_wgs)); break;
    case DRX_ENC_SEGMENTS: DRX_HIP(ctx, launch_encode_long(c, p->d_wave_rel, p->d_chunk_words, E.d_seg_bits, E.d_seg_pos)); break;
    case DRX_ENC_STREAM: DRX_HIP(ctx, launch_encode_stream(c, d_scan)); break;
    case DRX_ENC_FUSED: DRX_HIP(ctx, launch_encode_fused(c, R.wide, d_scan)); break;
    default: DRX_HIP(ctx, launch_encode(c, p->d_wave_rel, p->d_chunk_words));
    }
    return call_end(p, R.enc, /*encode*/ true);
}

drx_status drx_estimate_words(drx_plan *p, const int16_t *d_in, uint64_t words_out[16]) {
    if (!p || !d_in || !words_out) return DRX_ERR_ARG;
    drx_ctx *ctx = p->ctx;
    DRX_ON_DEVICE(ctx);
    // the look-back scratch is idle outside drx_encode/drx_decode: its first 16 words hold the sums
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DRX_HIP(ctx, launch_estimate_words(p->G, d_in, (unsigned long long *)p->enc.scan.ptr, ctx->stream));
    DRX_HIP(ctx, hipMemcpyAsync(words_out, p->enc.scan.ptr, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    DRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DRX_OK;
}

}  // extern "C"
