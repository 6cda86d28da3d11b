// drx_gather.hip -- gather SELECTED waveforms into a new ENCODED batch (drx_gather_encoded): no code is parsed.  A waveform's
// {n_i | payload_i} is a whole number of words coded on its own (src/deltaRice.c:365-381,427-432), so the chunk the
// reference's filter emits for any list of waveforms is a header word and the waveforms' word ranges back to back.
//
// Behind the header walk over the touched chunks (launch_select_walk(), or k_sideband_tables), on the same stream:
//   k_gather_sizes     entry e contributes wave_words[sel[e]] + 1 words, one more in front of an output chunk's first entry;
//                      a sum per block of kGsBlock entries
//   k_gather_scan      one workgroup: exclusive scan of the block sums, the total, the verdict (sizing call, capacity, a
//                      corrupt touched chunk: nothing is copied)
//   k_gather_offsets   every entry's first output word, d_out_chunk_word_off, d_out_wave_words, the chunk headers N_c
//   k_gather_waves     copy, a WAVEFRONT per entry (per piece of kGcPiece words of a long one): the destination in whole
//                      aligned 16-byte stores with a head and a tail of single words, 16-byte loads at the source's 4-byte
//                      alignment, four in flight per lane before the first store
//   k_gather_tiles     copy, a workgroup per kGtEntries consecutive SHORT entries, whose output is one contiguous range: their
//                      positions in LDS, every lane finds the entry of its output words by a search there; aligned
//                      coalesced stores, gathered loads
// Every write is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "drx_internal.h"
#include "drx_device.h"

namespace drx {

constexpr uint32_t kGsThreads = 256, kGsPer = 4, kGsBlock = kGsThreads * kGsPer;  // entries per workgroup of the sizes / offsets passes
constexpr uint32_t kGcPiece = 2048;  // words of a piece (a multiple of 4: every piece of an entry has the entry's phase)
constexpr int kGcInFlight = 4;       // 16-byte loads per lane before the first store
constexpr uint32_t kGtEntries = 256, kGtThreads = 256;

// exclusive prefix sum of v over a workgroup of NT threads (a multiple of 64); *total: the workgroup's sum.  ws: NT / 64 words of LDS
template <uint32_t NT> __device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *ws, uint64_t *total) {
    const int lane = lane_id(), wv = wave_id();
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();  // (ws may still be read from the last call)
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < NT / 64; ++w) { const uint64_t s = rfl64(ws[w]); before += ((int)w < wv) ? s : 0u; all += s; }
    *total = all;
    return before + inc - v;
}

// words entry e adds to the output: its header and payload, and the chunk header in front of a chunk's first entry
__device__ __forceinline__ uint64_t gather_entry_words(uint32_t n, uint64_t e, uint64_t chunk_waves) {
    return (uint64_t)n + 1u + ((e % chunk_waves) == 0 ? 1u : 0u);
}

__global__ __launch_bounds__(kGsThreads) void k_gather_sizes(uint64_t total_waves, const uint32_t *__restrict__ wave_words,
                                                             const uint64_t *__restrict__ sel, uint64_t n_sel, uint64_t chunk_waves,
                                                             uint32_t *__restrict__ ent_words, uint64_t *__restrict__ block_sum) {
    __shared__ uint64_t ws[kGsThreads / 64];
    const uint64_t e0 = (uint64_t)blockIdx.x * kGsBlock + threadIdx.x * kGsPer;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kGsPer; ++j) {
        const uint64_t e = e0 + j;
        if (e < n_sel) {
            const uint64_t g = sel[e];
            const uint32_t n = g < total_waves ? wave_words[g] : 0u;  // (the host checked the list; never index the table with anything else)
            ent_words[e] = n;
            sum += gather_entry_words(n, e, chunk_waves);
        }
    }
    uint64_t all;
    (void)block_excl_scan<kGsThreads>(sum, ws, &all);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = all;
}

// ctrl[0] = 1: copy nothing.  block_sum[n_blocks], [n_blocks + 1] keep the total and the walk's status for a call that resumes
// from these tables (resume: nothing is scanned, they are read back)
__global__ __launch_bounds__(1024) void k_gather_scan(uint64_t *__restrict__ block_sum, uint32_t n_blocks, const uint32_t *out,
                                                      uint64_t out_cap, DevStatus *st, uint32_t *__restrict__ ctrl, bool resume) {
    __shared__ uint64_t ws[1024 / 64];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks && !resume; b0 += 1024) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t v = b < n_blocks ? block_sum[b] : 0u;
        uint64_t all;
        const uint64_t ex = block_excl_scan<1024>(v, ws, &all);
        if (b < n_blocks) block_sum[b] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) {
        uint32_t failed = st->err;  // whatever a walker reported: nothing is copied out of a batch that failed
        if (resume) {
            carry = block_sum[n_blocks];
            failed = (uint32_t)block_sum[n_blocks + 1];
            if (failed) atomicOr(&st->err, failed);
        } else {
            block_sum[n_blocks] = carry;
            block_sum[n_blocks + 1] = failed;
        }
        st->total_words = carry;
        const bool over = out && carry > out_cap;
        if (over) atomicOr(&st->err, kErrCapacity);
        ctrl[0] = (!out || over || failed) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kGsThreads) void k_gather_offsets(const uint32_t *__restrict__ ent_words, const uint64_t *__restrict__ block_sum,
                                                               uint64_t n_sel, uint64_t chunk_waves, const uint32_t *__restrict__ chunk_samples,
                                                               const DevStatus *st, const uint32_t *__restrict__ ctrl,
                                                               uint64_t *__restrict__ ent_pos, uint64_t *__restrict__ out_chunk_off,
                                                               uint32_t *__restrict__ out_wave_words, uint32_t *__restrict__ out) {
    __shared__ uint64_t ws[kGsThreads / 64];
    const uint64_t e0 = (uint64_t)blockIdx.x * kGsBlock + threadIdx.x * kGsPer;
    uint32_t n[kGsPer];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kGsPer; ++j) {
        const uint64_t e = e0 + j;
        n[j] = e < n_sel ? ent_words[e] : 0u;
        if (e < n_sel) sum += gather_entry_words(n[j], e, chunk_waves);
    }
    uint64_t all;
    uint64_t at = block_sum[blockIdx.x] + block_excl_scan<kGsThreads>(sum, ws, &all);
    const bool copy = ctrl[0] == 0u;
#pragma unroll
    for (uint32_t j = 0; j < kGsPer; ++j) {
        const uint64_t e = e0 + j;
        if (e >= n_sel) break;
        if ((e % chunk_waves) == 0) {
            const uint64_t c = e / chunk_waves;
            out_chunk_off[c] = at;
            if (copy) out[at] = chunk_samples[c];  // N_c
            ++at;
        }
        ent_pos[e] = at;  // of the entry's header word n_i
        if (out_wave_words) out_wave_words[e] = n[j];
        at += (uint64_t)n[j] + 1u;
        if (e + 1 == n_sel) out_chunk_off[(e / chunk_waves) + 1] = st->total_words;
    }
}

// sixteen bytes at any word of the stream
struct __attribute__((packed, aligned(4))) Words4 { uint32_t x, y, z, w; };

// words [0, cnt) of src to dst by one wavefront
__device__ __forceinline__ void wave_copy_words(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t cnt, uint32_t lane) {
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u) >> 2;  // single words up to the first aligned piece
    head = head < cnt ? head : cnt;
    const uint32_t nvec = (cnt - head) >> 2, tail0 = head + nvec * 4u;
    if (lane < head) dst[lane] = src[lane];
    if (lane >= 60u && tail0 + (lane - 60u) < cnt) dst[tail0 + (lane - 60u)] = src[tail0 + (lane - 60u)];
    const uint32_t *s = src + head;
    uint4 *d = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t v0 = 0; v0 < nvec; v0 += 64u * kGcInFlight) {
        Words4 r[kGcInFlight];
        // all loads first, at an index clamped into the range, so that they are in flight together
#pragma unroll
        for (int j = 0; j < kGcInFlight; ++j) {
            const uint32_t v = v0 + (uint32_t)j * 64u + lane;
            r[j] = *reinterpret_cast<const Words4 *>(s + 4u * (v < nvec ? v : nvec - 1u));
        }
#pragma unroll
        for (int j = 0; j < kGcInFlight; ++j) {
            const uint32_t v = v0 + (uint32_t)j * 64u + lane;
            if (v < nvec) d[v] = make_uint4(r[j].x, r[j].y, r[j].z, r[j].w);
        }
    }
}

// item = entry * slots + slot; a wavefront takes pieces slot, slot + slots, ... of its entry, so that any entry is copied
// whole whatever `slots` the host chose from the batch's mean code length (a speed matter only)
__global__ __launch_bounds__(256) void k_gather_waves(uint64_t total_waves, const uint32_t *__restrict__ in, const uint64_t *__restrict__ wave_off,
                                                      const uint64_t *__restrict__ sel, const uint32_t *__restrict__ ent_words,
                                                      const uint64_t *__restrict__ ent_pos, uint64_t n_sel, uint32_t slots,
                                                      const uint32_t *__restrict__ ctrl, uint32_t *__restrict__ out) {
    if (ctrl[0]) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t n_items = n_sel * slots, stride = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (uint32_t)wave_id(); it < n_items; it += stride) {
        const uint64_t e = it / slots;
        const uint32_t slot = (uint32_t)(it - e * slots);
        const uint64_t g = sel[e];
        if (g >= total_waves) continue;
        const uint64_t cnt = (uint64_t)ent_words[e] + 1u;
        const uint32_t *src = in + wave_off[g];
        uint32_t *dst = out + ent_pos[e];
        for (uint64_t p = (uint64_t)slot * kGcPiece; p < cnt; p += (uint64_t)slots * kGcPiece)
            wave_copy_words(src + p, dst + p, (uint32_t)std::min<uint64_t>(cnt - p, kGcPiece), lane);
    }
}

// A workgroup per kGtEntries consecutive entries.  Their output is the range [ent_pos[first], ent_pos[last] + n + 1), with one
// word (a chunk header, k_gather_offsets') not theirs in front of every chunk's first entry.
__global__ __launch_bounds__(kGtThreads) void k_gather_tiles(uint64_t total_waves, const uint32_t *__restrict__ in, const uint64_t *__restrict__ wave_off,
                                                             const uint64_t *__restrict__ sel, const uint32_t *__restrict__ ent_words,
                                                             const uint64_t *__restrict__ ent_pos, uint64_t n_sel,
                                                             const uint32_t *__restrict__ ctrl, uint32_t *__restrict__ out) {
    __shared__ uint64_t s_pos[kGtEntries], s_src[kGtEntries];
    __shared__ uint32_t s_cnt[kGtEntries];
    if (ctrl[0]) return;
    const uint64_t e0 = (uint64_t)blockIdx.x * kGtEntries;
    const uint32_t ne = (uint32_t)std::min<uint64_t>(n_sel - e0, kGtEntries);
    for (uint32_t i = threadIdx.x; i < ne; i += kGtThreads) {
        const uint64_t g = sel[e0 + i];
        const bool ok = g < total_waves;
        s_pos[i] = ent_pos[e0 + i];
        s_src[i] = ok ? wave_off[g] : 0u;
        s_cnt[i] = ok ? ent_words[e0 + i] + 1u : 0u;  // (n_i <= 25 bits per sample of fewer than 2^31 samples: no wrap)
    }
    __syncthreads();
    const uint64_t begin = s_pos[0], end = s_pos[ne - 1] + s_cnt[ne - 1];
    // the range in aligned 16-byte pieces of the destination; the first and the last may be partly the workgroup's
    const uint64_t phase = ((uintptr_t)out >> 2) & 3u;  // out + w is 16-byte aligned where (w + phase) % 4 == 0
    const uint64_t q0 = (begin + phase) >> 2, q1 = (end + phase + 3u) >> 2;
    for (uint64_t q = q0 + threadIdx.x; q < q1; q += kGtThreads) {
        const uint64_t w0 = q * 4u - phase;  // (q0 * 4 may lie below phase: then the words below `begin` are skipped first)
        // the last entry that starts at or before the piece's first word of the range
        const uint64_t wf = (q * 4u < phase || w0 < begin) ? begin : w0;
        uint32_t lo = 0, hi = ne;  // invariant: s_pos[lo] <= wf < s_pos[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_pos[mid] <= wf) lo = mid; else hi = mid;
        }
        uint32_t v[4];
        uint32_t have = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t w = q * 4u + j - phase;
            if (q * 4u + j < phase || w < begin || w >= end) continue;
            while (lo + 1u < ne && s_pos[lo + 1u] <= w) ++lo;
            const uint64_t rel = w - s_pos[lo];
            if (rel < s_cnt[lo]) {  // (else: a chunk header between two entries)
                v[j] = in[s_src[lo] + rel];
                have |= 1u << j;
            }
        }
        if (have == 15u) {
            *reinterpret_cast<uint4 *>(out + (q * 4u - phase)) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (have & (1u << j)) out[q * 4u + j - phase] = v[j];
        }
    }
}

uint64_t gather_scan_blocks(uint64_t n_sel) { return (n_sel + kGsBlock - 1) / kGsBlock; }

// t: gather_scratch_view(); tiles: the copy form for short entries
hipError_t launch_gather(const StreamCall &c, const uint64_t *d_sel, uint64_t n_sel, uint64_t chunk_waves,
                         const uint32_t *d_chunk_samples, const EncOut &out, const GatherScratch &t, bool tiles, uint64_t mean_words,
                         bool resume) {
    if (!n_sel) return hipSuccess;
    const Geom &G = *c.G;
    const hipStream_t s = c.s;
    uint32_t *const d_out = out.d_out;
    const unsigned nb = (unsigned)gather_scan_blocks(n_sel);
    if (!resume) k_gather_sizes<<<nb, kGsThreads, 0, s>>>(G.total_waves, c.d_wave_words, d_sel, n_sel, chunk_waves, t.ent_words, t.block_sum);
    k_gather_scan<<<1, 1024, 0, s>>>(t.block_sum, nb, d_out, out.out_cap, c.d_status, t.ctrl, resume);
    k_gather_offsets<<<nb, kGsThreads, 0, s>>>(t.ent_words, t.block_sum, n_sel, chunk_waves, d_chunk_samples, c.d_status, t.ctrl, t.ent_pos,
                                               out.d_chunk_word_off, out.d_wave_words, d_out);
    mark(c.ev, 2, s);
    if (d_out) {
        if (tiles) {
            k_gather_tiles<<<blocks_for(n_sel, kGtEntries), kGtThreads, 0, s>>>(G.total_waves, c.d_in, c.d_wave_off, d_sel, t.ent_words, t.ent_pos,
                                                                                 n_sel, t.ctrl, d_out);
        } else {
            // pieces of an entry side by side while the list alone does not fill the chip (256 CUs x 32 wavefronts)
            uint64_t slots = (mean_words + kGcPiece - 1) / kGcPiece;
            slots = std::max<uint64_t>(1, std::min<uint64_t>(slots, 1024));
            const uint64_t wgs = (n_sel * slots + 3) / 4;
            k_gather_waves<<<(unsigned)std::min<uint64_t>(wgs, 1u << 20), 256, 0, s>>>(G.total_waves, c.d_in, c.d_wave_off, d_sel, t.ent_words,
                                                                                     t.ent_pos, n_sel, (uint32_t)slots, t.ctrl, d_out);
        }
    }
    return hipGetLastError();
}

}  // namespace drx
