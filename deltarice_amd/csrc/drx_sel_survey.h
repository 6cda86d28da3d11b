// drx_sel_survey.h -- what a list of waveforms asks of a batch: pure host arithmetic in front of drx_decode_select and
// drx_gather_encoded (drx_api_select.hip), which decides what their kernels are launched over.  No HIP and no project header: the
// host compiler builds it into tests/sel_survey_host.cpp, which holds it to a plain loop.
#ifndef DRX_SEL_SURVEY_H
#define DRX_SEL_SURVEY_H
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace drx {

// The batch as the survey sees it.  A ragged batch comes with the host's chunk table: n_chunks entries of any struct with
// wave_base, n_samples, wave_len and n_waves (ChunkDesc, drx_internal.h); a uniform one needs none.
struct SelGeom {
    bool uniform;
    uint64_t n_chunks, total_waves;
    uint32_t u_n_samples, u_wave_len, u_n_waves;  // every chunk's, uniform batches
};

constexpr int kSelBadIndex = -1;  // sel_survey(): an entry is no waveform of the batch

// Every entry's chunk and length (arithmetic for a uniform batch, a bisection of the chunk table for a ragged one) handed to
// per_entry(i, chunk, len), which returns 0 or refuses the list with a value of its own; and the sorted set of chunks the
// selection touches as the walk takes them -- three lists, each sorted, by walk_class(n_waves, wave_len) (select_walk_class(),
// drx_walk.hip); the side-band takes them as one.  Returns 0, or at the first entry refused -- its number in *at --
// kSelBadIndex or what per_entry returned.
template <typename Chunk, typename Cls, typename F>
int sel_survey(const SelGeom &G, const Chunk *chunks, const uint64_t *wave_idx, uint64_t n_sel, bool sideband, Cls &&walk_class,
               std::vector<uint32_t> &lists, uint32_t n_class[3], uint64_t *at, F &&per_entry) {
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
                if (chunks[mid].wave_base <= g) lo = mid; else hi = mid;
            }
            const Chunk &d = chunks[c = lo];
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
        *at = i;
        if (wave_idx[i] >= G.total_waves) return kSelBadIndex;
        uint32_t len;
        const uint64_t c = chunk_of(wave_idx[i], &len);
        if (const int refused = per_entry(i, c, len)) return refused;
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
        auto cls = [&](uint32_t c) { return G.uniform ? walk_class(G.u_n_waves, G.u_wave_len) : walk_class(chunks[c].n_waves, chunks[c].wave_len); };
        for (uint32_t c : touched) ++n_class[cls(c)];
        uint32_t at_list[3] = {0, n_class[0], n_class[0] + n_class[1]};
        for (uint32_t c : touched) lists[at_list[cls(c)]++] = c;
    }
    return 0;
}

// The output chunks of drx_gather_encoded: every `cw` entries of the list make one, a chunk under ONE WaveformLength (its first
// entry's; only its last entry may be shorter) of fewer than 2^31 samples (src/deltaRice.c:389).  add() takes the entries in
// order and keeps chunk_n[c] = the sample count N_c of output chunk c (ceil(n_sel / cw) entries, the caller's).
struct GatherChunks {
    enum Refusal {
        kOk = 0,
        kShorterNotLast,  // entry `entry` (the one before) is shorter than the chunk's first and not its last
        kLonger,          // entry `entry` is longer than the chunk's first
        kTooLong          // the chunk reaches 2^31 samples at entry `entry`
    };
    uint64_t cw;
    uint32_t *chunk_n;
    uint32_t first = 0;  // the current output chunk's first entry's length
    uint64_t left = 0, sum = 0, oc = ~0ull;  // entries left in the current output chunk, its samples so far, its number
    bool closed = false;                     // a shorter entry has been seen: it must be the chunk's last
    uint64_t entry = 0;                      // a refusal's entry

    Refusal add(uint64_t i, uint32_t len) {
        if (left == 0) { left = cw; first = len; sum = 0; closed = false; ++oc; }
        entry = closed ? i - 1 : i;
        if (closed) return kShorterNotLast;
        if (len > first) return kLonger;
        closed = len < first;
        sum += len;
        if (sum >= (1ull << 31)) return kTooLong;
        chunk_n[oc] = (uint32_t)sum;
        --left;
        return kOk;
    }
};

}  // namespace drx
#endif
