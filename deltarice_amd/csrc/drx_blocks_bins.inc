// drx_blocks_bins.inc -- phase 2 of k_bins_blocks (drx_bins_blocks.hip), included by drx_blocks_body.inc under `if constexpr (BINS)`:
// every lane reduces its own samples bin by bin, the block merges the partial rows into the caller's rows.  As in the statistics
// form everything in front of a lane's first code is exact by now -- its index in the waveform, how many of its codes are samples,
// the running sum in front of them -- and nothing is put in output order.  Where a lane is among the bins is a BinCursor begun at
// its first sample (drx_bin_cursor.h); where a partial row goes depends on the geometry and the sample index alone and is a row of
// the block's own waveform: a block whose start is later corrected may merge wrong values into those rows (the waveform is then
// listed, and k_wave_bins_list writes every one of its rows again), never outside them -- the rule copy_out states for WINDOWS.
// The caller's rows are the accumulators: k_bins_fill has set them to the identity, and partial rows are merged with 64-bit
// integer atomics (add, add, signed min, signed max), which give the same answer in any order.  They are reduced on chip first;
// the block chooses by the bins [bF, bF + nbm) its samples meet:
//   one bin           the statistics form's reduction: shuffles, then s_e across the wavefronts, four atomics per block;
//   up to `tcap`      a table in LDS, an entry per bin the block meets, merged into with LDS atomics and flushed by the threads
//                     with four atomics per entry.  No LDS is added for it: where the lanes read the running sums phase 1 staged
//                     the table lies in the block's IMAGE, which nothing reads behind phase 1, and where they parse a second
//                     time (they read the image then) it lies in the staging buffer, which nothing reads then;
//   more              every lane sends its partial rows to the caller's rows itself.  Correct, not tuned (bins of a few samples).
                const uint32_t base16 = (acc_base + pre_s + incl_s - sum) & 0xffffu;  // the running sum in front of my first sample
                const uint32_t i0 = blk_first + rel0;                                 // its index in the waveform
                const int64_t b_a = bins_origin(ba.start, ba.start_stride, ba.offset, g);
                const uint32_t b_bin = ba.bin, b_n = ba.n_bins;
                unsigned long long *const b_rows = reinterpret_cast<unsigned long long *>(ba.rows + g * ba.wave_stride);
                // the bins the block's samples [blk_first, blk_first + blk_count) meet (the same in every thread)
                uint32_t bF = 0, nbm = 0;
                if (blk_count != 0u) {
                    const uint32_t last = blk_first + blk_count - 1u;
                    if (b_a <= (int64_t)last) {
                        const uint32_t lo = b_a > (int64_t)blk_first ? (uint32_t)b_a : blk_first;
                        const uint64_t b_lo = ((uint64_t)lo - (uint64_t)b_a) / b_bin;  // (below 2^63 + 2^31)
                        if (b_lo < b_n) {
                            const uint64_t b_hi = ((uint64_t)last - (uint64_t)b_a) / b_bin;
                            bF = (uint32_t)b_lo;
                            nbm = (uint32_t)((b_hi < b_n ? b_hi : (uint64_t)b_n - 1u) - b_lo) + 1u;
                        }
                    }
                }
                const bool reparse = wg_any(cnt > kBlkLaneCap);
                if (nbm != 0u) {
                    // an entry: u64 sum | u64 sum of squares | i32 min | i32 max
                    constexpr uint32_t kEntry = 6u;
                    const uint32_t tcap = reparse ? kObufWords / kEntry : (kWSize - 4u) / kEntry;
                    uint32_t *const tab = reparse ? stage : W + 4u;  // (both 8-byte aligned; W[0 .. 3] are no part of an image)
                    const uint32_t regime = nbm == 1u ? 1u : (nbm <= tcap ? 2u : 3u);
                    if (regime == 2u) {
                        for (uint32_t e = tid; e < nbm; e += (uint32_t)NT) {
                            uint32_t *t = tab + kEntry * e;
                            t[0] = t[1] = t[2] = t[3] = 0u;
                            t[4] = 32767u;
                            t[5] = (uint32_t)-32768;
                        }
                        blk_barrier();
                    }
                    // one bin: what the lane keeps of it
                    int64_t r_s = 0;
                    uint64_t r_q = 0;
                    int32_t r_mn = 32767, r_mx = -32768;
                    auto merge = [&](unsigned long long *row, int64_t ps, uint64_t pq, int32_t pmn, int32_t pmx) __attribute__((always_inline)) {
                        __hip_atomic_fetch_add(row, (unsigned long long)ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_add(row + 1, (unsigned long long)pq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_min(reinterpret_cast<long long *>(row + 2), (long long)pmn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_max(reinterpret_cast<long long *>(row + 3), (long long)pmx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    };
                    // my partial row of bin b (bF <= b < bF + nbm: my samples are the block's)
                    auto emit = [&](uint32_t b, int32_t ps, uint64_t pq, int32_t pmn, int32_t pmx) __attribute__((always_inline)) {
                        const uint32_t e = b - bF;
                        if (e >= nbm) return;  // (cannot happen: no store leaves the bins the block meets)
                        if (regime == 1u) {
                            r_s += ps;
                            r_q += pq;
                            r_mn = pmn < r_mn ? pmn : r_mn;
                            r_mx = pmx > r_mx ? pmx : r_mx;
                        } else if (regime == 2u) {
                            uint32_t *t = tab + kEntry * e;
                            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(t), (unsigned long long)(int64_t)ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(t + 2), (unsigned long long)pq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_min(reinterpret_cast<int32_t *>(t + 4), pmn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_max(reinterpret_cast<int32_t *>(t + 5), pmx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        } else {
                            merge(b_rows + (uint64_t)b * (uint64_t)DRX_BIN_COLS, (int64_t)ps, pq, pmn, pmx);
                        }
                    };
                    // the walk: the current stretch's sums and extremes (a lane holds at most 32 kSegW codes: the sum is below 2^25
                    // in magnitude), handed on at every border and behind my last sample
                    BinCursor bc = {kNoBorder, 0u, false};
                    if (todo != 0u) (void)bins_begin(bc, b_a, b_bin, b_n, len, i0);
                    int32_t s32 = 0, mn = 32767, mx = -32768;
                    uint64_t sq = 0;
                    auto take = [&](uint32_t c, uint32_t rel) __attribute__((always_inline)) {  // my sample c, `rel` behind the base
                        const int32_t v = (int32_t)(int16_t)(uint16_t)(base16 + rel);
                        if (i0 + c == bc.nb) {
                            if (bc.live) emit(bc.cur, s32, sq, mn, mx);
                            bins_border(bc, b_bin, b_n, len);
                            s32 = 0;
                            sq = 0;
                            mn = 32767;
                            mx = -32768;
                        }
                        s32 += v;
                        sq += (uint64_t)(uint32_t)(v * v);
                        mn = v < mn ? v : mn;
                        mx = v > mx ? v : mx;
                    };
                    if (!reparse) {
                        // the common case: every lane's running sums are complete in its share of the staging buffer, two to a dword
                        const uint32_t wmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(todo));
                        for (uint32_t i = 0; 2u * i < wmax; ++i) {
                            const uint32_t d = my_stage[i];
                            if (2u * i < todo) take(2u * i, d & 0xffffu);
                            if (2u * i + 1u < todo) take(2u * i + 1u, d >> 16);
                        }
                    } else {
                        // some lane holds more codes than its share: every lane parses its codes again from f, with values
                        uint32_t Qr = C - (todo ? f : B0), rs = 0;
                        for (uint32_t c = 0; c < todo; ++c) {
                            const BlkPair p = blk_pair<true>(W, k, Qr);
                            rs += unzigzag(p.z1);
                            Qr += p.nu1;
                            take(c, rs);
                        }
                    }
                    if (todo != 0u && bc.live) emit(bc.cur, s32, sq, mn, mx);
                    if (regime == 1u) {
                        uint64_t u_s = (uint64_t)r_s;
#pragma unroll
                        for (int d = 32; d > 0; d >>= 1) {
                            const int32_t omn = __shfl_xor(r_mn, d), omx = __shfl_xor(r_mx, d);
                            r_mn = omn < r_mn ? omn : r_mn;
                            r_mx = omx > r_mx ? omx : r_mx;
                            u_s += (uint64_t)__shfl_xor((unsigned long long)u_s, d);
                            r_q += (uint64_t)__shfl_xor((unsigned long long)r_q, d);
                        }
                        // ... across the wavefronts through s_e (its last reader is barriers back), then four atomics per block
                        uint64_t *const s_red = reinterpret_cast<uint64_t *>(s_e);  // [NW][3]; 24 NW bytes of s_e's 4 NT
                        if (lane == 0) {
                            uint64_t *r = s_red + 3 * wv;
                            r[0] = u_s;
                            r[1] = r_q;
                            r[2] = ((uint64_t)(uint32_t)r_mn << 32) | (uint64_t)(uint32_t)r_mx;
                        }
                        blk_barrier();
                        if (tid == 0) {
#pragma unroll
                            for (int w = 1; w < NW; ++w) {
                                const uint64_t *r = s_red + 3 * w;
                                const int32_t omn = (int32_t)(uint32_t)(r[2] >> 32), omx = (int32_t)(uint32_t)r[2];
                                u_s += r[0];
                                r_q += r[1];
                                r_mn = omn < r_mn ? omn : r_mn;
                                r_mx = omx > r_mx ? omx : r_mx;
                            }
                            merge(b_rows + (uint64_t)bF * (uint64_t)DRX_BIN_COLS, (int64_t)u_s, r_q, r_mn, r_mx);
                        }
                    } else if (regime == 2u) {
                        blk_barrier();
                        for (uint32_t e = tid; e < nbm; e += (uint32_t)NT) {
                            const uint32_t *t = tab + kEntry * e;
                            const uint64_t ts = (uint64_t)t[0] | ((uint64_t)t[1] << 32), tq = (uint64_t)t[2] | ((uint64_t)t[3] << 32);
                            merge(b_rows + (uint64_t)(bF + e) * (uint64_t)DRX_BIN_COLS, (int64_t)ts, tq, (int32_t)t[4], (int32_t)t[5]);
                        }
                    }
                }
