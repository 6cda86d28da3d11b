// drx_blocks_trc.inc -- phase 2 of k_trc_blocks (drx_transcode_blocks.hip), included by drx_blocks_body.inc inside its
// `if constexpr (TRANSCODE)`: the block's residuals sized (the sizes launch) or re-coded (the pack launch) at the RiceParameter
// 2^ta.k2.  A lane's residuals are the `todo` codes from f on; the sizes launch reads them from the int16 pairs phase 1 staged,
// or -- where some lane holds more codes than its share of the staging buffer -- from a second parse, as the STATS form does.
                constexpr bool kAllK = decltype(ta)::kAllK;
                constexpr int NK = kAllK ? 16 : 1;
                const uint32_t k2 = ta.k2;
                uint32_t nbits[NK];  // my codes' bits at the new parameter(s): at most 608 codes of 25 bits
#pragma unroll
                for (int j = 0; j < NK; ++j) nbits[j] = 0u;
                auto add = [&](uint32_t z) __attribute__((always_inline)) {
#pragma unroll
                    for (int j = 0; j < NK; ++j) nbits[j] += trc_code_bits(z, kAllK ? (uint32_t)j : k2);
                };
                if (!wg_any(cnt > kBlkLaneCap)) {
                    for (uint32_t i = 0; 2u * i < todo; ++i) {
                        const uint32_t d = my_stage[i];
                        add(trc_canon16(d & 0xffffu));
                        if (2u * i + 1u < todo) add(trc_canon16(d >> 16));
                    }
                } else {
                    uint32_t Qr = C - (todo ? f : B0);
                    for (uint32_t c = 0; c < todo; ++c) {
                        const BlkPair p = blk_pair<true>(W, k, Qr);
                        add(trc_canon16(unzigzag(p.z1)));
                        Qr += p.nu1;
                    }
                }
                if (!t_pack) {
                    // ---- the sizes launch: the block's bits, to its slot (and everything its second run starts from) or, sixteen
                    // of them, to the waveform's accumulators.  (s_e's last reader is a barrier back.)
                    if constexpr (kAllK) {
#pragma unroll
                        for (int j = 0; j < NK; ++j) {
                            const uint64_t all = wave_sum_u64((uint64_t)nbits[j]);
                            if (lane == 0 && all != 0u)
                                __hip_atomic_fetch_add(ta.acc16 + 16u * g + (uint32_t)j, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    } else {
                        const uint32_t all = (uint32_t)wave_sum_u64((uint64_t)nbits[0]);
                        if (lane == 0) s_e[wv] = all;
                        blk_barrier();
                        if (tid == 0) {
                            uint32_t bits = 0;
#pragma unroll
                            for (int w = 0; w < NW; ++w) bits += s_e[w];
                            uint32_t *sl = ta.slots + (uint64_t)sidx * kTrcSlotWords;
                            sl[0] = bits; sl[1] = 0u; sl[2] = bits; sl[3] = f - B0; sl[4] = blk_first; sl[5] = blk_count;
                        }
                    }
                    if (tid == 0 && blk + 1u == n_blocks) ta.n_blocks[g] = n_blocks;
                } else if constexpr (!kAllK) {
                    // ---- the pack launch: a scan of the lanes' bits says where a lane's first code goes; the block's words are put
                    // together in the staging buffer -- no residual is read from it from here on: every lane parses its codes again
                    // from f -- and drained in passes of kOB words (a block is a fixed number of INPUT bits: re-coded at a small
                    // parameter it may be many times that).  A lane ORs whole words into the cleared buffer (ds_or_b32), so the words
                    // two lanes share need no other care.  Global words: the block's first and last word may be shared with its
                    // neighbours (a block of a few samples may lie inside one word with several others) and are OR-ed into words
                    // that k_trc_blocks_layout cleared; every other word is stored once, by 16-byte stores where four lie inside.
                    const uint32_t *sl = ta.slots + (uint64_t)sidx * kTrcSlotWords;
                    const uint64_t boff64 = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
                    const uint32_t blkbits = sl[2];
                    const uint32_t incl_b = wave_incl_scan_dpp(nbits[0]);
                    if (lane == 63) s_tot[0][wv] = incl_b;
                    blk_barrier();  // (also: every lane has read its staged residuals)
                    uint32_t pre_b = 0;
#pragma unroll
                    for (int i = 0; i < NW; ++i) pre_b += i < wv ? s_tot[0][i] : 0u;
                    if (blkbits != 0u) {
                        constexpr uint32_t kOB = kObufWords & ~3u;
                        const uint64_t pos = ta.out_chunk_off[r.chunk] + ta.new_rel[g];  // the waveform's header word
                        const uint64_t P = 32u * (pos + 1u) + boff64;                    // my block's first bit in the result
                        const uint64_t wlo = P >> 5, whi = (P + blkbits + 31u) >> 5;      // its words
                        const uint32_t lead = (uint32_t)((((uintptr_t)ta.outw >> 2) + wlo) & 3u);  // buffer word 0 is 16-byte aligned in the result
                        uint32_t *const gout = ta.outw + wlo - lead;  // buffer word i of pass 0 (never dereferenced in front of wlo)
                        const uint32_t nwords = lead + (uint32_t)(whi - wlo);
                        const uint32_t lo_plain = lead + ((P & 31u) ? 1u : 0u), hi_plain = nwords - (((P + blkbits) & 31u) ? 1u : 0u);
                        const uint32_t sb = 32u * lead + (uint32_t)(P & 31u) + (pre_b + incl_b - nbits[0]);
                        uint32_t wpos = sb >> 5, nacc = sb & 31u, c = 0, Qr = C - (todo ? f : B0);
                        uint64_t acc = 0;
                        bool fin = todo == 0u;
                        for (uint32_t pass_lo = 0; pass_lo < nwords; pass_lo += kOB) {
                            const uint32_t npass = nwords - pass_lo < kOB ? nwords - pass_lo : kOB, win_end = pass_lo + kOB;
                            for (uint32_t i = tid; 4u * i < npass; i += (uint32_t)NT) *reinterpret_cast<uint4 *>(stage + 4u * i) = make_uint4(0u, 0u, 0u, 0u);
                            blk_barrier();
                            auto put = [&](uint32_t zr) __attribute__((always_inline)) {  // rice_code()'s code and length, from the zig-zag value
                                const uint32_t z = trc_canon16(unzigzag(zr));
                                const uint32_t q = z >> k2;
                                const bool esc = q >= 8u;
                                const uint32_t nb = esc ? 25u : q + 1u + k2;
                                const uint32_t code = esc ? (0x10000u | z) : ((1u << k2) | (z & ((1u << k2) - 1u)));
                                acc = (acc << nb) | code;
                                nacc += nb;
                                if (nacc >= 32u) {
                                    nacc -= 32u;
                                    __hip_atomic_fetch_or(stage + (wpos - pass_lo), (uint32_t)(acc >> nacc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                    ++wpos;
                                }
                            };
                            while (!fin && wpos < win_end) {
                                if (c < todo) {
                                    const BlkPair p = blk_pair<true>(W, k, Qr);
                                    put(p.z1);
                                    ++c;
                                    Qr += p.nu1;
                                    if (c < todo && wpos < win_end) {
                                        put(p.z2);
                                        ++c;
                                        Qr += p.nu2;
                                    }
                                } else {  // what is left of my last code: left aligned (the waveform's last word: zero padded, :237-241)
                                    if (nacc)
                                        __hip_atomic_fetch_or(stage + (wpos - pass_lo), (uint32_t)(acc << (32u - nacc)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                    fin = true;
                                }
                            }
                            blk_barrier();
                            for (uint32_t i = tid; 4u * i < npass; i += (uint32_t)NT) {
                                const uint32_t i0 = pass_lo + 4u * i;
                                const uint4 v = *reinterpret_cast<const uint4 *>(stage + 4u * i);
                                if (i0 >= lo_plain && i0 + 4u <= hi_plain) {
                                    *(g_uint4 *)(gout + i0) = (u32x4v){v.x, v.y, v.z, v.w};
                                } else {
                                    const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                                    for (uint32_t j = 0; j < 4u; ++j) {
                                        const uint32_t ix = i0 + j;
                                        if (ix < lead || ix >= nwords) continue;
                                        if (ix >= lo_plain && ix < hi_plain) gout[ix] = vv[j];
                                        else if (vv[j]) atomicOr(gout + ix, vv[j]);
                                    }
                                }
                            }
                            blk_barrier();
                        }
                    }
                }
