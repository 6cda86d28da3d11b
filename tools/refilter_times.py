#!/usr/bin/env python3
"""Re-coding an encoded batch under another prediction filter (`plan.refilter`) against the route it replaces: `plan.decode` of
the whole batch, `plan.set_filter(new)`, `plan.encode`, `plan.set_filter(old)`.  The batch: --chunks chunks of 2000 x 7000
Gaussian samples, sigma = 10 (seeded), written with the delta filter at m = 8; the target: taps [1,-1,1,-1] at the same m.

Times are HIP events: the library's own (`ctx.set_option("profile", 1)`, `plan.last_timings()`: a call's kernels from its first
launch to its last) for refilter, decode and encode, and a pair of events around each whole route on the context's stream,
which for the old route includes the two `set_filter` calls (each waits for the stream and uploads the taps).  Both routes run
in one process, alternating; median [min .. max] of --calls calls behind --warmup.  Peak device memory is torch's peak
allocation during one call of a route that allocates its own buffers, above what the encoded source occupies.

usage: refilter_times.py [--chunks 500] [--calls 10] [--warmup 3] [--serial]
--serial adds the serial kernels on the same pair (DRX_DBG_REFILTER_SERIAL), one call."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import deltarice_amd as dr  # noqa: E402
from wave_stats_bench import samples  # noqa: E402

FIR4 = (1, -1, 1, -1)


def med(t):
    t = np.array(t)
    return f"{np.median(t):8.3f} [{t.min():.3f} .. {t.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--serial", action="store_true")
    a = ap.parse_args()
    ctx = dr.Context(0)
    dev = ctx.device
    N, L, m = 2000 * 7000, 7000, 8
    plan = ctx.plan_uniform(a.chunks, N, (m, L))
    x = samples(ctx, a.chunks * N, 10.0)
    torch.cuda.synchronize()
    enc = plan.encode(x)
    del x
    torch.cuda.empty_cache()
    est = plan.estimate_words_refiltered(enc, FIR4)
    total2 = int(est[3])
    print(f"{plan.total_waves} waveforms of {L}, {plan.total_samples / 1e9:.2f} GS; stream {enc.total_words * 4 / 1e9:.2f} GB (delta, m = {m}) -> "
          f"{total2 * 4 / 1e9:.2f} GB ({list(FIR4)}, m = {m}; smallest at m = {1 << int(np.argmin(est))}: {int(est.min()) * 4 / 1e9:.2f} GB)")
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")

    def whole(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ctx.stream):
            e0.record()
            r = fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def refilter(out):
        plan.refilter_async(enc.words, enc.chunk_word_off, FIR4, m, out, enc.total_words)
        plan.finish()
        return plan.last_timings()

    def old_route(y, out):
        plan.decode_async(enc.words, enc.chunk_word_off, y, in_words=enc.total_words)
        plan.finish()
        t_dec = plan.last_timings()[3]
        plan.set_filter(FIR4)
        plan.encode_async(y, out_words=out)
        n = plan.finish()
        t_enc = plan.last_timings()[3]
        plan.set_filter(None)
        return t_dec, t_enc, n

    ctx.set_option("profile", 1)
    out_r = torch.empty(total2, dtype=torch.int32, device=dev)
    out_o = torch.empty(total2, dtype=torch.int32, device=dev)
    y = torch.empty(plan.total_samples, dtype=torch.int16, device=dev)
    tr, tr_whole, split, to_whole, td, te = [], [], [], [], [], []
    for i in range(a.warmup + a.calls):
        w, ms = whole(lambda: refilter(out_r))
        tr.append(ms[3]); tr_whole.append(w); split.append(ms[:3])
        w, (t_dec, t_enc, n) = whole(lambda: old_route(y, out_o))
        to_whole.append(w); td.append(t_dec); te.append(t_enc)
        if i == 0:
            assert n == total2 and torch.equal(out_r, out_o), "the two routes differ"
    k = a.warmup
    walk, sizes, pack = np.median(np.array(split[k:]), axis=0)
    print(f"refilter              kernels {med(tr[k:])} (walk {walk:.3f} sizes+scan+offsets {sizes:.3f} pack {pack:.3f})  whole call {med(tr_whole[k:])}")
    print(f"decode, set_filter, encode, set_filter"
          f"\n                      kernels {med(np.array(td[k:]) + np.array(te[k:]))} (decode {med(td[k:])} encode {med(te[k:])})  whole route {med(to_whole[k:])}")
    print(f"refilter / old route: kernels x{np.median(tr[k:]) / np.median(np.array(td[k:]) + np.array(te[k:])):.2f}, whole x{np.median(tr_whole[k:]) / np.median(to_whole[k:]):.2f}")
    if a.serial:
        ctx.set_option("debug_flags", dr.DBG_REFILTER_SERIAL)
        w, ms = whole(lambda: refilter(out_r))
        ctx.set_option("debug_flags", 0)
        assert torch.equal(out_r, out_o), "the serial kernels differ"
        print(f"refilter, serial kernels (one call)  kernels {ms[3]:.3f} (walk {ms[0]:.3f} sizes+scan+offsets {ms[1]:.3f} pack {ms[2]:.3f})")
    del out_r, out_o, y
    torch.cuda.empty_cache()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    p_r = peak(lambda: refilter(torch.empty(total2, dtype=torch.int32, device=dev)))
    p_o = peak(lambda: old_route(torch.empty(plan.total_samples, dtype=torch.int16, device=dev), torch.empty(total2, dtype=torch.int32, device=dev)))
    print(f"peak device memory above the source: refilter {p_r / 1e9:.2f} GB, old route {p_o / 1e9:.2f} GB")
    ctx.set_option("profile", 0)
    plan.close()


if __name__ == "__main__":
    main()
