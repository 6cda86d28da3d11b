#!/usr/bin/env python3
"""Selected-waveform decode against what a user did without it: `plan.decode` of the whole batch followed by
`y.view(-1, L).index_select(0, idx)`.  Both are timed with HIP events around the call, in the same process and alternating,
so that the yardstick is taken in the same run; median of --calls calls behind --warmup.

  headline   500 chunks of 2000 x 7000 (Gaussian, sigma = 10, m = 8, seeded): selections of S waveforms drawn uniformly
             without replacement, S = 1, 64, 4096, 65 536, 1 000 000, and 4096 waveforms confined to 4 chunks; with and
             without the encoder's side-band
  noptrex, long-40   one line each: few long waveforms (reported, not gated)

usage: select_bench.py [--chunks 500] [--sizes 1,64,...] [--calls 20] [--warmup 5] [--only headline|noptrex|long-40]
A line is "ok" when the select call beats the yardstick by more than the yardstick's own min-max spread in this run.
Behind `rocprofv3 --kernel-trace --stats --` (no counters), `--only headline --sizes 4096 --no-yardstick` gives
k_decode_select's kernel time."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import deltarice_amd as dr  # noqa: E402
from workload import geometry  # noqa: E402


def samples(ctx, total, sigma=10.0, seed=5):
    g = torch.Generator(device=ctx.device).manual_seed(seed)
    x = torch.empty(total, dtype=torch.int16, device=ctx.device)
    slab = 1 << 28
    for s0 in range(0, total, slab):
        n = min(slab, total - s0)
        x[s0:s0 + n] = (torch.randn(n, device=ctx.device, generator=g) * sigma).to(torch.int16)
    return x


class Case:
    def __init__(self, ctx, n_chunks, chunk_samples, L, m=8):
        self.ctx, self.L = ctx, L
        self.x = samples(ctx, n_chunks * chunk_samples)
        self.plan = ctx.plan_uniform(n_chunks, chunk_samples, (m, L))
        torch.cuda.synchronize()
        self.enc = self.plan.encode(self.x)
        self.table = self.plan.wave_words_device()
        self.y = torch.empty_like(self.x)
        self.waves_per_chunk = chunk_samples // L

    def timed(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        self.plan.finish()
        return a.elapsed_time(b), r

    def yardstick(self, idx_dev):
        def fn():
            y = self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, self.y, in_words=self.enc.total_words)
            return y.view(-1, self.L).index_select(0, idx_dev)
        return self.timed(fn)

    def select(self, sel, sideband):
        return self.timed(lambda: self.plan.decode_select_async(self.enc.words, self.enc.chunk_word_off, sel,
                                                                in_words=self.enc.total_words,
                                                                wave_words=self.table if sideband else None))

    def line(self, label, sel, calls, warmup, yardstick=True):
        idx_dev = torch.from_numpy(sel.astype(np.int64)).to(self.ctx.device)
        ty, ts, tb = [], [], []
        ok = True
        for i in range(warmup + calls):
            if yardstick:
                t, want = self.yardstick(idx_dev)
                ty.append(t)
            t, got = self.select(sel, False)
            ts.append(t)
            t, got_b = self.select(sel, True)
            tb.append(t)
            if yardstick and i == 0:
                ok = torch.equal(got, want) and torch.equal(got_b, want)
        ts, tb = np.array(ts[warmup:]), np.array(tb[warmup:])
        # where a select call's time goes: the walk and the kernel, from the plan's own events
        self.ctx.set_option("profile", 1)
        self.select(sel, False)
        walk, kern = self.plan.last_timings()[:2]
        self.ctx.set_option("profile", 0)
        touched = np.unique(sel // self.waves_per_chunk).size
        if not yardstick:
            print(f"{label:24s} {sel.size:8d} {touched:6d}  select {np.median(ts):8.3f}  side-band {np.median(tb):8.3f}  "
                  f"(walk {walk:.3f} kernel {kern:.3f})", flush=True)
            return
        ty = np.array(ty[warmup:])
        spread = ty.max() - ty.min()
        verdict = "ok" if max(np.median(ts), np.median(tb)) < np.median(ty) - spread else "NOT FASTER"
        print(f"{label:24s} {sel.size:8d} {touched:6d}  yardstick {np.median(ty):8.3f} [{ty.min():.3f} .. {ty.max():.3f}]  "
              f"select {np.median(ts):8.3f} [{ts.min():.3f} .. {ts.max():.3f}]  side-band {np.median(tb):8.3f}  "
              f"(walk {walk:.3f} kernel {kern:.3f})  x{np.median(ty) / np.median(ts):.1f}  {verdict}{'' if ok else '  MISMATCH'}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--sizes", default="1,64,4096,65536,1000000")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    ctx = dr.Context(0)
    rng = np.random.default_rng(2025)
    print(f"{'case':24s} {'S':>8s} {'chunks':>6s}  times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")
    if a.only in ("", "headline"):
        c = Case(ctx, a.chunks, 2000 * 7000, 7000)
        W = a.chunks * 2000
        for S in [int(s) for s in a.sizes.split(",")]:
            S = min(S, W)
            c.line("headline", rng.choice(W, S, replace=False), a.calls, a.warmup, not a.no_yardstick)
        if not a.no_yardstick:
            four = rng.choice(a.chunks, 4, replace=False)
            sel = (four[:, None] * 2000 + np.arange(2000)[None, :]).reshape(-1)
            c.line("headline, 4 chunks", rng.choice(sel, min(4096, sel.size), replace=False), a.calls, a.warmup)
        del c
    for name in ("noptrex", "long-40"):
        if a.only not in ("", name):
            continue
        if name == "noptrex":
            Ns, Ls = geometry("noptrex")
        else:
            Ns, Ls = [32 * 50000] * 40, [50000] * 40
        c = Case(ctx, len(Ns), Ns[0], Ls[0])
        W = len(Ns) * (Ns[0] // Ls[0])
        c.line(name, rng.choice(W, 64, replace=False), a.calls, a.warmup, not a.no_yardstick)
        del c


if __name__ == "__main__":
    main()
