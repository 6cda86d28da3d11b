#!/usr/bin/env python3
"""Every pulse of every waveform from the encoded stream (`plan.find_pulses`) against the two calls that bracket it:
`plan.wave_stats` on the same stream, which does the same parse and writes 64 bytes per waveform (the ratio to it is the cost of
the fast reject and the state machine), and `plan.decode` of the whole batch, the first step of the only other route to the same
answer (a run-length search over the decoded samples would follow).  Everything is timed with HIP events around the call, in
one process and alternating, so that the yardsticks are taken in the same run; median [min .. max] of --calls calls behind
--warmup.

  headline        500 chunks of 2000 x 7000, m = 8, Gaussian sigma = 10 (seeded), a pulse of 3000 somewhere in every waveform
  headline-loud   the same with sigma = 400
  short           300 chunks of 8192 x 512
  noptrex         2048 waveforms of 500 000 samples  } few long waveforms: the block form of drx_pulses_blocks.hip
  nedm            8192 waveforms of 81 920 samples   } (before it existed: a lane each)
  long25          25 waveforms of 14 M samples       }

and for each batch three cells: `5sigma` = threshold at 5 sigma, rare pulses, max_pulses 4; `2sigma` = threshold at 2 sigma,
several pulses per waveform, max_pulses 8; `count` = the counting form (max_pulses 0) at 2 sigma.  Two more for the block form
(--cells ...,cap,fallback; sigma = 10 batches): `cap` = threshold 2000, the one planted pulse per waveform, max_pulses 32 -- above
what a block stages; `fallback` = threshold 1000 with max_pulses 32, where waveform 0's twenty pulses of 1500 within 2000
samples make one block need more records than it staged: the blocks run a second time over that waveform.  Every line
says which form the call took (drx_plan_last_pulses_form; `-` on a library that has no such query).

usage: find_pulses_bench.py [--chunks 500] [--calls 20] [--warmup 5] [--only NAME[,NAME]] [--cells 5sigma,2sigma,count] [--no-yardstick]
A line is "ok" when the call takes less time than `plan.decode` alone by more than that decode's min-to-max spread over the
alternating runs, and NOT FASTER THAN DECODE otherwise; MISMATCH: the counts differ from the rising edges over the threshold in
the decoded samples (checked once per line, at the size that is timed)."""
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
from workload import geometry  # noqa: E402


class Case:
    def __init__(self, ctx, n_chunks, N, L, sigma, m=8):
        opts = (m, L) if L else (m,)  # (L = 0: the whole chunk is one waveform)
        L = L or N
        self.ctx, self.L, self.sigma = ctx, L, sigma
        x = samples(ctx, n_chunks * N, sigma)
        W = n_chunks * (N // L)
        g = torch.Generator(device=ctx.device).manual_seed(7)
        at = torch.randint(0, L, (W,), device=ctx.device, generator=g) + torch.arange(W, device=ctx.device) * L
        x[at] = 3000  # a pulse in every waveform
        if L >= 50000 and sigma < 100:  # the long shapes' `fallback` cell: twenty pulses of 1500 close together in waveform 0
            x[torch.arange(1000, 3000, 100, device=ctx.device)] = 1500
        self.plan = ctx.plan_uniform(n_chunks, N, opts)
        torch.cuda.synchronize()
        self.enc = self.plan.encode(x)
        del x, at
        self.W = self.plan.total_waves
        self.y = torch.empty(self.plan.total_samples, dtype=torch.int16, device=ctx.device)
        self.rows = torch.empty((self.W, dr.STAT_COLS), dtype=torch.int64, device=ctx.device)
        self.count = torch.empty(self.W, dtype=torch.int32, device=ctx.device)

    def timed(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        self.plan.finish()
        return a.elapsed_time(b), r

    def decode(self):
        return self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, self.y, in_words=self.enc.total_words)

    def stats(self):
        return self.plan.wave_stats_async(self.enc.words, self.enc.chunk_word_off, out=self.rows, in_words=self.enc.total_words)

    def pulses(self, thr, max_pulses, out):
        return self.plan.find_pulses_async(self.enc.words, self.enc.chunk_word_off, thr, 1, 1, max_pulses, count=self.count, out=out,
                                           in_words=self.enc.total_words)

    def counts_from_samples(self, thr):
        """The counts the other route gives (min_width 1): rising edges over thr in the decoded samples, slab by slab."""
        v = self.y.view(self.W, self.L)
        n = torch.empty(self.W, dtype=torch.int32, device=v.device)
        rows = max(1, (1 << 27) // self.L)
        for r0 in range(0, self.W, rows):
            over = v[r0:r0 + rows] > thr
            n[r0:r0 + rows] = (over[:, 0].to(torch.int32) + (over[:, 1:] & ~over[:, :-1]).sum(dim=1, dtype=torch.int32))
        return n

    def line(self, label, cname, thr, max_pulses, calls, warmup, yardstick=True):
        out = torch.empty(self.W * max_pulses * dr.PULSE_COLS, dtype=torch.int64, device=self.ctx.device)
        td, ts, tp = [], [], []
        match = True
        for i in range(warmup + calls):
            if yardstick:
                td.append(self.timed(self.decode)[0])
                ts.append(self.timed(self.stats)[0])
            tp.append(self.timed(lambda: self.pulses(thr, max_pulses, out))[0])
            if yardstick and i == 0:  # the counts against the decoded samples, at the size that is timed
                match = torch.equal(self.count, self.counts_from_samples(thr))
        tp = np.array(tp[warmup:])
        self.ctx.set_option("profile", 1)
        self.timed(lambda: self.pulses(thr, max_pulses, out))
        walk, kern = self.plan.last_timings()[:2]
        self.ctx.set_option("profile", 0)
        n = self.count.to(torch.int64)
        form = getattr(self.plan, "last_pulses_form", None)
        form = {None: "-", 1: "lanes", 2: "blocks", 6: "blocks+all"}.get(form() if form else None, "?")
        head = (f"{label:14s} {cname:8s} form {form:6s} threshold {thr:5d} max_pulses {max_pulses} {self.W:8d} waveforms stream {self.enc.total_words * 4 / 1e9:5.2f} GB "
                f"pulses {float(n.sum()) / self.W:7.2f} per waveform, {float((n > max_pulses).sum()) / self.W * 100:5.1f} % of rows overflow, "
                f"records {out.numel() * 8 / 1e9:5.3f} GB  ")
        mine = f"find_pulses {np.median(tp):8.3f} [{tp.min():.3f} .. {tp.max():.3f}] (walk {walk:.3f} kernel {kern:.3f})"
        if not yardstick:
            print(head + mine, flush=True)
            return
        td, ts = np.array(td[warmup:]), np.array(ts[warmup:])
        verdict = "ok" if np.median(tp) < np.median(td) - (td.max() - td.min()) else "NOT FASTER THAN DECODE"
        print(head + f"decode {np.median(td):8.3f} [{td.min():.3f} .. {td.max():.3f}]  wave_stats {np.median(ts):8.3f} [{ts.min():.3f} .. {ts.max():.3f}]  "
              + mine + f"  x{np.median(tp) / np.median(ts):.2f} the time of wave_stats, x{np.median(td) / np.median(tp):.2f} of decode  {verdict}{'' if match else '  MISMATCH'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--cells", default="5sigma,2sigma,count")
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    ctx = dr.Context(0)
    only = [s for s in a.only.split(",") if s]
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")
    nN, nL = geometry("noptrex")
    cases = [
        ("headline", a.chunks, 2000 * 7000, 7000, 10.0),
        ("headline-loud", a.chunks, 2000 * 7000, 7000, 400.0),
        ("short", 300, 8192 * 512, 512, 10.0),
        ("noptrex", len(nN), nN[0], nL[0], 10.0),
        ("nedm", 256, 32 * 81920, 81920, 10.0),
        ("long25", 25, 14_000_000, 0, 10.0),
    ]
    for name, n_chunks, N, L, sigma in cases:
        if only and name not in only:
            continue
        c = Case(ctx, n_chunks, N, L, sigma)
        for cname in a.cells.split(","):
            if cname in ("cap", "fallback"):
                if sigma >= 100 or (L and L < 50000):
                    continue
                thr, max_pulses = {"cap": (2000, 32), "fallback": (1000, 32)}[cname]
            else:
                k, max_pulses = {"5sigma": (5, 4), "2sigma": (2, 8), "count": (2, 0)}[cname]
                thr = int(k * sigma)
            c.line(name, cname, thr, max_pulses, a.calls, a.warmup, not a.no_yardstick)
        c.plan.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
