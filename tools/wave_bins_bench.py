#!/usr/bin/env python3
"""Binned statistics from the encoded stream (`plan.wave_bins`) against what a user did without it: `plan.decode` of the whole
batch, then torch reductions over the decoded samples that give the same [W, n_bins, 4] tensor.  Everything is timed with HIP
events around the call, in one process and alternating, so that the yardsticks are taken in the same run; median [min .. max]
of --calls calls behind --warmup.  Run one shape per process (--only NAME).

  headline     500 chunks of 2000 x 7000, m = 8, Gaussian sigma = 10 (seeded), three binnings:
                 whole      bin = 7000, one bin: the whole waveform
                 bin500     bin = 500 from offset 0, 14 bins
                 gates      bin = 250, n_bins = 8, start = stats[:, STAT_ARGMAX], offset = -500: per-waveform origins
               each against plan.wave_stats, plan.decode alone, and plan.decode + the torch reductions
  noptrex      2048 waveforms of 500 000 samples, 1000 bins across the trace
  nedm         256 chunks of 32 x 81 920, 1000 bins across the trace
  long25       25 chunks of ONE 14 M-sample waveform, 1000 bins across the trace
               the long shapes against plan.decode alone and plan.wave_stats (its block form), under --impl 0 (a lane per
               waveform) and --impl 1 (the context option "bins_impl": the block form); the form that ran and the waveforms
               its blocks listed for the lane kernel are printed beside each time.  --bin N: bins of N samples across the trace
               instead of 1000 bins

Peak bytes: torch's peak allocation during one call that allocates its own results, above what the encoded batch occupies.

usage: wave_bins_bench.py --only NAME [--impl {0,1}] [--bin N] [--chunks 500] [--calls 20] [--warmup 5]"""
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
    def __init__(self, ctx, Ns, Ls, sigma, m=8):
        self.ctx, self.Ns, self.Ls = ctx, Ns, Ls
        x = samples(ctx, sum(Ns), sigma)
        self.plan = ctx.plan_uniform(len(Ns), Ns[0], (m, Ls[0]) if Ls[0] else (m,))
        torch.cuda.synchronize()
        self.enc = self.plan.encode(x)
        del x
        self.L = self.plan.longest_wave()
        self.y = torch.empty(self.plan.total_samples, dtype=torch.int16, device=ctx.device)

    def timed(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        self.plan.finish()
        return a.elapsed_time(b), r

    def peak(self, fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.cuda.stream(self.ctx.stream):
            r = fn()
        self.plan.finish()
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated() - base

    def decode(self, out=None):
        return self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, self.y if out is None else out, in_words=self.enc.total_words)

    def stats(self):
        return self.plan.wave_stats_async(self.enc.words, self.enc.chunk_word_off, 0, in_words=self.enc.total_words)

    def bins(self, bin, n_bins, start, offset):
        return self.plan.wave_bins_async(self.enc.words, self.enc.chunk_word_off, bin, n_bins, start, offset, in_words=self.enc.total_words)

    def reduce(self, y, bin, n_bins, start, offset):
        """The same tensor by torch reductions over decoded samples, in slabs of 2^15 waveforms (uniform waveforms of L samples)."""
        L, out = self.L, []
        v_all = y.view(-1, L)
        for g0 in range(0, v_all.shape[0], 1 << 15):
            v = v_all[g0:g0 + (1 << 15)]
            if start is None and offset == 0 and L % bin == 0 and n_bins == L // bin:
                w = v.view(v.shape[0], n_bins, bin)
                ok = None
            else:  # per-waveform origins: the samples of every bin gathered, those outside the waveform masked
                a = (start[g0:g0 + v.shape[0]] if start is not None else 0) + offset
                idx = a[:, None] + torch.arange(n_bins * bin, device=y.device)[None, :]
                ok = ((idx >= 0) & (idx < L)).view(v.shape[0], n_bins, bin)
                w = torch.gather(v, 1, idx.clamp(0, L - 1)).view(v.shape[0], n_bins, bin)
            w32 = w.to(torch.int32)
            if ok is None:
                out.append(torch.stack([w.sum(dim=2, dtype=torch.int64), (w32 * w32).sum(dim=2, dtype=torch.int64), w.amin(dim=2).long(),
                                        w.amax(dim=2).long()], dim=2))
            else:
                z = torch.where(ok, w32, 0)
                out.append(torch.stack([z.sum(dim=2, dtype=torch.int64), (z * z).sum(dim=2, dtype=torch.int64),
                                        torch.where(ok, w32, 32767).amin(dim=2).long(), torch.where(ok, w32, -32768).amax(dim=2).long()], dim=2))
        return torch.cat(out)

    def line(self, label, calls, warmup, bin, n_bins, start=None, offset=0, reduces=True, with_stats=True):
        td, tr, ts, tb = [], [], [], []
        match = True
        for i in range(warmup + calls):
            td.append(self.timed(self.decode)[0])
            if with_stats:
                ts.append(self.timed(self.stats)[0])
            t, got = self.timed(lambda: self.bins(bin, n_bins, start, offset))
            tb.append(t)
            if reduces:
                t, want = self.timed(lambda: self.reduce(self.decode(), bin, n_bins, start, offset))
                tr.append(t)
                if i == 0:
                    match = torch.equal(got, want)
                del want
            del got
        form = {0: "?", 1: "lanes", 2: "blocks"}[self.plan.last_bins_form() & 3] + f", listed {self.plan.last_bins_listed()}"
        self.ctx.set_option("profile", 1)
        self.timed(lambda: self.bins(bin, n_bins, start, offset))
        walk, kern = self.plan.last_timings()[:2]
        self.ctx.set_option("profile", 0)
        p_b = self.peak(lambda: self.bins(bin, n_bins, start, offset))

        def fmt(t):
            t = np.array(t[warmup:])
            return f"{np.median(t):9.3f} [{t.min():.3f} .. {t.max():.3f}]"

        med = lambda t: float(np.median(np.array(t[warmup:])))  # noqa: E731
        s = (f"{label:18s} {self.plan.total_waves:8d} waveforms {self.plan.total_samples / 1e9:6.2f} GS  bin {bin} x {n_bins}  "
             f"bins({form}) {fmt(tb)} (walk {walk:.3f} kernel {kern:.3f})  decode {fmt(td)}  x{med(tb) / med(td):.2f} of decode")
        if with_stats:
            s += f"  wave_stats {fmt(ts)}  x{med(tb) / med(ts):.2f} of wave_stats"
        if reduces:
            y_keep, self.y = self.y, None
            p_r = self.peak(lambda: self.reduce(self.decode(torch.empty(self.plan.total_samples, dtype=torch.int16, device=self.ctx.device)),
                                                bin, n_bins, start, offset))
            self.y = y_keep
            s += (f"  decode+torch {fmt(tr)}  x{med(tr) / med(tb):.1f} of bins  peak {p_b / 1e6:.1f} MB against {p_r / 1e9:.2f} GB"
                  f"{'' if match else '  MISMATCH'}")
        else:
            s += f"  peak {p_b / 1e6:.1f} MB"
        print(s, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", required=True)
    ap.add_argument("--impl", type=int, choices=(0, 1), default=0, help='the context option "bins_impl"')
    ap.add_argument("--bin", type=int, default=0, help="long shapes: bins of this many samples instead of 1000 bins")
    a = ap.parse_args()
    ctx = dr.Context(0)
    ctx.set_option("bins_impl", a.impl)
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")
    if a.only == "headline":
        c = Case(ctx, [2000 * 7000] * a.chunks, [7000] * a.chunks, 10.0)
        c.line("headline whole", a.calls, a.warmup, 7000, 1)
        c.line("headline bin500", a.calls, a.warmup, 500, 14)
        stats = c.plan.wave_stats(c.enc)
        c.line("headline gates", a.calls, a.warmup, 250, 8, stats[:, dr.STAT_ARGMAX], -500)
    else:
        Ns, Ls = geometry(a.only)
        c = Case(ctx, list(Ns), list(Ls), 10.0)
        bin = a.bin if a.bin else -(-c.L // 1000)
        c.line(f"{a.only} impl {a.impl}", a.calls, a.warmup, bin, -(-c.L // bin), reduces=False, with_stats=True)
    c.plan.close()


if __name__ == "__main__":
    main()
