#!/usr/bin/env python3
"""Per-waveform statistics from the encoded stream (`plan.wave_stats`) against what a user did without it: `plan.decode` of
the whole batch, then torch reductions over the decoded samples that give the same eight columns.  Everything is timed with
HIP events around the call, in one process and alternating, so that the yardsticks are taken in the same run; median of
--calls calls behind --warmup.  Two yardsticks per line: `plan.decode` alone (the floor of any route through decoded
samples), and `plan.decode` + the reductions (in slabs of chunks, so that the squares' temporaries stay small).

  headline        500 chunks of 2000 x 7000, m = 8, Gaussian sigma = 10 (seeded)
  headline-loud   the same with sigma = 400
  short           300 chunks of 8192 x 512
  config5         BASELINE's mixed-length config 5 (ragged: 512 / 2048 / 7000 / 16384)
  noptrex         2048 waveforms of 500 000 samples (few long waveforms: a workgroup per block of a waveform's stream)
  headline-sb     the headline with the encoder's side-band (no header walk)
  nedm            256 chunks of 32 x 81 920 (the block form)
  long25          25 chunks of ONE 14 M-sample waveform, the reference's default options (the block form; --decode-yardstick only:
                  the torch reductions take chunks of whole waveforms of one length)
  stream-quiet    4 chunks of 2100 x 7000: the batch at the decoder's break-even between blocks and lanes, a lane per waveform here

Peak bytes: torch's peak allocation during one call that allocates its own results (the decoded batch and the reductions'
temporaries, or the [W, 8] rows), above what the encoded batch occupies.

usage: wave_stats_bench.py [--chunks 500] [--calls 20] [--warmup 5] [--head 500] [--only NAME[,NAME]] [--no-yardstick]
                           [--decode-yardstick]
--decode-yardstick: `plan.decode` alone, alternating with the stats call, and the stats call's ratio to it (the long shapes:
profiles/wave_stats_blocks_bench.txt compares two builds of the library this way, in fresh processes that alternate).
Every line names the form the call took (drx_plan_last_stats_form) where the library reports it.
A line is "ok" when the stats call takes less time than `plan.decode` alone by more than that decode's min-to-max spread over
the alternating runs.  Behind `rocprofv3 --kernel-trace --stats --` (no counters), `--only headline --no-yardstick` gives
k_wave_stats' own time; behind `rocprofv3 --pmc ... --` (a run of its own) its memory traffic."""
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


def samples(ctx, total, sigma, seed=5):
    g = torch.Generator(device=ctx.device).manual_seed(seed)
    x = torch.empty(total, dtype=torch.int16, device=ctx.device)
    slab = 1 << 28
    for s0 in range(0, total, slab):
        n = min(slab, total - s0)
        x[s0:s0 + n] = (torch.randn(n, device=ctx.device, generator=g) * sigma).to(torch.int16)
    return x


class Case:
    def __init__(self, ctx, Ns, Ls, sigma, head, m=8, reduces=True):
        self.ctx, self.Ns, self.Ls, self.head = ctx, Ns, Ls, head
        x = samples(ctx, sum(Ns), sigma)
        uniform = len(set(Ns)) == 1 and len(set(Ls)) == 1
        self.plan = ctx.plan_uniform(len(Ns), Ns[0], (m, Ls[0]) if Ls[0] else (m,)) if uniform else ctx.plan(Ns, Ls, m)
        torch.cuda.synchronize()
        self.enc = self.plan.encode(x)
        self.table = self.plan.wave_words_device()
        del x
        self.y = torch.empty(self.plan.total_samples, dtype=torch.int16, device=ctx.device)
        self.rows = torch.empty((self.plan.total_waves, dr.STAT_COLS), dtype=torch.int64, device=ctx.device)
        # runs of chunks that share a WaveformLength dividing their sample count, at most ~2^28 samples each: one 2-D view per slab
        self.slabs, at, c = [], 0, 0
        while c < len(Ns):
            c1, n = c, 0
            while c1 < len(Ns) and Ls[c] > 0 and Ls[c1] == Ls[c] and Ns[c1] % Ls[c] == 0 and (n == 0 or n + Ns[c1] <= 1 << 28):
                n += Ns[c1]
                c1 += 1
            if c1 == c:
                if not reduces:
                    break
                raise SystemExit("the yardstick takes chunks of whole waveforms only")
            self.slabs.append((at, n, Ls[c]))
            at, c = at + n, c1

    def timed(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        self.plan.finish()
        return a.elapsed_time(b), r

    def reduce(self, y):
        """The eight columns by torch reductions over decoded samples (argmin / argmax: whichever index torch returns)."""
        out, h = [], self.head
        for at, n, L in self.slabs:
            v = y[at:at + n].view(-1, L)
            mn, amn = v.min(dim=1)
            mx, amx = v.max(dim=1)
            w = v.to(torch.int32)
            hw = w[:, :min(h, L)]
            out.append(torch.stack([mn.long(), amn, mx.long(), amx, v.sum(dim=1, dtype=torch.int64), (w * w).sum(dim=1, dtype=torch.int64),
                                    hw.sum(dim=1, dtype=torch.int64), (hw * hw).sum(dim=1, dtype=torch.int64)], dim=1))
        return torch.cat(out)

    def decode(self, out=None):
        return self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, self.y if out is None else out, in_words=self.enc.total_words)

    def stats(self, sideband, out=None):
        return self.plan.wave_stats_async(self.enc.words, self.enc.chunk_word_off, self.head, self.rows if out is None else out,
                                          self.table if sideband else None, in_words=self.enc.total_words)

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

    def line(self, label, calls, warmup, sideband=False, yardstick=True, decode_only=False):
        td, tr, ts = [], [], []
        match = True
        if decode_only:  # plan.decode and plan.wave_stats alternating, nothing else
            for i in range(warmup + calls):
                td.append(self.timed(self.decode)[0])
                ts.append(self.timed(lambda: self.stats(sideband))[0])
            td, ts = np.array(td[warmup:]), np.array(ts[warmup:])
            form = {0: "?", 1: "lanes", 2: "blocks"}.get(getattr(self.plan, "last_stats_form", lambda: 0)() & 3, "?")
            self.ctx.set_option("profile", 1)
            self.timed(lambda: self.stats(sideband))
            walk, kern = self.plan.last_timings()[:2]
            self.ctx.set_option("profile", 0)
            print(f"{label:14s} {self.plan.total_waves:8d} waveforms {self.plan.total_samples / 1e9:6.2f} GS stream {self.enc.total_words * 4 / 1e9:5.2f} GB  "
                  f"decode {np.median(td):8.3f} [{td.min():.3f} .. {td.max():.3f}]  stats({form}) {np.median(ts):8.3f} [{ts.min():.3f} .. {ts.max():.3f}] "
                  f"(walk {walk:.3f} kernels {kern:.3f})  x{np.median(ts) / np.median(td):.2f} of decode", flush=True)
            return
        for i in range(warmup + calls):
            if yardstick:
                td.append(self.timed(self.decode)[0])
                t, want = self.timed(lambda: self.reduce(self.decode()))
                tr.append(t)
            t, got = self.timed(lambda: self.stats(sideband))
            ts.append(t)
            if yardstick and i == 0:
                cols = [dr.STAT_MIN, dr.STAT_MAX, dr.STAT_SUM, dr.STAT_SUMSQ, dr.STAT_HEAD_SUM, dr.STAT_HEAD_SUMSQ]
                match = torch.equal(got[:, cols], want[:, cols])
        ts = np.array(ts[warmup:])
        self.ctx.set_option("profile", 1)
        self.timed(lambda: self.stats(sideband))
        walk, kern = self.plan.last_timings()[:2]
        self.ctx.set_option("profile", 0)
        stream_gb = self.enc.total_words * 4 / 1e9
        head = f"{label:14s} {self.plan.total_waves:8d} waveforms {self.plan.total_samples / 1e9:6.2f} GS stream {stream_gb:5.2f} GB  "
        if not yardstick:
            print(head + f"stats {np.median(ts):8.3f} [{ts.min():.3f} .. {ts.max():.3f}] (walk {walk:.3f} kernel {kern:.3f})", flush=True)
            return
        # peak bytes of one call of each kind that allocates its own results
        self.y = self.rows = None
        p_red = self.peak(lambda: self.reduce(self.decode(torch.empty(self.plan.total_samples, dtype=torch.int16, device=self.ctx.device))))
        p_st = self.peak(lambda: self.stats(sideband, torch.empty((self.plan.total_waves, dr.STAT_COLS), dtype=torch.int64, device=self.ctx.device)))
        td, tr = np.array(td[warmup:]), np.array(tr[warmup:])
        spread = td.max() - td.min()
        verdict = "ok" if np.median(ts) < np.median(td) - spread else "NOT FASTER THAN DECODE"
        print(head + f"decode {np.median(td):8.3f} [{td.min():.3f} .. {td.max():.3f}]  decode+torch {np.median(tr):8.3f} [{tr.min():.3f} .. {tr.max():.3f}]  "
              f"stats {np.median(ts):8.3f} [{ts.min():.3f} .. {ts.max():.3f}] (walk {walk:.3f} kernel {kern:.3f})  "
              f"x{np.median(td) / np.median(ts):.2f} of decode, x{np.median(tr) / np.median(ts):.1f} of decode+torch  "
              f"peak {p_st / 1e6:.1f} MB against {p_red / 1e9:.2f} GB  {verdict}{'' if match else '  MISMATCH'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head", type=int, default=500)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--decode-yardstick", action="store_true")
    a = ap.parse_args()
    ctx = dr.Context(0)
    only = [s for s in a.only.split(",") if s]
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}; head = {a.head}")
    cases = [
        ("headline", lambda: ([2000 * 7000] * a.chunks, [7000] * a.chunks), 10.0, False),
        ("headline-loud", lambda: ([2000 * 7000] * a.chunks, [7000] * a.chunks), 400.0, False),
        ("short", lambda: ([8192 * 512] * 300, [512] * 300), 10.0, False),
        ("config5", lambda: geometry("config5"), 10.0, False),
        ("noptrex", lambda: geometry("noptrex"), 10.0, False),
        ("headline-sb", lambda: ([2000 * 7000] * a.chunks, [7000] * a.chunks), 10.0, True),
        ("nedm", lambda: geometry("nedm"), 10.0, False),
        ("long25", lambda: geometry("long25"), 10.0, False),
        ("stream-quiet", lambda: ([2100 * 7000] * 4, [7000] * 4), 10.0, False),
    ]
    for name, geom, sigma, sideband in cases:
        if only and name not in only:
            continue
        Ns, Ls = geom()
        if name == "long25" and not (a.decode_yardstick or a.no_yardstick):
            print("long25         skipped: --decode-yardstick or --no-yardstick only", flush=True)
            continue
        c = Case(ctx, list(Ns), list(Ls), sigma, a.head, reduces=not (a.decode_yardstick or a.no_yardstick))
        c.line(name, a.calls, a.warmup, sideband, not a.no_yardstick, a.decode_yardstick)
        c.plan.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
