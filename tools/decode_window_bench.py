#!/usr/bin/env python3
"""A window of every waveform from the encoded stream (`plan.decode_window`) against what a user did without it: `plan.decode`
of the whole batch, then `torch.gather` of the same windows out of the decoded samples.  Everything is timed with HIP events
around the call, in one process and alternating, so that the yardsticks are taken in the same run; median [min .. max] of
--calls calls behind --warmup.  Two yardsticks per line: `plan.decode` alone (the floor of any route through decoded samples)
and `plan.decode` + the gather (for the whole-waveform window the decoded batch IS the result: decode alone).

  headline        500 chunks of 2000 x 7000, m = 8, Gaussian sigma = 10 (seeded), a pulse of 3000 somewhere in every waveform
  headline-loud   the same with sigma = 400
  short           300 chunks of 8192 x 512
  noptrex         2048 waveforms of 500 000 samples (few long waveforms: a lane each, reported, not gated)

and for each batch three windows: `head` = [0, 500); `pulse` = 256 samples from STAT_ARGMAX - 64 (the start column of a
`plan.wave_stats` result, passed as it is); `whole` = [0, WaveformLength), the worst case for the stores.

Peak bytes: torch's peak allocation during one call that allocates its own result, above what the encoded batch occupies.

usage: decode_window_bench.py [--chunks 500] [--calls 20] [--warmup 5] [--only NAME[,NAME]] [--windows head,pulse,whole] [--no-yardstick]
A line is "ok" when the window call takes less time than `plan.decode` alone by more than that decode's min-to-max spread over
the alternating runs.  Behind `rocprofv3 --kernel-trace --pmc FETCH_SIZE -- ` (a run of its own), `--only headline
--no-yardstick --calls 1 --warmup 0` gives k_decode_window's HBM read per window; the line prints the stream bytes the
windows need (the payload words up to each window's last code, from the parse itself: `needed`) to divide it by."""
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
        self.ctx, self.L = ctx, L
        x = samples(ctx, n_chunks * N, sigma)
        W = n_chunks * (N // L)
        g = torch.Generator(device=ctx.device).manual_seed(7)
        at = torch.randint(0, L, (W,), device=ctx.device, generator=g) + torch.arange(W, device=ctx.device) * L
        x[at] = 3000  # the pulse the argmax column finds
        self.plan = ctx.plan_uniform(n_chunks, N, (m, L))
        torch.cuda.synchronize()
        self.enc = self.plan.encode(x)
        del x, at
        self.W = self.plan.total_waves
        self.stats = self.plan.wave_stats(self.enc)
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

    def decode(self, out=None):
        return self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, self.y if out is None else out, in_words=self.enc.total_words)

    def gather(self, y, start, offset, width):
        """The same rows out of decoded samples: indices, a gather, the pads."""
        v = y.view(self.W, self.L)
        if start is None and width == self.L:
            return v
        if start is None:
            return v[:, :width].contiguous()
        idx = (start + offset)[:, None] + torch.arange(width, device=y.device)[None, :]
        rows = torch.gather(v, 1, idx.clamp(0, self.L - 1))
        return torch.where((idx >= 0) & (idx < self.L), rows, torch.zeros_like(rows))

    def window(self, start, offset, width, out=None):
        return self.plan.decode_window_async(self.enc.words, self.enc.chunk_word_off, start, width, offset=offset, out=out,
                                             in_words=self.enc.total_words)

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

    def needed_bytes(self, start, offset, width):
        """Stream bytes the windows need: every payload up to its window's end, taken as e / L of the payload (the codes of a
        stationary signal are of one mean length), plus the headers."""
        n = self.plan.wave_words_device().to(torch.float64)
        a = torch.zeros(self.W, dtype=torch.int64, device=n.device) if start is None else start + offset
        e = torch.where(a < self.L, (a + width).clamp(0, self.L), torch.zeros_like(a)).to(torch.float64)
        return float((n * e / self.L).sum() + self.W) * 4

    def line(self, label, wname, start, offset, width, calls, warmup, yardstick=True):
        out = torch.empty((self.W, width), dtype=torch.int16, device=self.ctx.device)
        td, tg, tw = [], [], []
        match = True
        whole = start is None and width == self.L
        for i in range(warmup + calls):
            if yardstick:
                td.append(self.timed(self.decode)[0])
                if whole:
                    want = self.y.view(self.W, self.L)
                else:
                    t, want = self.timed(lambda: self.gather(self.decode(), start, offset, width))
                    tg.append(t)
            t, got = self.timed(lambda: self.window(start, offset, width, out))
            tw.append(t)
            if yardstick and i == 0:
                match = torch.equal(got, want)
            want = None
        tw = np.array(tw[warmup:])
        self.ctx.set_option("profile", 1)
        self.timed(lambda: self.window(start, offset, width, out))
        walk, kern = self.plan.last_timings()[:2]
        self.ctx.set_option("profile", 0)
        stream_gb, need_gb = self.enc.total_words * 4 / 1e9, self.needed_bytes(start, offset, width) / 1e9
        head = (f"{label:14s} {wname:6s} width {width:6d} {self.W:8d} waveforms stream {stream_gb:5.2f} GB needed {need_gb:6.3f} GB "
                f"rows {self.W * width * 2 / 1e9:6.3f} GB  ")
        mine = f"window {np.median(tw):8.3f} [{tw.min():.3f} .. {tw.max():.3f}] (walk {walk:.3f} kernel {kern:.3f})"
        if not yardstick:
            print(head + mine, flush=True)
            return
        del out
        p_y = self.peak(lambda: self.gather(self.decode(torch.empty(self.plan.total_samples, dtype=torch.int16, device=self.ctx.device)),
                                            start, offset, width))
        p_w = self.peak(lambda: self.window(start, offset, width))
        td = np.array(td[warmup:])
        tg = td if whole else np.array(tg[warmup:])
        spread = td.max() - td.min()
        verdict = "ok" if np.median(tw) < np.median(td) - spread else "NOT FASTER THAN DECODE"
        print(head + f"decode {np.median(td):8.3f} [{td.min():.3f} .. {td.max():.3f}]  decode+gather {np.median(tg):8.3f} [{tg.min():.3f} .. {tg.max():.3f}]  "
              + mine + f"  x{np.median(td) / np.median(tw):.2f} of decode, x{np.median(tg) / np.median(tw):.2f} of decode+gather  "
              f"peak {p_w / 1e9:.3f} GB against {p_y / 1e9:.2f} GB  {verdict}{'' if match else '  MISMATCH'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--windows", default="head,pulse,whole")
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
    ]
    for name, n_chunks, N, L, sigma in cases:
        if only and name not in only:
            continue
        c = Case(ctx, n_chunks, N, L, sigma)
        for wname in a.windows.split(","):
            start, offset, width = {"head": (None, 0, min(500, L)), "pulse": (c.stats[:, dr.STAT_ARGMAX], -64, 256), "whole": (None, 0, L)}[wname]
            c.line(name, wname, start, offset, width, a.calls, a.warmup, not a.no_yardstick)
        c.plan.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
