#!/usr/bin/env python3
"""The samples around every pulse of every waveform from the encoded stream (`plan.decode_windows` over the records of
`plan.find_pulses`) against `plan.decode` of the whole batch, the first step of the only other route to those samples (a gather
over the pulse records would follow).  Everything is timed with HIP events around the call, in one process and alternating, so
that the yardstick is taken in the same run; median [min .. max] of --calls calls behind --warmup.

The batches are those of tools/find_pulses_bench.py (headline, noptrex, nedm, long25: a pulse of 3000 planted in every
waveform); the starts are the START column of `find_pulses` at 5 sigma with max_pulses = 4, passed as they are with their
counts: K = 4 window slots, width 256, offset -64.  Per batch:

  windows   the call as it routes itself (lanes for headline, blocks for the three long shapes) against `plan.decode`
  lanes     the long shapes again under DRX_DBG_WINDOWS_LANES: the block form's gain, and the lane kernel's rate in
            microseconds per sample of the longest parse (kernel time / WaveformLength) for the routing test of
            drx_windows_blocks.hip
  one       headline only: K = 1 (the first pulse of every waveform) against `plan.decode_window` with the same starts

usage: decode_windows_bench.py [--chunks 500] [--calls 20] [--warmup 5] [--only NAME[,NAME]]
A `windows` line is "ok" when the call takes less time than `plan.decode` alone by more than that decode's min-to-max spread
over the alternating runs, and NOT FASTER THAN DECODE otherwise; a `one` line is "ok" unless the call is slower than
`plan.decode_window` by more than that call's spread (SLOWER THAN DECODE_WINDOW).  MISMATCH: rows differ from a gather over the
decoded samples (checked once per line on the first and last 2048 waveforms, at the size that is timed)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import deltarice_amd as dr  # noqa: E402
from deltarice_amd import _lib as D  # noqa: E402
from find_pulses_bench import Case  # noqa: E402
from workload import geometry  # noqa: E402

K, WIDTH, OFFSET, PAD = 4, 256, -64, -1
FORMS = {1: "lanes", 2: "blocks", 6: "blocks+all"}


def spread(t):
    return f"{np.median(t):8.3f} [{t.min():.3f} .. {t.max():.3f}]"


class Windows(Case):
    def __init__(self, ctx, n_chunks, N, L, sigma):
        super().__init__(ctx, n_chunks, N, L, sigma)
        self.pulses_out = torch.empty(self.W * K * dr.PULSE_COLS, dtype=torch.int64, device=ctx.device)
        self.timed(lambda: self.pulses(int(5 * sigma), K, self.pulses_out))
        self.records = self.pulses_out.view(self.W, K, dr.PULSE_COLS)
        self.win_rows = torch.empty(self.W * K * WIDTH, dtype=torch.int16, device=ctx.device)

    def windows(self, k=K, count=True):
        return self.plan.decode_windows_async(self.enc.words, self.enc.chunk_word_off, self.records[:, :k, dr.PULSE_START], WIDTH,
                                              count=self.count if count else None, offset=OFFSET, pad=PAD, out=self.win_rows,
                                              in_words=self.enc.total_words)

    def window(self):
        return self.plan.decode_window_async(self.enc.words, self.enc.chunk_word_off, self.records[:, 0, dr.PULSE_START], WIDTH,
                                             offset=OFFSET, pad=PAD, out=self.win_rows, in_words=self.enc.total_words)

    def rows_match(self, got, k, count):
        """got [W, k, WIDTH] against a gather over the decoded samples in self.y, on the first and last 2048 waveforms"""
        ok = True
        for sl in (slice(0, min(2048, self.W)), slice(max(0, self.W - 2048), self.W)):
            g = torch.arange(self.W, device=self.y.device)[sl]
            a = self.records[sl, :k, dr.PULSE_START] + OFFSET
            idx = a[:, :, None] + torch.arange(WIDTH, device=a.device)[None, None, :]
            live = torch.arange(k, device=a.device)[None, :] < (self.count[sl].to(torch.int64)[:, None] if count else k)
            inside = (idx >= 0) & (idx < self.L) & live[:, :, None]
            src = torch.where(inside, g[:, None, None] * self.L + idx, torch.zeros_like(idx))
            want = torch.where(inside, self.y[src], torch.full_like(self.y[src], PAD))
            ok = ok and torch.equal(got[sl], want)
        return ok

    def head(self, label, cname, k):
        n = self.count.to(torch.int64)
        form = FORMS.get(self.plan.last_windows_form(), "?")
        return (f"{label:9s} {cname:8s} form {form:6s} K {k} width {WIDTH} {self.W:8d} waveforms of {self.L:9d} stream {self.enc.total_words * 4 / 1e9:5.2f} GB "
                f"live windows {float(n.clamp(max=k).sum()) / self.W:5.2f} per waveform, rows {self.W * k * WIDTH * 2 / 1e9:5.3f} GB  ")

    def profile(self, fn):
        self.ctx.set_option("profile", 1)
        self.timed(fn)
        walk, kern = self.plan.last_timings()[:2]
        self.ctx.set_option("profile", 0)
        return walk, kern

    def line_windows(self, label, calls, warmup):
        td, tw = [], []
        match = True
        for i in range(warmup + calls):
            td.append(self.timed(self.decode)[0])
            t, got = self.timed(self.windows)
            tw.append(t)
            if i == 0:
                match = self.rows_match(got, K, True)
        td, tw = np.array(td[warmup:]), np.array(tw[warmup:])
        walk, kern = self.profile(self.windows)
        verdict = "ok" if np.median(tw) < np.median(td) - (td.max() - td.min()) else "NOT FASTER THAN DECODE"
        print(self.head(label, "windows", K) + f"decode {spread(td)}  decode_windows {spread(tw)} (walk {walk:.3f} kernels {kern:.3f})  "
              f"x{np.median(td) / np.median(tw):.2f} of decode  {verdict}{'' if match else '  MISMATCH'}", flush=True)
        return np.median(tw)

    def line_lanes(self, label, calls, warmup, blocks_ms):
        self.ctx.set_option("debug_flags", D.DBG_WINDOWS_LANES)
        try:
            tw = []
            for i in range(warmup + calls):
                t, got = self.timed(self.windows)
                tw.append(t)
                if i == 0:
                    match = self.rows_match(got, K, True)
            tw = np.array(tw[warmup:])
            walk, kern = self.profile(self.windows)
            print(self.head(label, "lanes", K) + f"decode_windows {spread(tw)} (walk {walk:.3f} kernels {kern:.3f})  x{np.median(tw) / blocks_ms:.1f} the "
                  f"time of the block form, {kern * 1000 / self.L:.4f} us per sample of the longest parse{'' if match else '  MISMATCH'}", flush=True)
        finally:
            self.ctx.set_option("debug_flags", 0)

    def line_one(self, label, calls, warmup):
        t1, tw = [], []
        match = True
        for i in range(warmup + calls):
            t1.append(self.timed(self.window)[0])
            if i == 0:
                one = self.win_rows[:self.W * WIDTH].view(self.W, WIDTH).clone()
            t, got = self.timed(lambda: self.windows(1, False))
            tw.append(t)
            if i == 0:
                match = torch.equal(got[:, 0], one)
        t1, tw = np.array(t1[warmup:]), np.array(tw[warmup:])
        verdict = "ok" if np.median(tw) <= np.median(t1) + (t1.max() - t1.min()) else "SLOWER THAN DECODE_WINDOW"
        print(self.head(label, "one", 1) + f"decode_window {spread(t1)}  decode_windows {spread(tw)}  x{np.median(tw) / np.median(t1):.2f} the time "
              f"of decode_window  {verdict}{'' if match else '  MISMATCH'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    ctx = dr.Context(0)
    only = [s for s in a.only.split(",") if s]
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")
    nN, nL = geometry("noptrex")
    cases = [
        ("headline", a.chunks, 2000 * 7000, 7000, 10.0),
        ("noptrex", len(nN), nN[0], nL[0], 10.0),
        ("nedm", 256, 32 * 81920, 81920, 10.0),
        ("long25", 25, 14_000_000, 0, 10.0),
    ]
    for name, n_chunks, N, L, sigma in cases:
        if only and name not in only:
            continue
        c = Windows(ctx, n_chunks, N, L, sigma)
        ms = c.line_windows(name, a.calls, a.warmup)
        if name == "headline":
            c.line_one(name, a.calls, a.warmup)
        else:
            c.line_lanes(name, max(3, a.calls // 4), 1, ms)
        c.plan.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
