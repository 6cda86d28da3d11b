#!/usr/bin/env python3
"""The stack of selected, aligned waveforms from the encoded stream (`plan.wave_stack`) against what a user did without it, on
the headline batch (500 chunks of 2000 x 7000, m = 8, Gaussian sigma = 10, seeded): one process, HIP events around every call,
the yardsticks alternating with the call in the same run; median [min .. max] of --calls calls behind --warmup.  Every step
that uses the GPU runs under a time limit of its own (--limit seconds): a watchdog ends the process with status 124.

  full      wave_stack, no origins, the full width of 7000             against  decode + y.sum(0) + the squares
  argmax    wave_stack(start = ARGMAX, offset -64, width 512)          against  decode_window + the same two reductions
  select    `argmax` with a random 10 % selection                      against  decode_window + the reductions over the
                                                                                 selected rows, and the same on gather_encoded's batch
  forms     the two forms of a group apart, no yardstick: width 512 with no origins (equal) and with ARGMAX (distinct), width
            7000 with no origins (equal) and with origins random in [-300, 300] (distinct)

Each line also gives the header walk and the kernels behind it apart (drx_plan_last_timings), and the peak bytes torch allocated
during one call above what the encoded batch occupies.  The first call of every pair is compared: MISMATCH is printed otherwise.

usage: bench_stack.py [--only {full,argmax,select,forms}] [--chunks 500] [--calls 10] [--warmup 3] [--limit 120]"""
import argparse
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import deltarice_amd as dr  # noqa: E402
from wave_stats_bench import samples  # noqa: E402

L, WAVES, WIDTH, OFFSET, SLAB = 7000, 2000, 512, -64, 1 << 15


class step:
    """A GPU step under its own time limit: the process ends with status 124 where the step does not"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def expired():
            print(f"time limit of {self.seconds} s reached in step: {self.what}", flush=True)
            os._exit(124)
        self.timer = threading.Timer(self.seconds, expired)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


class Case:
    def __init__(self, ctx, chunks, limit):
        self.ctx, self.limit = ctx, limit
        with step("samples and encode", limit):
            x = samples(ctx, chunks * WAVES * L, 10.0)
            self.plan = ctx.plan_uniform(chunks, WAVES * L, (8, L))
            torch.cuda.synchronize()
            self.enc = self.plan.encode(x)
            del x
            self.W = self.plan.total_waves
            self.y = torch.empty(self.plan.total_samples, dtype=torch.int16, device=ctx.device)
            self.stats = self.plan.wave_stats(self.enc)
            self.start = self.stats[:, dr.STAT_ARGMAX]  # the column as it is
            g = torch.Generator(device=ctx.device).manual_seed(6)
            # a tenth of the waveforms, in whole output chunks of gather_encoded
            n_sel = max(WAVES, self.W // 10 // WAVES * WAVES)
            self.idx = torch.randperm(self.W, device=ctx.device, generator=g)[:n_sel].sort().values
            self.select = torch.zeros(self.W, dtype=torch.bool, device=ctx.device)
            self.select[self.idx] = True
            torch.cuda.synchronize()

    def timed(self, fn, plan=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        (plan or self.plan).finish()
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

    # ---- the call
    def stack(self, width=None, start=None, offset=0, select=None):
        return self.plan.wave_stack_async(self.enc.words, self.enc.chunk_word_off, width, start, offset, select, in_words=self.enc.total_words)

    # ---- what a user does today
    @staticmethod
    def reduce(rows, ok=None):
        """int16 [n, width] -> int64 [width, 3] in slabs of 2^15 rows; ok: which cells hold a sample (None: all)"""
        width = rows.shape[1]
        out = torch.zeros((width, 3), dtype=torch.int64, device=rows.device)
        for g0 in range(0, rows.shape[0], SLAB):
            v = rows[g0:g0 + SLAB]
            v32 = v.to(torch.int32)
            if ok is None:
                out[:, 0] += v.shape[0]
            else:
                m = ok[g0:g0 + SLAB]
                out[:, 0] += m.sum(0, dtype=torch.int64)
                v32 = torch.where(m, v32, 0)
            out[:, 1] += v32.sum(0, dtype=torch.int64)
            out[:, 2] += (v32 * v32).sum(0, dtype=torch.int64)
        return out

    def decode_and_reduce(self, y=None):
        y = self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, self.y if y is None else y, in_words=self.enc.total_words)
        return self.reduce(y.view(-1, L))

    def window_and_reduce(self, rows_of=None):
        w = self.plan.decode_window_async(self.enc.words, self.enc.chunk_word_off, self.start, WIDTH, OFFSET, in_words=self.enc.total_words)
        idx = self.start[:, None] + (OFFSET + torch.arange(WIDTH, device=w.device))[None, :]
        ok = (idx >= 0) & (idx < L)
        if rows_of is not None:
            w, ok = w[rows_of], ok[rows_of]
        return self.reduce(w, ok)

    def gather_window_and_reduce(self, gplan):
        got = self.plan.gather_encoded(self.enc, self.idx_host, WAVES)
        st = self.start[self.idx].contiguous()
        w = gplan.decode_window(got.enc, st, WIDTH, OFFSET)
        idx = st[:, None] + (OFFSET + torch.arange(WIDTH, device=w.device))[None, :]
        return self.reduce(w, (idx >= 0) & (idx < L))

    def line(self, label, calls, warmup, call, baselines):
        """call: () -> rows; baselines: [(name, () -> rows, the plan to finish or None)]"""
        t_call, t_base = [], [[] for _ in baselines]
        match = True
        for i in range(warmup + calls):
            with step(f"{label}: wave_stack", self.limit):
                t, got = self.timed(call)
            t_call.append(t)
            for k, (name, fn, plan) in enumerate(baselines):
                with step(f"{label}: {name}", self.limit):
                    t, want = self.timed(fn, plan)
                t_base[k].append(t)
                if i == 0:
                    match = match and torch.equal(got, want)
                del want
            del got
        with step(f"{label}: profile and peak", self.limit):
            self.ctx.set_option("profile", 1)
            self.timed(call)
            walk, kern = self.plan.last_timings()[:2]
            self.ctx.set_option("profile", 0)
            p_call = self.peak(call)
            y_keep, self.y = self.y, None
            p_base = self.peak(baselines[0][1] if label != "full" else
                               lambda: self.decode_and_reduce(torch.empty(self.plan.total_samples, dtype=torch.int16, device=self.ctx.device)))
            self.y = y_keep

        def fmt(t):
            t = np.array(t[warmup:])
            return f"{np.median(t):9.3f} [{t.min():.3f} .. {t.max():.3f}]"

        med = lambda t: float(np.median(np.array(t[warmup:])))  # noqa: E731
        s = (f"{label:8s} {self.W:8d} waveforms {self.plan.total_samples / 1e9:6.2f} GS  wave_stack {fmt(t_call)} "
             f"(walk {walk:.3f} behind it {kern:.3f})  peak {p_call / 1e6:.3f} MB")
        for (name, _, _), t in zip(baselines, t_base):
            s += f"  | {name} {fmt(t)}  x{med(t) / med(t_call):.1f} of wave_stack"
        s += f"  | first baseline's peak {p_base / 1e9:.2f} GB{'' if match else '  MISMATCH'}"
        print(s, flush=True)


def forms(c, calls, warmup):
    g = torch.Generator(device=c.ctx.device).manual_seed(7)
    near = torch.randint(-300, 301, (c.W,), device=c.ctx.device, generator=g)
    for label, call in (("512 equal", lambda: c.stack(WIDTH)), ("512 distinct", lambda: c.stack(WIDTH, c.start, OFFSET)),
                        ("7000 equal", lambda: c.stack(L)), ("7000 distinct", lambda: c.stack(L, near))):
        ts = []
        for _ in range(warmup + calls):
            with step(f"forms: {label}", c.limit):
                ts.append(c.timed(call)[0])
        t = np.array(ts[warmup:])
        print(f"forms    width {label:14s} wave_stack {np.median(t):9.3f} [{t.min():.3f} .. {t.max():.3f}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds every GPU step may take")
    ap.add_argument("--only", choices=("full", "argmax", "select", "forms"))
    a = ap.parse_args()
    ctx = dr.Context(0)
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}", flush=True)
    c = Case(ctx, a.chunks, a.limit)
    if a.only in (None, "full"):
        c.line("full", a.calls, a.warmup, c.stack, [("decode + torch", c.decode_and_reduce, None)])
    if a.only in (None, "argmax"):
        c.line("argmax", a.calls, a.warmup, lambda: c.stack(WIDTH, c.start, OFFSET), [("decode_window + torch", c.window_and_reduce, None)])
    if a.only in (None, "select"):
        with step("the gathered batch's plan", a.limit):
            c.idx_host = c.idx.cpu()
            gplan = c.plan.gather_encoded(c.enc, c.idx_host, WAVES).plan(ctx)
        c.line("select", a.calls, a.warmup, lambda: c.stack(WIDTH, c.start, OFFSET, c.select),
               [("decode_window + torch", lambda: c.window_and_reduce(c.select), None),
                ("gather_encoded + decode_window + torch", lambda: c.gather_window_and_reduce(gplan), gplan)])
        gplan.close()
    if a.only in (None, "forms"):
        forms(c, a.calls, a.warmup)
    c.plan.close()


if __name__ == "__main__":
    main()
