#!/usr/bin/env python3
"""The encoded gather (Plan.gather_encoded) against what a user did without it for the same job: decode the selected
waveforms, then encode them on a plan of the result.  The yardstick is `decode_select` + `encode`; for selections of a
fifth of the batch and more also `decode` + `index_select` + `encode`, and the better of the two counts.  All are timed
with HIP events around the call (the host's part included), in the same process and alternating; median of --calls calls
behind --warmup, [min .. max] printed.  The plan of the result and every buffer exist before the timed calls on both sides:
"gather" is ONE drx_gather_encoded call into a buffer of the known size.  "wrapper" is what Plan.gather_encoded costs a
caller who knows nothing: the geometry check, the sizing call, the wait for its total, the allocation and the call that
resumes from the sizing call's tables; a line whose wrapper loses to the yardstick says so.

  headline    --chunks (500) chunks of 2000 x 7000 (Gaussian, sigma = 10, m = 8, seeded): S = 1, 64, 4096, 4096 out of 4
              chunks, 65 536, 262 144, a permutation of all waveforms, and the identity re-chunked to 4 x as many chunks
  short       100 chunks of 14 M samples, WaveformLength 64 and 512, a 10 % selection (the copy by tiles)
  noptrex     64 of 2048 waveforms of 500 000 samples;  long-40: 64 of 1280 waveforms of 50 000 (the copy by pieces)
  fir5        a five-tap prediction filter (the yardstick's decode and encode are the serial kernels)

usage: gather_bench.py [--chunks 500] [--calls 20] [--warmup 5] [--only headline|short|noptrex|long-40|fir5] [--no-yardstick]
                       [--other-copy]
A line is "ok" when the gather beats the yardstick by more than the yardstick's own min-max spread in this run.  For the
permutation and the identity the line also gives the bytes moved (the gathered stream read and written once) over the time
of the copy kernel, from the plan's own events, as a share of 8 TB/s and of the 6.29 TB/s a float4 copy reaches.
Behind `rocprofv3 --kernel-trace --stats --` (no counters), `--only headline --no-yardstick` gives the kernels' own times."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import deltarice_amd as dr  # noqa: E402
from select_bench import samples  # noqa: E402


class Case:
    def __init__(self, ctx, n_chunks, chunk_samples, L, m=8, taps=None, sigma=10.0):
        self.ctx, self.L, self.m, self.taps = ctx, L, m, taps
        self.x = samples(ctx, n_chunks * chunk_samples, sigma)
        ftaps = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()
        self.opts = (m, L) + ftaps
        self.plan = ctx.plan_uniform(n_chunks, chunk_samples, self.opts)
        torch.cuda.synchronize()
        self.enc = self.plan.encode(self.x)
        self.W = n_chunks * (chunk_samples // L)
        self.waves_per_chunk = chunk_samples // L
        self.y = None  # the whole batch decoded (allocated when a line needs the second yardstick)

    def timed(self, fn, plan=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        (plan or self.plan).finish()
        return a.elapsed_time(b), r

    def line(self, label, sel, cw, calls, warmup, yardstick=True, bandwidth=False):
        ctx, plan, enc, L = self.ctx, self.plan, self.enc, self.L
        S = sel.size
        n_out = -(-S // cw)
        # sizing call, then every buffer of both sides
        t_size, (_, off, tab) = self.timed(lambda: plan.gather_encoded_async(enc.words, enc.chunk_word_off, sel, cw, None, enc.total_words))
        total = plan.finish()
        out = torch.empty(total, dtype=torch.int32, device=ctx.device)
        rp = ctx.plan_uniform(n_out, cw * L, self.opts) if S % cw == 0 else ctx.plan([cw * L] * (n_out - 1) + [(S - (n_out - 1) * cw) * L], [L] * n_out, self.m, self.taps)
        rows = torch.empty((S, L), dtype=torch.int16, device=ctx.device)
        ywords = torch.empty(rp.max_encoded_words, dtype=torch.int32, device=ctx.device)
        yoff = torch.empty(n_out + 1, dtype=torch.int64, device=ctx.device)
        idx_dev = torch.from_numpy(sel.astype(np.int64)).to(ctx.device)
        whole = yardstick and S * 5 >= self.W
        if whole and self.y is None:
            self.y = torch.empty_like(self.x)

        def gather():
            return plan.gather_encoded_async(enc.words, enc.chunk_word_off, sel, cw, out, enc.total_words, None, off, tab)

        def by_select():
            plan.decode_select_async(enc.words, enc.chunk_word_off, sel, out=rows, in_words=enc.total_words)
            return rp.encode_async(rows.view(-1), ywords, yoff)

        def by_decode():
            y = plan.decode_async(enc.words, enc.chunk_word_off, self.y, in_words=enc.total_words)
            torch.index_select(y.view(-1, L), 0, idx_dev, out=rows)
            return rp.encode_async(rows.view(-1), ywords, yoff)

        def wrapper():
            return plan.gather_encoded(enc, sel, cw)

        tg, t1, t2, tw = [], [], [], []
        same = True
        for i in range(warmup + calls):
            if yardstick:
                t, _ = self.timed(by_select, rp)
                t1.append(t)
                if whole:
                    t, _ = self.timed(by_decode, rp)
                    t2.append(t)
            t, _ = self.timed(gather)  # (a whole call: only the call right behind a sizing call resumes, and the wrapper's did)
            tg.append(t)
            t, g = self.timed(wrapper)
            tw.append(t)
            del g
            if yardstick and i == 0:
                same = rp.finish() == total and torch.equal(ywords[:total], out) and torch.equal(yoff, off)
        tg, tw = np.array(tg[warmup:]), np.array(tw[warmup:])
        ctx.set_option("profile", 1)
        self.timed(gather)
        walk, scan, copy, _ = plan.last_timings()
        ctx.set_option("profile", 0)
        touched = np.unique(sel // self.waves_per_chunk).size
        text = (f"{label:26s} {S:8d} {touched:5d} -> {n_out:5d}  gather {np.median(tg):8.3f} [{tg.min():.3f} .. {tg.max():.3f}]  "
                f"(walk {walk:.3f} scan {scan:.3f} copy {copy:.3f})  wrapper {np.median(tw):8.3f} [{tw.min():.3f} .. {tw.max():.3f}]")
        if bandwidth:
            tbs = 2 * total * 4 / (copy * 1e-3) / 1e12
            text += f"  copy {tbs:.2f} TB/s = {tbs / 8 * 100:.0f} % of 8, {tbs / 6.29 * 100:.0f} % of 6.29"
        if yardstick:
            ty = np.array(t1[warmup:])
            name = "select+encode"
            if whole and np.median(t2[warmup:]) < np.median(ty):
                ty, name = np.array(t2[warmup:]), "decode+index+encode"
            spread = ty.max() - ty.min()
            verdict = "ok" if np.median(tg) < np.median(ty) - spread else "NOT FASTER"
            text += (f"  yardstick ({name}) {np.median(ty):8.3f} [{ty.min():.3f} .. {ty.max():.3f}]  x{np.median(ty) / np.median(tg):.1f}  "
                     f"{verdict}{'' if same else '  MISMATCH'}{'' if np.median(tw) < np.median(ty) - spread else '  (wrapper NOT FASTER)'}")
        print(text, flush=True)
        rp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--other-copy", action="store_true", help="the copy form the code length does not choose (A/B of the route)")
    a = ap.parse_args()
    ctx = dr.Context(0)
    if a.other_copy:
        ctx.set_option("debug_flags", dr._lib.DBG_GATHER_OTHER_COPY)
    rng = np.random.default_rng(2025)
    yd = not a.no_yardstick
    print(f"{'case':26s} {'S':>8s} chunks in -> out  times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")
    if a.only in ("", "headline"):
        c = Case(ctx, a.chunks, 2000 * 7000, 7000)
        W = c.W
        for S in (1, 64, 4096, 65536, 262144):
            S = min(S, W)
            c.line("headline", rng.choice(W, S, replace=False), min(S, 2048), a.calls, a.warmup, yd)
        four = rng.choice(a.chunks, 4, replace=False)
        sel = (four[:, None] * 2000 + np.arange(2000)[None, :]).reshape(-1)
        c.line("headline, 4 chunks", rng.choice(sel, min(4096, sel.size), replace=False), 2048, a.calls, a.warmup, yd)
        c.line("headline, permutation", rng.permutation(W), 2000, a.calls, a.warmup, yd, bandwidth=True)
        c.line("headline, identity x4", np.arange(W), 500, a.calls, a.warmup, yd, bandwidth=True)
        del c
    for name, n_chunks, N, L, S, taps, sigma, m in (("short-64", 100, 14_000_000 // 64 * 64, 64, None, None, 10.0, 8),
                                                    ("short-512", 100, 14_000_000 // 512 * 512, 512, None, None, 10.0, 8),
                                                    ("noptrex", 2048, 500_000, 500_000, 64, None, 10.0, 8),
                                                    ("long-40", 40, 32 * 50_000, 50_000, 64, None, 10.0, 8),
                                                    ("fir5", 100, 200 * 7000, 7000, 2000, (1, -1, 1, -1, 1), 40.0, 32)):
        if a.only not in ("", name, name.split("-")[0]):
            continue
        c = Case(ctx, n_chunks, N, L, m, taps, sigma)
        S = c.W // 10 if S is None else S
        cw = {"short-64": 20000, "short-512": 2500, "noptrex": 1, "long-40": 32, "fir5": 200}[name]
        S = S // cw * cw
        c.line(name, rng.choice(c.W, S, replace=False), cw, a.calls, a.warmup, yd)
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
