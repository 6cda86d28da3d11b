#!/usr/bin/env python3
"""Re-coding an encoded batch at its best RiceParameter (`plan.transcode`) against what a user did without it: `plan.decode`
of the whole batch, then `plan.encode` of the samples under a plan of the new parameter -- both the existing routes.  Everything
is timed with HIP events around the calls, in one process and alternating, so that the yardstick is taken in the same run;
median [min .. max] of --calls calls behind --warmup.

  headline        500 chunks of 2000 x 7000, m = 8 -> its best m, Gaussian sigma = 10 (seeded)
  headline-loud   the same with sigma = 400
  short           300 chunks of 8192 x 512
  config5         BASELINE's mixed-length config 5 (ragged: 512 / 2048 / 7000 / 16384)
  nedm, noptrex, long25, noptrex_fir4
                  few long waveforms (the geometries of tools/workload.py; _fir4: under taps [1,-1,1,-1]): the block form of
                  drx_transcode_blocks.hip.  Columns: transcode as the library routes it (its form named), the lane form under
                  DRX_DBG_TRANSCODE_LANES in the same process, alternating (long25: 3 calls behind 1, a lane call takes seconds;
                  elsewhere --calls behind --warmup), decode + encode, the sizing call, the estimate.  These rows also run on a
                  library that has no block form (the form query is looked up): there both transcode columns are the lane form.

Columns: decode + encode; transcode into a given buffer, split as last_timings() splits it (walk, sizes + scan + offsets,
pack); the sizing call alone; `estimate_words_encoded` against decode + `estimate_words`; peak device bytes of each route
(torch's peak allocation during one call that allocates its own buffers, above what the encoded batch occupies: the decoded
samples and the new stream, or the new stream alone).

usage: transcode_bench.py [--chunks 500] [--calls 20] [--warmup 5] [--only NAME[,NAME]] [--no-yardstick]
A line is "ok" when the transcode takes less time than decode + encode by more than that pair's min-to-max spread over the
alternating runs.  Behind `rocprofv3 --pmc ... --` (a run of its own), `--only headline --no-yardstick` gives the memory
traffic of the transcode's kernels alone."""
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
from workload import FIR4, geometry  # noqa: E402


def med(t):
    t = np.array(t)
    return f"{np.median(t):8.3f} [{t.min():.3f} .. {t.max():.3f}]"


class Case:
    def __init__(self, ctx, Ns, Ls, sigma, m=8, taps=None):
        self.ctx, self.m = ctx, m
        self.uniform = len(set(Ns)) == 1 and len(set(Ls)) == 1
        ftaps = (len(taps),) + tuple(int(t) & 0xFFFFFFFF for t in taps) if taps else ()
        opts = lambda mm: (mm, Ls[0] if Ls[0] > 0 else 0xFFFFFFFF) + ftaps  # noqa: E731
        self.mk = lambda mm: ctx.plan_uniform(len(Ns), Ns[0], opts(mm)) if self.uniform else ctx.plan(Ns, Ls, mm, taps)
        self.taps = taps
        self.plan = self.mk(m)
        x = samples(ctx, sum(Ns), sigma)
        torch.cuda.synchronize()
        self.enc = self.plan.encode(x)
        self.est = self.plan.estimate_words_encoded(self.enc)
        assert taps is not None or self.est.tolist() == self.plan.estimate_words(x).tolist(), "the two estimates differ"
        del x
        self.m2 = 1 << int(np.argmin(self.est))
        self.total2 = int(self.est.min())
        self.plan2 = self.mk(self.m2)

    def timed(self, fn, plans):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ctx.stream):
            a.record()
            r = fn()
            b.record()
        b.synchronize()
        for p in plans:
            p.finish()
        return a.elapsed_time(b), r

    def pair(self, y, out):
        self.plan.decode_async(self.enc.words, self.enc.chunk_word_off, y, in_words=self.enc.total_words)
        return self.plan2.encode_async(y, out_words=out)

    def transcode(self, out, off=None, tab=None):
        return self.plan.transcode_async(self.enc.words, self.enc.chunk_word_off, self.m2, out, self.enc.total_words, None, off, tab)

    def peak(self, fn, plans):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.cuda.stream(self.ctx.stream):
            r = fn()
        for p in plans:
            p.finish()
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated() - base

    def line(self, label, calls, warmup, yardstick=True):
        dev, plan, plan2 = self.ctx.device, self.plan, self.plan2
        out = torch.empty(self.total2, dtype=torch.int32, device=dev)
        off = torch.empty(plan.n_chunks + 1, dtype=torch.int64, device=dev)
        tab = torch.empty(plan.total_waves, dtype=torch.int32, device=dev)
        tp, tt, tsz, te, tde = [], [], [], [], []
        match = True
        if yardstick:
            y = torch.empty(plan.total_samples, dtype=torch.int16, device=dev)
            out_y = torch.empty(self.total2, dtype=torch.int32, device=dev)
        for i in range(warmup + calls):
            if yardstick:
                tp.append(self.timed(lambda: self.pair(y, out_y), (plan, plan2))[0])
            tt.append(self.timed(lambda: self.transcode(out, off, tab), (plan,))[0])
            if yardstick and i == 0:
                match = torch.equal(out, out_y)
            tsz.append(self.timed(lambda: self.transcode(None, off, tab), (plan,))[0])
            if yardstick:
                te.append(self.timed(lambda: plan.estimate_words_encoded(self.enc), ())[0])

                def decode_estimate():
                    plan.decode_async(self.enc.words, self.enc.chunk_word_off, y, in_words=self.enc.total_words)
                    return plan.estimate_words(y)
                tde.append(self.timed(decode_estimate, (plan,))[0])
        self.ctx.set_option("profile", 1)
        self.timed(lambda: self.transcode(out, off, tab), (plan,))
        walk, sizes, pack = plan.last_timings()[:3]
        self.ctx.set_option("profile", 0)
        tt, tsz = tt[warmup:], tsz[warmup:]
        head = (f"{label:14s} {plan.total_waves:8d} waveforms {plan.total_samples / 1e9:6.2f} GS  m {self.m} -> {self.m2}  "
                f"stream {self.enc.total_words * 4 / 1e9:5.2f} -> {self.total2 * 4 / 1e9:5.2f} GB\n    ")
        split = f"transcode {med(tt)} (walk {walk:.3f} sizes+scan+offsets {sizes:.3f} pack {pack:.3f})  sizing call {med(tsz)}"
        if not yardstick:
            print(head + split, flush=True)
            return
        del y, out_y, out
        tp, te, tde = np.array(tp[warmup:]), te[warmup:], tde[warmup:]
        p_pair = self.peak(lambda: self.pair(torch.empty(plan.total_samples, dtype=torch.int16, device=dev),
                                             torch.empty(self.total2, dtype=torch.int32, device=dev)), (plan, plan2))
        p_tr = self.peak(lambda: self.transcode(torch.empty(self.total2, dtype=torch.int32, device=dev)), (plan,))
        spread = tp.max() - tp.min()
        verdict = "ok" if np.median(tt) < np.median(tp) - spread else "NOT FASTER THAN DECODE + ENCODE"
        print(head + f"decode+encode {med(tp)}  {split}  x{np.median(tp) / np.median(tt):.2f}\n    "
              f"estimate_words_encoded {med(te)} against decode+estimate_words {med(tde)}  "
              f"peak {p_tr / 1e9:.2f} GB against {p_pair / 1e9:.2f} GB  {verdict}{'' if match else '  MISMATCH'}", flush=True)


    def line_long(self, label, calls, warmup):
        """The rows of few long waveforms: the library's route and the lane form, alternating in one process."""
        dev, plan, plan2 = self.ctx.device, self.plan, self.plan2
        lanes_flag = getattr(dr._lib, "DBG_TRANSCODE_LANES", 1024)
        form_of = getattr(plan, "last_transcode_form", lambda: 0)
        out = torch.empty(self.total2, dtype=torch.int32, device=dev)
        out_l = torch.empty(self.total2, dtype=torch.int32, device=dev)
        out_y = torch.empty(self.total2, dtype=torch.int32, device=dev)
        off = torch.empty(plan.n_chunks + 1, dtype=torch.int64, device=dev)
        tab = torch.empty(plan.total_waves, dtype=torch.int32, device=dev)
        y = torch.empty(plan.total_samples, dtype=torch.int16, device=dev)
        tb, tl, tp, tsz, te = [], [], [], [], []
        form = 0
        for i in range(warmup + calls):
            tb.append(self.timed(lambda: self.transcode(out, off, tab), (plan,))[0])
            form = form_of()
            self.ctx.set_option("debug_flags", lanes_flag)
            tl.append(self.timed(lambda: self.transcode(out_l, off, tab), (plan,))[0])
            self.ctx.set_option("debug_flags", 0)
            tp.append(self.timed(lambda: self.pair(y, out_y), (plan, plan2))[0])
            tsz.append(self.timed(lambda: self.transcode(None, off, tab), (plan,))[0])
            te.append(self.timed(lambda: plan.estimate_words_encoded(self.enc), ())[0])
            if i == 0:
                match = torch.equal(out, out_l) and (self.taps is not None or torch.equal(out, out_y))
        tb, tl, tp, tsz, te = (np.array(t[warmup:]) for t in (tb, tl, tp, tsz, te))
        name = {0: "no form query", 1: "LANES", 2: "BLOCKS"}.get(form, str(form))
        print(f"{label:14s} {plan.total_waves:8d} waveforms {plan.total_samples / 1e9:6.2f} GS  m {self.m} -> {self.m2}  "
              f"stream {self.enc.total_words * 4 / 1e9:5.2f} -> {self.total2 * 4 / 1e9:5.2f} GB\n    "
              f"transcode ({name}) {med(tb)}  lane form {med(tl)}  x{np.median(tl) / np.median(tb):.1f} "
              f"(lane form {np.median(tl) * 1e3 / max(plan.longest_wave(), 1):.4f} us per sample of the longest waveform)\n    "
              f"decode+encode {med(tp)}  sizing call {med(tsz)}  estimate_words_encoded {med(te)}"
              f"{'' if match else '  MISMATCH'}", flush=True)


LONG_ROWS = {"nedm": None, "noptrex": None, "long25": None, "noptrex_fir4": FIR4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    ctx = dr.Context(0)
    only = [s for s in a.only.split(",") if s]
    print(f"times in ms: median [min .. max] of {a.calls} calls behind {a.warmup}")
    cases = [
        ("headline", lambda: ([2000 * 7000] * a.chunks, [7000] * a.chunks), 10.0),
        ("headline-loud", lambda: ([2000 * 7000] * a.chunks, [7000] * a.chunks), 400.0),
        ("short", lambda: ([8192 * 512] * 300, [512] * 300), 10.0),
        ("config5", lambda: geometry("config5"), 10.0),
    ]
    for name, taps in LONG_ROWS.items():
        if name not in only:  # (these rows run where they are asked for)
            continue
        Ns, Ls = geometry(name)
        c = Case(ctx, list(Ns), list(Ls), 10.0, taps=taps)
        c.line_long(name, *((3, 1) if name == "long25" else (a.calls, a.warmup)))
        c.plan.close()
        c.plan2.close()
        del c
        torch.cuda.empty_cache()
    for name, geom, sigma in cases:
        if only and name not in only:
            continue
        Ns, Ls = geom()
        c = Case(ctx, list(Ns), list(Ls), sigma)
        c.line(name, a.calls, a.warmup, not a.no_yardstick)
        c.plan.close()
        c.plan2.close()
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
