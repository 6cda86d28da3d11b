#!/usr/bin/env python3
"""The kernels every block-form call launches, in stream order: drx_decode, drx_wave_stats, drx_find_pulses and
drx_decode_windows once each on a uniform and on a ragged batch of few long waveforms (the shapes of test_forms and
test_ragged_long_batch of the block-form test files), find_pulses a second time with max_pulses above DRX_PULSES_STAGE_CAP (the
second launch of its blocks), and drx_decode with a general filter on both sides of the block decoder's `fuse` condition
(DRX_DBG_IIR_SEPARATE: the unfused side).

  blocks_launch_order.py          runs itself behind `rocprofv3 --kernel-trace --` (nothing else is traced) under a time limit,
                                  then prints, per call, the forms the library reports and the kernel names of the trace in the
                                  order of their start
  blocks_launch_order.py --run    the traced program: the calls, a torch kernel behind each as a separator, one line per call
  blocks_launch_order.py --dir D  the same as the first, and the trace stays in directory D

Two builds of the library (DRX_LIB_PATH) launch the same kernels in the same order when the two outputs are equal:
  DRX_LIB_PATH=old.so python3 tools/blocks_launch_order.py > a.txt; python3 tools/blocks_launch_order.py > b.txt; diff a.txt b.txt"""
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OURS = ("drx::", "__amd_rocclr_")  # the library's kernels and the runtime's (memsets); any other kernel is torch's: a separator


def run():
    import numpy as np
    import torch

    import deltarice_amd as dr
    from deltarice_amd import _lib as D

    ctx = dr.Context(0)
    sep = torch.zeros(64, dtype=torch.int32, device=ctx.device)

    def done(label, plan, what=lambda: ""):
        plan.finish()
        sep.add_(1)  # the separator, behind everything the call launched (whatever `what` runs is torch's as well)
        torch.cuda.synchronize()
        print(f"{label} | {what()}", flush=True)
        torch.cuda.synchronize()

    def forms(plan):
        return (f"decode_path {plan.last_decode_path()} stats_form {plan.last_stats_form()} pulses_form {plan.last_pulses_form()} "
                f"pulses_listed {plan.last_pulses_listed()} pulses_redone {plan.last_pulses_redone()} "
                f"windows_form {plan.last_windows_form()} windows_listed {plan.last_windows_listed()}")

    def batch(name, plan, n_samples, sigma, seed):
        x = torch.from_numpy(np.random.default_rng(seed).normal(0, sigma, n_samples).astype(np.int16)).to(ctx.device)
        enc = plan.encode(x)
        done(f"{name} encode", plan)
        return x, enc

    def four_calls(name, plan, n_samples, seed):
        x, enc = batch(name, plan, n_samples, 10, seed)
        y = plan.decode(enc)
        done(f"{name} decode", plan, lambda: forms(plan) + f" equal {bool(torch.equal(x, y))}")
        plan.wave_stats(enc, 500)
        done(f"{name} wave_stats", plan, lambda: forms(plan))
        n, p = plan.find_pulses(enc, 30, 1, 1, 4)
        done(f"{name} find_pulses max_pulses 4", plan, lambda: forms(plan))
        plan.find_pulses(enc, 15, 1, 1, D.PULSES_STAGE_CAP + 4)  # (15: 1.5 sigma, more pulses in a block than it stages)
        done(f"{name} find_pulses max_pulses {D.PULSES_STAGE_CAP + 4}", plan, lambda: forms(plan))
        plan.decode_windows(enc, p[:, :, D.PULSE_START], 64, count=n, offset=-16)
        done(f"{name} decode_windows", plan, lambda: forms(plan))
        plan.close()

    four_calls("uniform", ctx.plan_uniform(2, 32 * 50000, (8, 50000)), 2 * 32 * 50000, 1)
    Ns, Ls = [2048 * 5 + 9, 30000 * 3, 150001, 9001 * 4 - 3000], [2048, 30000, 0, 9001]
    four_calls("ragged", ctx.plan(Ns, Ls, 8), sum(Ns), 6)
    # a general filter the fast kernels take, as many long waveforms as the block decoder keeps resident: fused, then not
    N = 800 * 9001 - 9001 // 3
    plan = ctx.plan_uniform(2, N, (8, 9001, 4, 1, -1, 1, -1))
    x, enc = batch("filter", plan, 2 * N, 10, 3)
    for flags, side in ((0, "fused"), (D.DBG_IIR_SEPARATE, "separate")):
        ctx.set_option("debug_flags", flags)
        y = plan.decode(enc)
        done(f"filter decode {side}", plan, lambda: forms(plan) + f" equal {bool(torch.equal(x, y))}")
    ctx.set_option("debug_flags", 0)
    plan.close()
    ctx.close()


def short_name(name):
    """A demangled kernel name without its parameter list (the template arguments stay)."""
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    if "--run" in sys.argv[1:]:
        return run()
    keep = sys.argv[sys.argv.index("--dir") + 1] if "--dir" in sys.argv[1:] else None
    with tempfile.TemporaryDirectory() as tmp:
        td = keep or tmp
        r = subprocess.run(["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "-d", td, "-o", "t", "--output-format", "csv", "--",
                            sys.executable, os.path.abspath(__file__), "--run"], capture_output=True, text=True)
        labels = [ln for ln in r.stdout.splitlines() if " | " in ln]
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"the traced program ended with {r.returncode}")
        traces = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise SystemExit(f"expected one kernel trace, found {traces}")
        with open(traces[0], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda row: int(row["Start_Timestamp"]))
    groups, cur = [], []  # (every call launches a kernel of the library: a group without one lies between two of torch's kernels)
    for row in rows:
        if any(o in row["Kernel_Name"] for o in OURS):
            cur.append(short_name(row["Kernel_Name"]))
        else:
            if any(OURS[0] in n for n in cur):
                groups.append(cur)
            cur = []
    if len(groups) != len(labels):
        raise SystemExit(f"{len(labels)} calls, {len(groups)} separators in the trace")
    for label, names in zip(labels, groups):
        print(f"#### {label}")
        for n in names:
            print(f"    {n}")


if __name__ == "__main__":
    main()
