"""CPU: deltarice_amd/csrc/drx_pulse_runs.h -- the run summaries, pulse_combine() and the per-waveform stitch that the block
form of drx_find_pulses uses at the level of lanes and of blocks -- compiled by the HOST compiler without HIP, with
-fsanitize=address,undefined, into tests/pulse_runs_host.cpp's stand-alone program, which holds them to a plain loop over some
thousands of random sequences (all-over, none-over and alternating ones among them; thresholds beyond both clamps; both
polarities; min_width 1-8; max_pulses 0-6; staging caps below, at and above what a block holds).  The program carries the
sanitizers' runtimes itself and is run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_summaries_combine_and_stitch_against_a_plain_loop(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    header = os.path.join(ROOT, "deltarice_amd", "csrc", "drx_pulse_runs.h")
    assert os.path.exists(header), "the run summaries have no header of their own"
    exe = tmp_path / "pulse_runs_host"
    # the sanitizers' runtimes inside the program: GCC and clang spell that differently
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined"] + static_rt + ["-I", os.path.dirname(header),
                            os.path.join(ROOT, "tests", "pulse_runs_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
