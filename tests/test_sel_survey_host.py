"""CPU: deltarice_amd/csrc/drx_sel_survey.h -- which chunk holds each listed waveform, which chunks a selection touches and in
which of the walk's three lists, and the output-chunk rule of drx_gather_encoded -- compiled by the HOST compiler without HIP,
with -fsanitize=address,undefined, into tests/sel_survey_host.cpp's stand-alone program, which holds it to a plain loop (a
linear search, a std::set, a stable partition) over written-out lists and some thousands of random ones on uniform and ragged
plans, a plan of more than 2^32 waveforms among them.  The program carries the sanitizers' runtimes itself and is run
directly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selection_survey_and_gather_rule_against_a_plain_loop(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    header = os.path.join(ROOT, "deltarice_amd", "csrc", "drx_sel_survey.h")
    assert os.path.exists(header), "the selection survey has no header of its own"
    text = open(header).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower() and "drx_internal.h" not in re.sub(r"//[^\n]*", "", text), \
        "drx_sel_survey.h is host arithmetic: no HIP, no project header"
    exe = tmp_path / "sel_survey_host"
    # the sanitizers' runtimes inside the program: GCC and clang spell that differently
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined"] + static_rt + ["-I", os.path.dirname(header),
                            os.path.join(ROOT, "tests", "sel_survey_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
    assert int(r.stdout.split(" cases")[0].split()[-1]) > 5000, r.stdout[-2000:]
