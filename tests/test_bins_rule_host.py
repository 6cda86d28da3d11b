"""CPU: the bin cursor of drx_wave_bins (deltarice_amd/csrc/drx_bin_cursor.h: the origin, where a cursor begun at any sample
stands among the bins, how it moves on at a border), compiled host-side into tests/bins_rule_host.cpp's stand-alone program and
held there to a scalar model in 128-bit arithmetic over 240 000 drawn (origin, bin, n_bins, len, first sample, count) tuples --
the int64 ends and +-2^31 among the origins, 1 ... 2^32 - 1 among the bins; once plainly and once under the address and
undefined-behaviour sanitizers (a plain program: nothing is preloaded)."""
import os
import subprocess

import pytest

from kernel_build import CSRC, ROOT, find_compiler

TUPLES = 240000


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_cursor_against_the_scalar_model(tmp_path, sanitize):
    cc, _ = find_compiler()
    exe = tmp_path / "bins_rule_host"
    # the header is HIP (host and device functions): the host half of a HIP compile, no device code, no GPU
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    build = subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Werror", "-x", "hip", "--offload-host-only", *flags, "-I", CSRC,
                            os.path.join(ROOT, "tests", "bins_rule_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == "", r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == f"{TUPLES} tuples, 0 mismatches", r.stdout[-2000:]
