"""CPU: the window rule of the decoupled look-back (deltarice_amd/csrc/drx_lookback.h: where the nearest prefix of a polled
window lies, whether an entry in front of it is still missing, which lanes' entries count), compiled host-side into
tests/lookback_rule_host.cpp's stand-alone program and held there to a scalar model over every (prefix, hole) pair of a
window, the windows without a prefix and 200 000 drawn ones; once plainly and once under the address and undefined-behaviour
sanitizers (a plain program: nothing is preloaded)."""
import os
import subprocess

import pytest

from kernel_build import CSRC, ROOT, find_compiler

WINDOWS = 129 * 129 + 200000


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_window_rule_against_the_scalar_model(tmp_path, sanitize):
    cc, _ = find_compiler()
    exe = tmp_path / "lookback_rule_host"
    # the header is HIP (the device walk beside the rule): the host half of a HIP compile, no device code, no GPU
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    build = subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Werror", "-x", "hip", "--offload-host-only", *flags, "-I", CSRC,
                            os.path.join(ROOT, "tests", "lookback_rule_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == "", r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == f"{WINDOWS} windows, 0 mismatches", r.stdout[-2000:]
