"""CPU: deltarice_amd/csrc/h5_direct_plan.h -- the slabs the direct-chunk HDF5 path moves data in, rows to fetched chunks and
waveform indices, the row geometry read_rows and copy_rows accept, and the cd_values of a new dataset -- compiled by the HOST
compiler without HDF5 or HIP, with -fsanitize=address,undefined, into tests/h5_direct_plan_host.c's stand-alone program, which
holds each function to a plain restatement over written-out cases and some thousands of random ones.  The program carries the
sanitizers' runtimes itself and is run directly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_direct_chunk_arithmetic_against_a_plain_restatement(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    header = os.path.join(ROOT, "deltarice_amd", "csrc", "h5_direct_plan.h")
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    assert not re.search(r"hdf5|H5[A-Z]|hip|deltarice", text), "h5_direct_plan.h is host arithmetic: no HDF5, no HIP, no project header"
    source = open(os.path.join(ROOT, "deltarice_amd", "csrc", "h5_direct.c")).read()
    assert '#include "h5_direct_plan.h"' in source and "qsort" not in source, "h5_direct.c keeps no second copy"
    exe = tmp_path / "h5_direct_plan_host"
    # the sanitizers' runtimes inside the program: GCC and clang spell that differently
    version = subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined"] + static_rt + ["-I", os.path.dirname(header),
                            os.path.join(ROOT, "tests", "h5_direct_plan_host.c"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
    assert int(r.stdout.split(" cases")[0].split()[-1]) > 5000, r.stdout[-2000:]
