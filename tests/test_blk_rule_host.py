"""CPU: the block geometry rules of deltarice_amd/csrc/drx_blocks.h -- nt_for_len (lanes per block), blk_segw_plan and
blk_segw_bits10 (stream words per lane) and blk_lane_cap (a lane's share of the staging buffer) -- compiled host-side into
tests/blk_rule_host.cpp's stand-alone program, whose output over a grid is compared line by line with the Python mirror of the
same rules in tests/block_cells.py: the mirror is what says which kernel instantiation every cell of
tests/test_gpu_block_forms_parameters.py runs."""
import os
import subprocess

import block_cells as bc
from kernel_build import CSRC, ROOT, find_compiler


def test_python_mirror_of_the_block_geometry_rules(tmp_path):
    cc, _ = find_compiler()
    exe = tmp_path / "blk_rule_host"
    # the header is HIP (device code beside the rules): the host half of a HIP compile, no device code, no GPU
    build = subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Werror", "-x", "hip", "--offload-host-only", "-I", CSRC,
                            os.path.join(ROOT, "tests", "blk_rule_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"{len(lines) - 1} lines" and len(lines) > 50000, lines[-1]
    seen = {"nt": set(), "sw": set(), "cap": set()}
    for line in lines[:-1]:
        what, *v = line.split()
        v = [int(t) for t in v]
        if what == "nt":
            wave_len, k, nt, plan = v
            assert (bc.nt_for_len(wave_len, k), bc.blk_segw_plan(k)) == (nt, plan), line
            seen["nt"].add(nt)
        elif what == "sw":
            assert bc.blk_segw_bits10(v[0]) == v[1], line
            seen["sw"].add(v[1])
        else:
            assert what == "cap" and bc.blk_lane_cap(v[0]) == v[1], line
            seen["cap"].add(v[1])
    assert seen == {"nt": {64, 128, 256}, "sw": {9, 11, 15, 19}, "cap": {76, 68, 60}}, seen
    # the three lengths of the table: which k take which lanes per block
    assert [k for k in range(16) if bc.nt_for_len(3000, k) == 64] == [0, 1, 2, 3, 4, 5, 6, 8, 9]
    assert all(bc.nt_for_len(3000, k) == 128 for k in (7, 10, 11, 12, 13, 14, 15))
    assert [bc.nt_for_len(6000, k) for k in range(16)] == [64] + [128] * 6 + [256] + [128] * 2 + [256] * 6
    assert all(bc.nt_for_len(20000, k) == 256 for k in range(16))
