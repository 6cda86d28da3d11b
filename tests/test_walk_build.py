"""CPU: where the compiler puts the LDS block walker's chase loop (walk_chunk_block() of drx_walk.h) in k_walk_block and
k_walk_block_only.  The loop is one wavefront's chain of dependent LDS reads and scalar branches, and its place inside a 64-byte
line of code decides its speed: with the loop's backward branch landing 56 bytes into a line (the loop's first compare 4 bytes
into the next) k_walk_block takes 3.55 ms on 25 chunks of 14 M samples at L = 512, four bytes earlier 3.87 (measured:
profiles/walk_refactor_ab.txt, section 3c).  The source holds the place with an aligned line plus kChasePad s_nop in front of
the block loop, run once per chunk -- a statement directly at the chase would run once per block, which was measured too and
costs the 0.2 % that put the kernel beyond the parent's spread.  The distance from the statement to the loop is therefore the
compiler's: this file compiles drx_walk.hip with the Makefile's compiler and flags and fails when a change to the code between
them, or another compiler, has moved the loop.  Then choose kChasePad so that this test passes; the place it holds is the
measured one."""
import importlib.util
import os
import re
import subprocess

import pytest

from kernel_build import CSRC, ROOT, find_compiler

spec = importlib.util.spec_from_file_location("check_asm_hazards", os.path.join(ROOT, "tools", "check_asm_hazards.py"))
hazards = importlib.util.module_from_spec(spec)
spec.loader.exec_module(hazards)

WANT = 56  # bytes into a 64-byte line: where the chase loop's backward branch lands


@pytest.fixture(scope="module")
def walk_disassembly(tmp_path_factory):
    cc, flags = find_compiler()
    obj = tmp_path_factory.mktemp("obj") / "drx_walk.o"
    subprocess.run([cc] + flags + ["-c", os.path.join(CSRC, "drx_walk.hip"), "-o", str(obj)], check=True, capture_output=True, text=True)
    kernels, cur = {}, None
    for line in hazards.disassemble(str(obj)):
        m = re.match(r"^[0-9a-f]+ <(\w+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return kernels


@pytest.mark.parametrize("kernel", ["k_walk_blockE", "k_walk_block_onlyE"])
def test_chase_loop_stays_where_it_is_fast(walk_disassembly, kernel):
    body = [v for k, v in walk_disassembly.items() if kernel in k]
    assert len(body) == 1, sorted(walk_disassembly)
    body = body[0]
    # the chase: the kernel's last v_readfirstlane (the header read out of LDS); its loop closes with the next backward s_branch
    at = max(i for i, (_, op, _) in enumerate(body) if op == "v_readfirstlane_b32")
    back = next((a, int(arg)) for a, op, arg in body[at:] if op == "s_branch" and int(arg) >= 0x8000)
    target = back[0] + 4 + 4 * (back[1] - 0x10000)
    print(f"{kernel}: the chase loop's backward branch at {back[0]:#x} lands at {target:#x}, {target % 64} bytes into its line")
    assert target % 64 == WANT, (kernel, hex(target), target % 64)
