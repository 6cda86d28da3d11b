"""CPU: what the compiler makes of k_decode_lanes ("whole lines").  Compiles drx_decode_kernels.hip to
gfx950 assembly with the Makefile's compiler and flags and holds all four instantiations (FUSED x GEN) to:
  LDS 26 112 bytes       (the ring and the transposition buffer: six wavefronts per CU)
  no private segment     (no scratch)
  .vgpr_count <= 256     (two wavefronts on a SIMD; 206 / 210 (GEN) with this compiler now, 162 / 164 with two 64-byte pieces)
and records the pair chain of the interior rounds' group (the basic block of eight pairs without the edge rounds' captures):
262 instructions, 217 of them VALU, as in the parent.  The shorter length chain (the negated code length as one v_sub behind a
select, no v_not between a pair's windows) was built and measured and is not in the kernel: it returned nothing
(profiles/lanes_lines_ab.txt), so nothing is asserted about v_not here."""
import re

import pytest

from kernel_build import _field, _remark, compile_asm, find_compiler, kernel_resources

PAIRS = 8  # per group of 16 samples


@pytest.fixture(scope="module")
def lanes_kernels(tmp_path_factory):
    """mangled name -> (body text, metadata block, the compiler's resource remarks) of the four instantiations"""
    asm, stderr = compile_asm(find_compiler(), tmp_path_factory.mktemp("asm"), "drx_decode_kernels.hip")
    found = {}
    for m in re.finditer(r"^(_ZN3drx14k_decode_lanesI\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        name, body = m.group(1), m.group(2)
        found[name] = (body.split(".section")[0],) + kernel_resources(asm, stderr, name)
    assert len(found) == 4, sorted(found)
    return found


def _instructions(block):
    return [ln.split()[0] for ln in block.splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]


def _interior_group(body):
    """The basic block of PAIRS pairs (three v_alignbit each) with the fewest instructions: the interior rounds' group."""
    blocks = [_instructions(b) for b in re.split(r"^\.LBB\d+_\d+:.*$", body, flags=re.M)]
    groups = [b for b in blocks if sum(i.startswith("v_alignbit") for i in b) == 3 * PAIRS]
    assert groups, "no basic block of eight pairs"
    return min(groups, key=len)


def test_lanes_decoder_resources(lanes_kernels):
    for name, (body, meta, remarks) in lanes_kernels.items():
        vgprs, lds, scratch = _field(meta, "vgpr_count"), _field(meta, "group_segment_fixed_size"), _field(meta, "private_segment_fixed_size")
        print(f"{name}: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
        assert lds == 26112 and _remark(remarks, "LDS Size [bytes/block]") == 26112, (name, lds)
        assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, (name, scratch)
        assert vgprs <= 256 and _remark(remarks, "VGPRs") <= 256, (name, vgprs)


def test_lanes_decoder_pair_chain(lanes_kernels):
    for name, (body, meta, remarks) in lanes_kernels.items():
        ins = _interior_group(body)
        at = [i for i, x in enumerate(ins) if x.startswith("v_alignbit")]
        assert len(at) == 3 * PAIRS, name
        between = []
        for p in range(PAIRS):  # a pair: source windows A and B, then the second sample's window
            lo, hi = at[3 * p + 1], at[3 * p + 2]
            between.append([x for x in ins[lo + 1:hi] if x.startswith("v_")])
        n_valu = sum(x.startswith("v_") for x in ins)
        print(f"{name}: interior group {len(ins)} instructions, {n_valu} VALU (parent: 262 / 217 without a general filter); "
              f"VALU between a pair's last source window and its second window: {[len(b) for b in between]}, "
              f"v_not among them: {sum(x.startswith('v_not') for b in between for x in b)}")
        if "ILb0ELb0E" in name or "ILb1ELb0E" in name:  # the delta filter's instantiations: no more work per group than the parent
            assert len(ins) <= 262 and n_valu <= 217, (name, len(ins), n_valu)
