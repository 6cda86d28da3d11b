"""CPU: what the compiler makes of k_stats_blocks, by the method of test_stats_kernel_build.py.
Compiles drx_stats_blocks.hip and drx_blocks.hip to gfx950 assembly with the Makefile's compiler and flags and holds, for every
instantiation k_stats_blocks<NT, SW>:
  no private segment (no scratch);
  workgroups per CU -- by LDS (163 840 bytes per CU) and by .vgpr_count (512 registers per SIMD lane, NT / 64 wavefronts over
  four SIMDs) -- not below those of k_decode_blocks<NT, false, SW>, the delta-filter decoder of the same geometry: the kernel
  shares that decoder's phase 1 and must not be the reason fewer blocks are resident;
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import os
import re
import subprocess
import sys

import pytest

from test_stats_kernel_build import _field, _make_var, _remark, compiler  # noqa: F401  (compiler: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deltarice_amd", "csrc")
GEOMETRIES = [(nt, sw) for nt in (64, 128, 256) for sw in (9, 11, 15, 19)]


def kernels_of(compiler, tmp, src, pattern):
    """{(NT, SW): (metadata block, the compiler's resource remarks)} of the kernels of `src` whose mangled name matches."""
    cc, flags = compiler
    out = tmp / (os.path.basename(src) + ".s")
    r = subprocess.run([cc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(out)],
                       check=True, capture_output=True, text=True)
    asm = out.read_text()
    blocks = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    found = {}
    for m in re.finditer(r"^(_ZN3drx\d+" + pattern + r"\w+):", asm, re.M):
        name = m.group(1)
        meta = [b for b in blocks if re.search(r"\.name:\s+" + re.escape(name) + r"\n", b)]
        assert len(meta) == 1, name
        remarks = re.search(r"Function Name: " + re.escape(name) + r"\b(.*?)(?=Function Name:|\Z)", r.stderr, re.S)
        assert remarks, name
        found[(int(m.group(2)), int(m.group(3)))] = (meta[0], remarks.group(1))
    return found


@pytest.fixture(scope="module")
def built(compiler, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    stats = kernels_of(compiler, tmp, os.path.join(CSRC, "drx_stats_blocks.hip"), r"k_stats_blocksILi(\d+)ELi(\d+)EE")
    decode = kernels_of(compiler, tmp, os.path.join(CSRC, "drx_blocks.hip"), r"k_decode_blocksILi(\d+)ELb0ELi(\d+)ELb0EE")
    assert sorted(stats) == sorted(decode) == sorted(GEOMETRIES), (sorted(stats), sorted(decode))
    return stats, decode


def per_cu(meta, nt):
    lds, vgprs = _field(meta, "group_segment_fixed_size"), _field(meta, "vgpr_count")
    by_lds = 163840 // lds
    waves_per_simd = 512 // (-(-vgprs // 8) * 8)  # registers are allotted in eights
    by_vgprs = waves_per_simd * 4 // (nt // 64)
    return min(by_lds, by_vgprs), lds, vgprs


@pytest.mark.parametrize("nt,sw", GEOMETRIES)
def test_stats_blocks_resources(built, nt, sw):
    stats, decode = built
    meta, remarks = stats[(nt, sw)]
    scratch = _field(meta, "private_segment_fixed_size")
    mine, lds, vgprs = per_cu(meta, nt)
    theirs, dlds, dvgprs = per_cu(decode[(nt, sw)][0], nt)
    print(f"k_stats_blocks<{nt}, {sw}>: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}, {mine} workgroups per CU; "
          f"k_decode_blocks<{nt}, false, {sw}>: vgpr_count {dvgprs}, LDS {dlds}, {theirs} per CU")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert mine >= theirs, (mine, theirs)


def test_stats_blocks_object_passes_the_asm_hazard_check(compiler, tmp_path):
    """The check `make` runs over every object before it links the library, on this translation unit's."""
    cc, flags = compiler
    obj = tmp_path / "drx_stats_blocks.o"
    subprocess.run([cc] + flags + ["-c", os.path.join(CSRC, "drx_stats_blocks.hip"), "-o", str(obj)], check=True, capture_output=True, text=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_hazards.py"), str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    srcs = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "print-hip-srcs"], check=True, capture_output=True, text=True).stdout.split()
    assert "deltarice_amd/csrc/drx_stats_blocks.hip" in srcs, "drx_stats_blocks.hip is not among the Makefile's HIP_SRCS"
