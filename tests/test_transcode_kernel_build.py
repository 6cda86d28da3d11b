"""CPU: what the compiler makes of the re-coding kernels, by the method of
test_stats_kernel_build.py.  Compiles drx_transcode.hip to gfx950 assembly with the Makefile's compiler and flags and holds
  k_recode_sizes<false>  LDS x 9 <= 163 840 bytes (the input ring alone, 16 896 bytes), no private segment (no scratch),
                         .vgpr_count <= 168 (three wavefronts on a SIMD); 148 VGPRs with this compiler now
  k_recode_sizes<true>   the same LDS, no private segment, .vgpr_count <= 256 (sixteen 64-bit counts and their group sums:
                         two wavefronts on a SIMD, eight per CU); 234 now
  k_recode_pack          LDS x 6 <= 163 840 bytes (an input ring of 64 and an output ring of 32 words a lane, 25 088 bytes:
                         the LDS allows six wavefronts per CU), no private segment, .vgpr_count <= 256 (two wavefronts on a
                         SIMD: the registers never allow fewer than the LDS does); 156 now
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "deltarice_amd", "csrc", "drx_transcode.hip")
KERNELS = {"k_recode_sizesILb0EE": "sizes", "k_recode_sizesILb1EE": "sizes-all-k", "k_recode_packE": "pack"}


def _make_var(name):
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "--eval", f"print-var: ; @echo $({name})", "print-var"],
                         check=True, capture_output=True, text=True).stdout
    return out.strip().split()


@pytest.fixture(scope="module")
def compiler():
    cc = _make_var("HIPCC")
    if not cc or not (os.path.exists(cc[0]) or shutil.which(cc[0])):
        pytest.skip("hipcc not found")
    return cc[0], _make_var("HIPFLAGS")


@pytest.fixture(scope="module")
def kernels(compiler, tmp_path_factory):
    """short name -> (metadata block, the compiler's resource remarks)"""
    cc, flags = compiler
    out = tmp_path_factory.mktemp("asm") / "drx_transcode.s"
    r = subprocess.run([cc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(out)],
                       check=True, capture_output=True, text=True)
    asm = out.read_text()
    blocks = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    found = {}
    for m in re.finditer(r"^(_ZN3drx\d+(k_recode_(?:sizesILb[01]EE|packE))\w+):", asm, re.M):
        name, short = m.group(1), KERNELS[m.group(2)]
        meta = [b for b in blocks if re.search(r"\.name:\s+" + re.escape(name) + r"\n", b)]
        assert len(meta) == 1, name
        remarks = re.search(r"Function Name: " + re.escape(name) + r"\b(.*?)(?=Function Name:|\Z)", r.stderr, re.S)
        assert remarks, name
        found[short] = (meta[0], remarks.group(1))
    assert sorted(found) == sorted(KERNELS.values()), sorted(found)
    return found


def _field(meta, key):
    m = re.search(r"\." + key + r":\s+(\d+)", meta)
    assert m, key
    return int(m.group(1))


def _remark(remarks, key):
    m = re.search(re.escape(key) + r":\s+(\d+)", remarks)
    assert m, key
    return int(m.group(1))


@pytest.mark.parametrize("short,per_cu,vgpr_max,lds_want", [("sizes", 9, 168, 16896), ("sizes-all-k", 9, 256, 16896), ("pack", 6, 256, 25088)])
def test_recode_kernel_resources(kernels, short, per_cu, vgpr_max, lds_want):
    meta, remarks = kernels[short]
    vgprs, lds, scratch = _field(meta, "vgpr_count"), _field(meta, "group_segment_fixed_size"), _field(meta, "private_segment_fixed_size")
    print(f"{short}: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds == lds_want and lds * per_cu <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * per_cu <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= vgpr_max and _remark(remarks, "VGPRs") <= vgpr_max, vgprs


def test_transcode_object_passes_the_asm_hazard_check(compiler, tmp_path):
    """The check `make` runs over every object before it links the library, on this translation unit's."""
    cc, flags = compiler
    obj = tmp_path / "drx_transcode.o"
    subprocess.run([cc] + flags + ["-c", SRC, "-o", str(obj)], check=True, capture_output=True, text=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_hazards.py"), str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    srcs = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "print-hip-srcs"], check=True, capture_output=True, text=True).stdout.split()
    assert "deltarice_amd/csrc/drx_transcode.hip" in srcs, "drx_transcode.hip is not among the Makefile's HIP_SRCS"
