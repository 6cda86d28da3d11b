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
import pytest

from kernel_build import _remark, check_object_hazards, find_compiler, kernels_of, resources

SRC = "drx_transcode.hip"
KERNELS = {"k_recode_sizesILb0EE": "sizes", "k_recode_sizesILb1EE": "sizes-all-k", "k_recode_packE": "pack"}


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def kernels(compiler, tmp_path_factory):
    """short name -> (metadata block, the compiler's resource remarks)"""
    found = kernels_of(compiler, tmp_path_factory.mktemp("asm"), SRC, r"(k_recode_(?:sizesILb[01]EE|packE))", key=lambda m: KERNELS[m.group(2)])
    assert sorted(found) == sorted(KERNELS.values()), sorted(found)
    return found


@pytest.mark.parametrize("short,per_cu,vgpr_max,lds_want", [("sizes", 9, 168, 16896), ("sizes-all-k", 9, 256, 16896), ("pack", 6, 256, 25088)])
def test_recode_kernel_resources(kernels, short, per_cu, vgpr_max, lds_want):
    meta, remarks = kernels[short]
    vgprs, lds, scratch = resources(kernels[short])
    print(f"{short}: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds == lds_want and lds * per_cu <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * per_cu <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= vgpr_max and _remark(remarks, "VGPRs") <= vgpr_max, vgprs


def test_transcode_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
