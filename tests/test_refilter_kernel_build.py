"""CPU: what the compiler makes of the re-filter kernels, by the method of
test_transcode_kernel_build.py.  Compiles drx_refilter.hip to gfx950 assembly with the Makefile's compiler and flags and holds
the fast pair to the bounds of the re-code kernels it shares its bodies with
  k_refilter_sizes<false>  LDS 16 896 bytes (the input ring alone), x 9 <= 163 840, no private segment, .vgpr_count <= 168;
                           152 VGPRs with this compiler now (k_recode_sizes<false>: 148)
  k_refilter_sizes<true>   the same LDS, no private segment, .vgpr_count <= 256 -- the sixteen counts fit one launch; 232 now
  k_refilter_pack          LDS 25 088 bytes (input and output ring), x 6 <= 163 840, no private segment, .vgpr_count <= 256;
                           160 now (k_recode_pack: 156)
that the filter stage is 24-bit multiply-adds (seven per sample and code path, no full 32-bit multiply added to the parse),
and that `make`'s hazard check of hand-written asm statements passes on the object file.  The serial kernels are correct, not
tuned; their only requirement is LDS x wavefronts per CU <= 163 840.  Their figures with this compiler:
  k_refilter_sizes_serial<false>  LDS  8 192 (the history column) x 20 wavefronts per CU, 30 VGPRs, no private segment
  k_refilter_sizes_serial<true>   LDS  8 192 x 20, 62 VGPRs, no private segment
  k_refilter_pack_serial          LDS 16 384 (history column and output ring) x 10, 64 VGPRs, no private segment"""
import re

import pytest

from kernel_build import _remark, check_object_hazards, compile_asm, find_compiler, kernel_resources, resources

SRC = "drx_refilter.hip"
KERNELS = {"k_refilter_sizesILb0EE": "sizes", "k_refilter_sizesILb1EE": "sizes-all-k", "k_refilter_packE": "pack",
           "k_refilter_sizes_serialILb0EE": "serial-sizes", "k_refilter_sizes_serialILb1EE": "serial-sizes-all-k",
           "k_refilter_pack_serialE": "serial-pack"}


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def unit(compiler, tmp_path_factory):
    """(assembly text, the compiler's remarks)"""
    return compile_asm(compiler, tmp_path_factory.mktemp("asm"), SRC)


@pytest.fixture(scope="module")
def kernels(unit):
    """short name -> (metadata block, the compiler's resource remarks)"""
    asm, stderr = unit
    found = {}
    for m in re.finditer(r"^(_ZN3drx\d+(k_refilter_(?:sizes(?:_serial)?ILb[01]EE|pack(?:_serial)?E))\w+):", asm, re.M):
        found[KERNELS[m.group(2)]] = kernel_resources(asm, stderr, m.group(1))
    assert sorted(found) == sorted(KERNELS.values()), sorted(found)
    return found


@pytest.mark.parametrize("short,per_cu,vgpr_max,lds_want", [("sizes", 9, 168, 16896), ("sizes-all-k", 9, 256, 16896), ("pack", 6, 256, 25088)])
def test_refilter_kernel_resources(kernels, short, per_cu, vgpr_max, lds_want):
    meta, remarks = kernels[short]
    vgprs, lds, scratch = resources(kernels[short])
    print(f"{short}: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds == lds_want and lds * per_cu <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * per_cu <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= vgpr_max and _remark(remarks, "VGPRs") <= vgpr_max, vgprs


@pytest.mark.parametrize("short,per_cu", [("serial-sizes", 20, ), ("serial-sizes-all-k", 20), ("serial-pack", 10)])
def test_refilter_serial_kernels_fit_the_lds(kernels, short, per_cu):
    meta, remarks = kernels[short]
    vgprs, lds, scratch = resources(kernels[short])
    print(f"{short}: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds * per_cu <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * per_cu <= 163840, lds
    assert vgprs <= 512 * 4 // per_cu, vgprs  # (the registers allow those wavefronts: per_cu / 4 on a SIMD)


def test_refilter_stage_is_24_bit_multiply_adds(unit):
    """the fast kernels add no 32-bit multiply to the parse they share with the re-code kernels: the filter stage is
    v_mad_u32_u24, seven per sample in every code path that takes a sample"""
    asm = unit[0]
    for name in ("k_refilter_sizesILb0EE", "k_refilter_packE"):
        m = re.search(r"^_ZN3drx\d+" + name + r"\w+:", asm, re.M)
        assert m, name
        body = asm[m.end():asm.index(".Lfunc_end", m.end())]
        mads = len(re.findall(r"\bv_mad_u32_u24\b", body))
        assert mads >= 7 and mads % 7 == 0, (name, mads)


def test_refilter_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
