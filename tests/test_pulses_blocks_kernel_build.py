"""CPU: what the compiler makes of k_pulses_blocks, by the method of test_stats_blocks_kernel_build.py.
Compiles drx_pulses_blocks.hip and drx_blocks.hip to gfx950 assembly with the Makefile's compiler and flags and holds, for every
instantiation k_pulses_blocks<NT, SW>:
  no private segment (no scratch);
  LDS not above that of k_decode_blocks<NT, false, SW>, the delta-filter decoder of the same geometry (the kernel shares that
  decoder's phase 1 and its one LDS object);
and records .vgpr_count beside the decoder's and the workgroups per CU that both allow (163 840 bytes of LDS per CU; 512
registers per SIMD lane, NT / 64 wavefronts over four SIMDs); and that `make`'s hazard check of hand-written asm statements
passes on the object file."""
import pytest

from kernel_build import _field, _remark, check_object_hazards, find_compiler, kernels_of

GEOMETRIES = [(nt, sw) for nt in (64, 128, 256) for sw in (9, 11, 15, 19)]


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def built(compiler, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    geometry = lambda m: (int(m.group(2)), int(m.group(3)))  # noqa: E731
    pulses = kernels_of(compiler, tmp, "drx_pulses_blocks.hip", r"k_pulses_blocksILi(\d+)ELi(\d+)EE", key=geometry)
    decode = kernels_of(compiler, tmp, "drx_blocks.hip", r"k_decode_blocksILi(\d+)ELb0ELi(\d+)ELb0EE", key=geometry)
    assert sorted(pulses) == sorted(decode) == sorted(GEOMETRIES), (sorted(pulses), sorted(decode))
    return pulses, decode


def per_cu(meta, nt):
    lds, vgprs = _field(meta, "group_segment_fixed_size"), _field(meta, "vgpr_count")
    by_lds = 163840 // lds
    waves_per_simd = 512 // (-(-vgprs // 8) * 8)  # registers are allotted in eights
    by_vgprs = waves_per_simd * 4 // (nt // 64)
    return min(by_lds, by_vgprs), lds, vgprs


@pytest.mark.parametrize("nt,sw", GEOMETRIES)
def test_pulses_blocks_resources(built, nt, sw):
    pulses, decode = built
    meta, remarks = pulses[(nt, sw)]
    scratch = _field(meta, "private_segment_fixed_size")
    mine, lds, vgprs = per_cu(meta, nt)
    theirs, dlds, dvgprs = per_cu(decode[(nt, sw)][0], nt)
    print(f"k_pulses_blocks<{nt}, {sw}>: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}, {mine} workgroups per CU; "
          f"k_decode_blocks<{nt}, false, {sw}>: vgpr_count {dvgprs}, LDS {dlds}, {theirs} per CU")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert lds <= dlds, (lds, dlds)


def test_pulses_blocks_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, "drx_pulses_blocks.hip")
