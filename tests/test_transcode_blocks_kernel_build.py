"""CPU: what the compiler makes of k_trc_blocks ("block form"), by the method of
test_stats_blocks_kernel_build.py.  Compiles drx_transcode_blocks.hip and drx_blocks.hip to gfx950 assembly with the Makefile's
compiler and flags and holds, for every (NT, SW):
  no private segment (no scratch) in the kernel of the sizes and pack launches (k_trc_blocks<NT, SW, BlkTrcArgs>: one kernel, the
  launch is chosen by an argument) nor in the all-k sizes kernel of the estimate (k_trc_blocks<NT, SW, BlkTrcAllKArgs>);
  workgroups per CU -- by LDS (163 840 bytes per CU) and by .vgpr_count -- of both not below those of
  k_decode_blocks<NT, false, SW>, computed here: the pack launch drains its output through the decoder's own staging buffer, so
  equality with the decoder's figure is required of it and no workgroup per CU is given away;
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
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
    pack = kernels_of(compiler, tmp, "drx_transcode_blocks.hip", r"k_trc_blocksILi(\d+)ELi(\d+)ENS_10BlkTrcArgsEEE", key=geometry)
    allk = kernels_of(compiler, tmp, "drx_transcode_blocks.hip", r"k_trc_blocksILi(\d+)ELi(\d+)ENS_14BlkTrcAllKArgsEEE", key=geometry)
    decode = kernels_of(compiler, tmp, "drx_blocks.hip", r"k_decode_blocksILi(\d+)ELb0ELi(\d+)ELb0EE", key=geometry)
    assert sorted(pack) == sorted(allk) == sorted(decode) == sorted(GEOMETRIES), (sorted(pack), sorted(allk), sorted(decode))
    return pack, allk, decode


def per_cu(meta, nt):
    lds, vgprs = _field(meta, "group_segment_fixed_size"), _field(meta, "vgpr_count")
    by_lds = 163840 // lds
    waves_per_simd = 512 // (-(-vgprs // 8) * 8)  # registers are allotted in eights
    by_vgprs = waves_per_simd * 4 // (nt // 64)
    return min(by_lds, by_vgprs), lds, vgprs


@pytest.mark.parametrize("nt,sw", GEOMETRIES)
def test_transcode_blocks_resources(built, nt, sw):
    pack, allk, decode = built
    theirs, dlds, dvgprs = per_cu(decode[(nt, sw)][0], nt)
    for what, (meta, remarks) in (("sizes and pack", pack[(nt, sw)]), ("all-k sizes", allk[(nt, sw)])):
        scratch = _field(meta, "private_segment_fixed_size")
        mine, lds, vgprs = per_cu(meta, nt)
        print(f"k_trc_blocks<{nt}, {sw}> ({what}): vgpr_count {vgprs}, LDS {lds}, private segment {scratch}, {mine} workgroups per CU; "
              f"k_decode_blocks<{nt}, false, {sw}>: vgpr_count {dvgprs}, LDS {dlds}, {theirs} per CU")
        assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, (what, scratch)
        assert mine >= theirs, (what, mine, theirs)


def test_transcode_blocks_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, "drx_transcode_blocks.hip")
