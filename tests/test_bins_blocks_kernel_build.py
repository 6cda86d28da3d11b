"""CPU: what the compiler makes of k_bins_blocks, by the method of test_stats_blocks_kernel_build.py.
Compiles drx_bins_blocks.hip and drx_blocks.hip to gfx950 assembly with the Makefile's compiler and flags and holds, for every
instantiation k_bins_blocks<NT, SW>:
  no private segment (no scratch);
  workgroups per CU -- by LDS (163 840 bytes per CU) and by .vgpr_count (512 registers per SIMD lane, NT / 64 wavefronts over
  four SIMDs) -- not below those of k_decode_blocks<NT, false, SW>, the delta-filter decoder of the same geometry: the table of
  the bins a block meets lies in LDS the body already has, and the kernel must not be the reason fewer blocks are resident;
that the kernels beside it (the fill, the list's, the lane kernel over the list) have no private segment either;
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import pytest

from kernel_build import _field, _remark, check_object_hazards, find_compiler, kernels_of
from test_stats_blocks_kernel_build import GEOMETRIES, per_cu

SRC = "drx_bins_blocks.hip"


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def built(compiler, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    geometry = lambda m: (int(m.group(2)), int(m.group(3)))  # noqa: E731
    bins = kernels_of(compiler, tmp, SRC, r"k_bins_blocksILi(\d+)ELi(\d+)EE", key=geometry)
    decode = kernels_of(compiler, tmp, "drx_blocks.hip", r"k_decode_blocksILi(\d+)ELb0ELi(\d+)ELb0EE", key=geometry)
    others = kernels_of(compiler, tmp, SRC, r"(k_bins_fill|k_bins_blocks_finish|k_wave_bins_list)E")
    assert sorted(bins) == sorted(decode) == sorted(GEOMETRIES), (sorted(bins), sorted(decode))
    assert sorted(others) == ["k_bins_blocks_finish", "k_bins_fill", "k_wave_bins_list"], sorted(others)
    return bins, decode, others


@pytest.mark.parametrize("nt,sw", GEOMETRIES)
def test_bins_blocks_resources(built, nt, sw):
    bins, decode, _ = built
    meta, remarks = bins[(nt, sw)]
    scratch = _field(meta, "private_segment_fixed_size")
    mine, lds, vgprs = per_cu(meta, nt)
    theirs, dlds, dvgprs = per_cu(decode[(nt, sw)][0], nt)
    print(f"k_bins_blocks<{nt}, {sw}>: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}, {mine} workgroups per CU; "
          f"k_decode_blocks<{nt}, false, {sw}>: vgpr_count {dvgprs}, LDS {dlds}, {theirs} per CU")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert lds == dlds, (lds, dlds)  # no LDS beyond what the body has
    assert mine >= theirs, (mine, theirs)


def test_the_kernels_beside_the_blocks_have_no_private_segment(built):
    for name, (meta, remarks) in built[2].items():
        scratch = _field(meta, "private_segment_fixed_size")
        assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, (name, scratch)


def test_bins_blocks_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
