"""CPU: what the compiler makes of the binned-statistics kernels, by the method of
test_stats_kernel_build.py.  Compiles drx_bins.hip to gfx950 assembly with the Makefile's compiler and flags and holds
  k_wave_bins         LDS x 9 <= 163 840 bytes (the reader's ring alone, 16 896 bytes: nine wavefronts per CU fit the LDS),
                      no private segment (no scratch), .vgpr_count <= 168 (three wavefronts on a SIMD, what k_wave_stats is
                      held to); 160 VGPRs, 16 896 bytes with this compiler now
  k_wave_bins_serial  no private segment
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import pytest

from kernel_build import _remark, check_object_hazards, find_compiler, kernels_of, resources

SRC = "drx_bins.hip"


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def bins_kernels(compiler, tmp_path_factory):
    """kernel (unmangled) -> (metadata block, the compiler's resource remarks)"""
    found = kernels_of(compiler, tmp_path_factory.mktemp("asm"), SRC, r"(k_wave_bins(?:_serial)?)E")
    assert sorted(found) == ["k_wave_bins", "k_wave_bins_serial"], sorted(found)
    return found


def test_wave_bins_resources(bins_kernels):
    meta, remarks = bins_kernels["k_wave_bins"]
    vgprs, lds, scratch = resources(bins_kernels["k_wave_bins"])
    print(f"k_wave_bins: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds * 9 <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * 9 <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= 168 and _remark(remarks, "VGPRs") <= 168, vgprs


def test_wave_bins_serial_resources(bins_kernels):
    meta, remarks = bins_kernels["k_wave_bins_serial"]
    vgprs, lds, scratch = resources(bins_kernels["k_wave_bins_serial"])
    print(f"k_wave_bins_serial: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch


def test_bins_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
