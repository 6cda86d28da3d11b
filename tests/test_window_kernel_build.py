"""CPU: what the compiler makes of the window kernels, by the method of
test_stats_kernel_build.py.  Compiles drx_window.hip to gfx950 assembly with the Makefile's compiler and flags and holds
  k_decode_window         LDS x 9 <= 163 840 bytes (the ring alone, 16 896 bytes: the stores need no staging, and nine
                          wavefronts per CU fit the LDS), no private segment (no scratch), .vgpr_count <= 168 (three wavefronts
                          on a SIMD, twelve per CU: the registers bind, not the LDS); 158 VGPRs, 16 896 bytes with this
                          compiler now
  k_decode_window_serial  no private segment
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import pytest

from kernel_build import _remark, check_object_hazards, find_compiler, kernels_of, resources

SRC = "drx_window.hip"


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def window_kernels(compiler, tmp_path_factory):
    """kernel (unmangled) -> (metadata block, the compiler's resource remarks)"""
    found = kernels_of(compiler, tmp_path_factory.mktemp("asm"), SRC, r"(k_decode_window(?:_serial)?)E")
    assert sorted(found) == ["k_decode_window", "k_decode_window_serial"], sorted(found)
    return found


def test_decode_window_resources(window_kernels):
    meta, remarks = window_kernels["k_decode_window"]
    vgprs, lds, scratch = resources(window_kernels["k_decode_window"])
    print(f"k_decode_window: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds * 9 <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * 9 <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= 168 and _remark(remarks, "VGPRs") <= 168, vgprs


def test_decode_window_serial_resources(window_kernels):
    meta, remarks = window_kernels["k_decode_window_serial"]
    vgprs, lds, scratch = resources(window_kernels["k_decode_window_serial"])
    print(f"k_decode_window_serial: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch


def test_window_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
