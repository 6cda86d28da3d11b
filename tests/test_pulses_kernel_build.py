"""CPU: what the compiler makes of the pulse kernels, by the method of
test_window_kernel_build.py.  Compiles drx_pulses.hip to gfx950 assembly with the Makefile's compiler and flags and holds
  k_find_pulses         LDS x 9 <= 163 840 bytes (the ring alone, 16 896 bytes, and nine wavefronts per CU fit the LDS), no
                        private segment (no scratch: the state machine's loop over a group's eight registers rotates them, so
                        every index is a constant), .vgpr_count <= 168 (three wavefronts on a SIMD, the occupancy
                        k_wave_stats and k_find_pulses are held to); 158 VGPRs, 16 896 bytes with this compiler now
  k_find_pulses_serial  no private segment
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import pytest

from kernel_build import _remark, check_object_hazards, find_compiler, kernels_of, resources

SRC = "drx_pulses.hip"


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def pulse_kernels(compiler, tmp_path_factory):
    """kernel (unmangled) -> (metadata block, the compiler's resource remarks)"""
    found = kernels_of(compiler, tmp_path_factory.mktemp("asm"), SRC, r"(k_find_pulses(?:_serial)?)E")
    assert sorted(found) == ["k_find_pulses", "k_find_pulses_serial"], sorted(found)
    return found


def test_find_pulses_resources(pulse_kernels):
    meta, remarks = pulse_kernels["k_find_pulses"]
    vgprs, lds, scratch = resources(pulse_kernels["k_find_pulses"])
    print(f"k_find_pulses: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds * 9 <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * 9 <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= 168 and _remark(remarks, "VGPRs") <= 168, vgprs


def test_find_pulses_serial_resources(pulse_kernels):
    meta, remarks = pulse_kernels["k_find_pulses_serial"]
    vgprs, lds, scratch = resources(pulse_kernels["k_find_pulses_serial"])
    print(f"k_find_pulses_serial: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch


def test_pulses_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
