"""CPU: what the compiler makes of the stacking kernels, by the method of test_bins_kernel_build.py.
Compiles drx_stack.hip to gfx950 assembly with the Makefile's compiler and flags and holds
  k_wave_stack<512>    LDS x 2 <= 163 840 bytes (four reader rings, four transposition buffers and the accumulator of 512
                       positions: two workgroups, eight wavefronts per CU, the residency section 4.2m claims for widths up to 512)
  k_wave_stack<7168>   LDS x 1 <= 163 840 bytes (the accumulator of 7168 positions: one workgroup per CU)
  both                 no private segment (no scratch), .vgpr_count <= 192.  NOT the sibling lane kernels' 168: that bound keeps
                       three wavefronts on a SIMD, and these kernels' residency is the LDS's -- eight wavefronts per CU at most,
                       two on a SIMD, for which up to 256 registers cost no residency.  An argument from occupancy, not a
                       measurement: the kernel was not built under 168 and timed.  Both forms of a group (equal and distinct
                       origins) live in one loop: 183 and 184 VGPRs with this compiler now, and 192 is held so that a
                       change that drifts towards spilling shows
  k_wave_stack_serial  no private segment
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import pytest

from kernel_build import _remark, check_object_hazards, find_compiler, kernels_of, resources

SRC = "drx_stack.hip"
WORKGROUPS_PER_CU = {"512": 2, "7168": 1}  # by tile size


@pytest.fixture(scope="module")
def compiler():
    return find_compiler()


@pytest.fixture(scope="module")
def stack_kernels(compiler, tmp_path_factory):
    """kernel (unmangled, a template's argument behind it) -> (metadata block, the compiler's resource remarks)"""
    found = kernels_of(compiler, tmp_path_factory.mktemp("asm"), SRC, r"(k_wave_stack(?:ILi(\d+)E|_serial)E)",
                       key=lambda m: "k_wave_stack_serial" if m.group(3) is None else "k_wave_stack<" + m.group(3) + ">")
    assert sorted(found) == ["k_wave_stack<512>", "k_wave_stack<7168>", "k_wave_stack_serial"], sorted(found)
    return found


@pytest.mark.parametrize("tile", list(WORKGROUPS_PER_CU))
def test_wave_stack_resources(stack_kernels, tile):
    entry = stack_kernels["k_wave_stack<" + tile + ">"]
    remarks, per_cu = entry[1], WORKGROUPS_PER_CU[tile]
    vgprs, lds, scratch = resources(entry)
    print(f"k_wave_stack<{tile}>: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds * per_cu <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * per_cu <= 163840, lds
    assert lds * (per_cu + 1) > 163840, lds  # ... and no more than that: the residency is the LDS's
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= 192 and _remark(remarks, "VGPRs") <= 192, vgprs


def test_wave_stack_serial_resources(stack_kernels):
    entry = stack_kernels["k_wave_stack_serial"]
    vgprs, lds, scratch = resources(entry)
    print(f"k_wave_stack_serial: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert scratch == 0 and _remark(entry[1], "ScratchSize [bytes/lane]") == 0, scratch


def test_stack_object_passes_the_asm_hazard_check(compiler, tmp_path):
    check_object_hazards(compiler, tmp_path, SRC)
