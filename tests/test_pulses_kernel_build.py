"""CPU: what the compiler makes of the pulse kernels, by the method of
test_window_kernel_build.py.  Compiles drx_pulses.hip to gfx950 assembly with the Makefile's compiler and flags and holds
  k_find_pulses         LDS x 9 <= 163 840 bytes (the ring alone, 16 896 bytes, and nine wavefronts per CU fit the LDS), no
                        private segment (no scratch: the state machine's loop over a group's eight registers rotates them, so
                        every index is a constant), .vgpr_count <= 168 (three wavefronts on a SIMD, the occupancy
                        k_wave_stats and k_find_pulses are held to); 158 VGPRs, 16 896 bytes with this compiler now
  k_find_pulses_serial  no private segment
and that `make`'s hazard check of hand-written asm statements passes on the object file."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "deltarice_amd", "csrc", "drx_pulses.hip")


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
def pulse_kernels(compiler, tmp_path_factory):
    """kernel (unmangled) -> (metadata block, the compiler's resource remarks)"""
    cc, flags = compiler
    out = tmp_path_factory.mktemp("asm") / "drx_pulses.s"
    r = subprocess.run([cc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(out)],
                       check=True, capture_output=True, text=True)
    asm = out.read_text()
    blocks = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    found = {}
    for m in re.finditer(r"^(_ZN3drx\d+(k_find_pulses(?:_serial)?)E\w+):", asm, re.M):
        name, short = m.group(1), m.group(2)
        meta = [b for b in blocks if re.search(r"\.name:\s+" + re.escape(name) + r"\n", b)]
        assert len(meta) == 1, name
        remarks = re.search(r"Function Name: " + re.escape(name) + r"\b(.*?)(?=Function Name:|\Z)", r.stderr, re.S)
        assert remarks, name
        found[short] = (meta[0], remarks.group(1))
    assert sorted(found) == ["k_find_pulses", "k_find_pulses_serial"], sorted(found)
    return found


def _field(meta, key):
    m = re.search(r"\." + key + r":\s+(\d+)", meta)
    assert m, key
    return int(m.group(1))


def _remark(remarks, key):
    m = re.search(re.escape(key) + r":\s+(\d+)", remarks)
    assert m, key
    return int(m.group(1))


def test_find_pulses_resources(pulse_kernels):
    meta, remarks = pulse_kernels["k_find_pulses"]
    vgprs, lds, scratch = _field(meta, "vgpr_count"), _field(meta, "group_segment_fixed_size"), _field(meta, "private_segment_fixed_size")
    print(f"k_find_pulses: vgpr_count {vgprs}, LDS {lds}, private segment {scratch}")
    assert lds * 9 <= 163840 and _remark(remarks, "LDS Size [bytes/block]") * 9 <= 163840, lds
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch
    assert vgprs <= 168 and _remark(remarks, "VGPRs") <= 168, vgprs


def test_find_pulses_serial_resources(pulse_kernels):
    meta, remarks = pulse_kernels["k_find_pulses_serial"]
    scratch = _field(meta, "private_segment_fixed_size")
    print(f"k_find_pulses_serial: vgpr_count {_field(meta, 'vgpr_count')}, LDS {_field(meta, 'group_segment_fixed_size')}, private segment {scratch}")
    assert scratch == 0 and _remark(remarks, "ScratchSize [bytes/lane]") == 0, scratch


def test_pulses_object_passes_the_asm_hazard_check(compiler, tmp_path):
    """The check `make` runs over every object before it links the library, on this translation unit's."""
    cc, flags = compiler
    obj = tmp_path / "drx_pulses.o"
    subprocess.run([cc] + flags + ["-c", SRC, "-o", str(obj)], check=True, capture_output=True, text=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_hazards.py"), str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    srcs = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "print-hip-srcs"], check=True, capture_output=True, text=True).stdout.split()
    assert "deltarice_amd/csrc/drx_pulses.hip" in srcs, "drx_pulses.hip is not among the Makefile's HIP_SRCS"
