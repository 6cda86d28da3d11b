"""What the kernel-build tests (test_*_kernel_build.py, test_lanes_decoder_build.py) share: the Makefile's compiler and flags,
one translation unit compiled to gfx950 assembly, a kernel's metadata block and the compiler's resource remarks, and `make`'s
hazard check on one object.  A plain helper module: the tests keep their own bounds."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deltarice_amd", "csrc")


def _make_var(name):
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "--eval", f"print-var: ; @echo $({name})", "print-var"],
                         check=True, capture_output=True, text=True).stdout
    return out.strip().split()


def find_compiler():
    """(compiler, flags) of the Makefile; the body of the tests' module-scoped `compiler` fixture"""
    cc = _make_var("HIPCC")
    if not cc or not (os.path.exists(cc[0]) or shutil.which(cc[0])):
        pytest.skip("hipcc not found")
    return cc[0], _make_var("HIPFLAGS")


def compile_asm(compiler, tmp, src):
    """(assembly text, the compiler's remarks) of CSRC/src"""
    cc, flags = compiler
    out = tmp / (src + ".s")
    r = subprocess.run([cc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, src),
                                       "-o", str(out)], check=True, capture_output=True, text=True)
    return out.read_text(), r.stderr


def kernel_resources(asm, stderr, name):
    """(metadata block, resource remarks) of the kernel with the mangled `name`"""
    blocks = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    meta = [b for b in blocks if re.search(r"\.name:\s+" + re.escape(name) + r"\n", b)]
    assert len(meta) == 1, name
    remarks = re.search(r"Function Name: " + re.escape(name) + r"\b(.*?)(?=Function Name:|\Z)", stderr, re.S)
    assert remarks, name
    return meta[0], remarks.group(1)


def kernels_of(compiler, tmp, src, pattern, key=lambda m: m.group(2)):
    """{key(match): (metadata block, resource remarks)} of the kernels of CSRC/src whose mangled name is _ZN3drx<n><pattern>..."""
    asm, stderr = compile_asm(compiler, tmp, src)
    return {key(m): kernel_resources(asm, stderr, m.group(1)) for m in re.finditer(r"^(_ZN3drx\d+" + pattern + r"\w+):", asm, re.M)}


def _field(meta, key):
    m = re.search(r"\." + key + r":\s+(\d+)", meta)
    assert m, key
    return int(m.group(1))


def _remark(remarks, key):
    m = re.search(re.escape(key) + r":\s+(\d+)", remarks)
    assert m, key
    return int(m.group(1))


def resources(entry):
    """(vgpr_count, LDS bytes, private segment bytes) of a (metadata, remarks) entry"""
    meta = entry[0]
    return _field(meta, "vgpr_count"), _field(meta, "group_segment_fixed_size"), _field(meta, "private_segment_fixed_size")


def check_object_hazards(compiler, tmp_path, src):
    """The check `make` runs over every object before it links the library, on CSRC/src's; and that `make` builds it."""
    cc, flags = compiler
    obj = tmp_path / (os.path.splitext(src)[0] + ".o")
    subprocess.run([cc] + flags + ["-c", os.path.join(CSRC, src), "-o", str(obj)], check=True, capture_output=True, text=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_hazards.py"), str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    srcs = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "print-hip-srcs"], check=True, capture_output=True, text=True).stdout.split()
    assert "deltarice_amd/csrc/" + src in srcs, src + " is not among the Makefile's HIP_SRCS"
