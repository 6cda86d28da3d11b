"""CPU: the stream encoders keep their wave-uniform bookkeeping (ticket, waveform index, bit count, ring limits, the loop
conditions) in scalar registers ("Wave-uniform bookkeeping").  Compiles drx_encode_stream.hip to gfx950
assembly with the Makefile's compiler and flags and holds both k_encode_stream instantiations to:
  .vgpr_count <= 100   (114 while the wave index and the LDS-published ticket were vector values; 83 with this compiler now)
  saveexec    <= 300   (447 then: wave-uniform `if`s compiled as exec-mask regions; 257 now)
  no private segment (no scratch)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "deltarice_amd", "csrc", "drx_encode_stream.hip")


def _make_var(name):
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", ROOT, "--eval", f"print-var: ; @echo $({name})", "print-var"],
                         check=True, capture_output=True, text=True).stdout
    return out.strip().split()


def _hipcc():
    cc = _make_var("HIPCC")
    if not cc or not (os.path.exists(cc[0]) or shutil.which(cc[0])):
        pytest.skip("hipcc not found")
    return cc[0]


@pytest.fixture(scope="module")
def stream_asm(tmp_path_factory):
    hipcc = _hipcc()
    out = tmp_path_factory.mktemp("asm") / "drx_encode_stream.s"
    subprocess.run([hipcc] + _make_var("HIPFLAGS") + ["-S", "--cuda-device-only", SRC, "-o", str(out)], check=True,
                   capture_output=True, text=True)
    return out.read_text()


def _kernels(asm, mangled_prefix):
    """mangled name -> (body text, metadata block) of every kernel whose mangled name starts with `mangled_prefix`"""
    blocks = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    found = {}
    for m in re.finditer(r"^(" + mangled_prefix + r"\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = [b for b in blocks if re.search(r"\.name:\s+" + re.escape(name) + r"\n", b)]
        assert len(meta) == 1, name
        found[name] = (body.split(".section")[0], meta[0])
    return found


def _field(meta, key):
    m = re.search(r"\." + key + r":\s+(\d+)", meta)
    assert m, key
    return int(m.group(1))


def test_stream_encoders_keep_uniform_bookkeeping_scalar(stream_asm):
    ks = _kernels(stream_asm, "_ZN3drx15k_encode_streamI")
    assert len(ks) == 2, sorted(ks)  # the delta filter's instantiation and the general filter's
    for name, (body, meta) in ks.items():
        vgprs = _field(meta, "vgpr_count")
        saveexec = len(re.findall(r"^\s+s_\w*saveexec\w*\s", body, re.M))
        scratch = _field(meta, "private_segment_fixed_size")
        print(f"{name}: vgpr_count {vgprs}, saveexec {saveexec}, private segment {scratch}")
        assert vgprs <= 100, (name, vgprs)
        assert saveexec <= 300, (name, saveexec)
        assert scratch == 0, (name, scratch)
