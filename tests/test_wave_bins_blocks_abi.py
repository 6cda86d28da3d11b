"""CPU: the surface of drx_wave_bins' block form -- the header documents the context option "bins_impl" and no longer calls the
two form values and the two debug flags reserved, their values are what they were, and Context.set_option passes the key and
its value through to drx_ctx_set_option (over the recording library of tests/plan_standin.py)."""
import os
import re

from plan_standin import RecordingLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()


def test_the_header_documents_the_option():
    txt = header()
    assert '"bins_impl"' in txt
    options = txt[txt.index("Tuning / diagnostics."):txt.index("#define DRX_DBG_BINS_LANES")]
    assert re.search(r'"bins_impl"\s+0 \(default\)', options), options
    # ... says that the block form is not the default and that flipping it is a follow-up
    bins = txt[:txt.index("#define DRX_BIN_SUM")]
    assert "BY DEFAULT" in bins and "follow-up" in bins


def test_the_defines_keep_their_values_and_are_not_reserved():
    from deltarice_amd import _lib
    txt = header()
    lines = {m.group(1): m.group(0) for m in re.finditer(r"^#define DRX_(\w+) \d+u\b.*$", txt, flags=re.M)}
    want = {"BINS_FORM_LANES": 1, "BINS_FORM_BLOCKS": 2, "BINS_FORM_FALLBACK_ALL": 4, "DBG_BINS_LANES": 64, "DBG_BINS_ALL_FALLBACK": 128,
            "PATH_BINS": 16384}
    for name, value in want.items():
        assert int(re.search(r" (\d+)u\b", lines[name]).group(1)) == value == getattr(_lib, name), name
        assert "reserved" not in lines[name], lines[name]


def test_set_option_passes_the_key_through():
    from deltarice_amd import codec

    class Ctx:
        lib, _h = RecordingLib(), 7
        _check = staticmethod(lambda st: None)

    for value in (1, 0):
        codec.Context.set_option(Ctx, "bins_impl", value)
    assert Ctx.lib.calls == [("drx_ctx_set_option", (7, b"bins_impl", 1)), ("drx_ctx_set_option", (7, b"bins_impl", 0))]
    for name in ("wave_bins", "last_bins_form"):
        assert "bins_impl" in getattr(codec.Plan, name).__doc__, name


def test_a_null_context():
    from deltarice_amd import _lib
    assert _lib.load().drx_ctx_set_option(None, b"bins_impl", 1) == 1
