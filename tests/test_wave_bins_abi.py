"""CPU: the surface of drx_wave_bins -- exports, signatures, the DRX_BIN_* columns, DRX_PATH_BINS, the two debug flags and the
DRX_BINS_FORM_* values agree between the header, the library, deltarice_amd._lib and the package; a NULL plan; the Python
entry's refusals and a closed plan."""
import os
import re

import pytest

from plan_standin import plan as _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()


def test_exports_signatures_and_constants():
    from deltarice_amd import _lib
    import deltarice_amd as dr
    lib = _lib.load()
    for name in ("drx_wave_bins", "drx_wave_bins_with_wave_words", "drx_plan_last_bins_form", "drx_plan_last_bins_listed"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    plain, sideband = _lib.SIGNATURES["drx_wave_bins"][1], _lib.SIGNATURES["drx_wave_bins_with_wave_words"][1]
    assert len(plain) == 11 and len(sideband) == 12  # the side-band form has one argument more
    assert sideband[:4] == plain[:4] and sideband[5:] == plain[4:]  # ... behind d_chunk_word_off, as in the other pairs
    txt = header()
    cols = {k: int(v) for k, v in re.findall(r"^#define DRX_BIN_(\w+) (\d+)\b", txt, flags=re.M)}
    assert cols == {"SUM": 0, "SUMSQ": 1, "MIN": 2, "MAX": 3, "COLS": 4}
    for name, value in cols.items():
        assert getattr(_lib, "BIN_" + name) == value == getattr(dr, "BIN_" + name), name
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(\w+) (\d+)u\b", txt, flags=re.M)}
    assert defs["PATH_BINS"] == 16384 == _lib.PATH_BINS == dr.PATH_BINS
    assert (defs["BINS_FORM_LANES"], defs["BINS_FORM_BLOCKS"], defs["BINS_FORM_FALLBACK_ALL"]) == (1, 2, 4)
    assert (_lib.BINS_FORM_LANES, _lib.BINS_FORM_BLOCKS, _lib.BINS_FORM_FALLBACK_ALL) == (1, 2, 4)
    assert (dr.BINS_FORM_LANES, dr.BINS_FORM_BLOCKS, dr.BINS_FORM_FALLBACK_ALL) == (1, 2, 4)
    for decl in ("drx_status drx_wave_bins(", "drx_status drx_wave_bins_with_wave_words(",
                 "uint32_t drx_plan_last_bins_form(const drx_plan *plan);", "uint32_t drx_plan_last_bins_listed(const drx_plan *plan);",
                 "after drx_wave_bins: ms = { header-chain walk, everything behind the walk, 0, whole call }"):
        assert decl in txt, decl


def test_the_two_flags_are_single_bits_of_their_own():
    from deltarice_amd import _lib
    import deltarice_amd as dr
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(\w+) (\d+)u\b", header(), flags=re.M)}
    flags = {k: v for k, v in defs.items() if k.startswith("DBG_")}
    for name in ("DBG_BINS_LANES", "DBG_BINS_ALL_FALLBACK"):
        v = flags[name]
        assert v and v & (v - 1) == 0 and v < 1 << 32, name
        assert getattr(_lib, name) == v == getattr(dr, name), name
        assert [k for k, o in flags.items() if o == v] == [name], name
    # no two paths and no two debug flags share a bit
    for prefix in ("PATH_", "DBG_"):
        values = [v for k, v in defs.items() if k.startswith(prefix)]
        assert len(set(values)) == len(values) and all(v & (v - 1) == 0 for v in values), prefix


def test_a_null_plan():
    from deltarice_amd import _lib
    lib = _lib.load()
    assert lib.drx_wave_bins(None, None, 0, None, None, 1, 0, 1, 1, None, 4) == 1
    assert lib.drx_wave_bins_with_wave_words(None, None, 0, None, None, None, 1, 0, 1, 1, None, 4) == 1
    assert lib.drx_plan_last_bins_form(None) == 0
    assert lib.drx_plan_last_bins_listed(None) == 0


def test_python_entry_refusals_and_a_closed_plan():
    import torch
    from deltarice_amd import DeltaRiceError, _lib
    plan = _plan()
    words, off = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    refused = {
        "bin 0": dict(bin=0),
        "bin -1": dict(bin=-1),
        "bin 2^32": dict(bin=1 << 32),
        "n_bins -1": dict(n_bins=-1),
        "n_bins 2^32": dict(n_bins=1 << 32),
        "offset": dict(offset=1 << 63),
        "start an int": dict(start=5),
        "start dtype": dict(start=torch.zeros(3, dtype=torch.int32)),
        "start 2-D": dict(start=torch.zeros((3, 1), dtype=torch.int64)),
        "start waves": dict(start=torch.zeros(4, dtype=torch.int64)),
        "start device": dict(start=torch.zeros(3, dtype=torch.int64, device="meta")),
        "start stride 0": dict(start=torch.zeros(1, dtype=torch.int64).expand(3)),
        "out too small": dict(n_bins=2, out=torch.zeros(3 * 2 * 4 - 1, dtype=torch.int64)),
        "out dtype": dict(n_bins=2, out=torch.zeros(24, dtype=torch.int32)),
        "out device": dict(n_bins=2, out=torch.zeros(24, dtype=torch.int64, device="meta")),
        "words dtype": dict(words=torch.zeros(8, dtype=torch.int64)),
        "wave_words length": dict(wave_words=torch.zeros(2, dtype=torch.int32)),
    }
    for what, kw in refused.items():
        w, b = kw.pop("words", words), kw.pop("bin", 10)
        with pytest.raises(DeltaRiceError) as e:
            plan.wave_bins_async(w, off, b, **kw)
        assert e.value.status == 1, what
    # no bin: an empty result, and the library is not called (tests/test_codec_calls.py holds the stand-in's record to that)
    assert plan.wave_bins_async(words, off, 10, 0).shape == (3, 0, _lib.BIN_COLS)
    # the default n_bins covers the plan's longest waveform (100 samples) from the offset
    assert plan.wave_bins_async(words, off, 10, offset=100).shape == (3, 0, _lib.BIN_COLS)
    assert plan.wave_bins_async(words, off, 10, offset=1000).shape == (3, 0, _lib.BIN_COLS)
    # a closed plan, in every entry
    plan._h = None
    for call in (lambda: plan.wave_bins(None, 10), lambda: plan.wave_bins_async(None, None, 10), plan.last_bins_form, plan.last_bins_listed):
        with pytest.raises(DeltaRiceError) as e:
            call()
        assert e.value.status == 1
