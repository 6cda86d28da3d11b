"""CPU: the surface of drx_wave_stack -- exports, signatures, the DRX_STACK_* columns and DRX_PATH_STACK agree between the header,
the library, deltarice_amd._lib and the package; a NULL plan; what the Python entry passes on, its refusals and a closed plan."""
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
    for name in ("drx_wave_stack", "drx_wave_stack_with_wave_words"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    plain, sideband = _lib.SIGNATURES["drx_wave_stack"][1], _lib.SIGNATURES["drx_wave_stack_with_wave_words"][1]
    assert len(plain) == 11 and len(sideband) == 12  # the side-band form has one argument more
    assert sideband[:4] == plain[:4] and sideband[5:] == plain[4:]  # ... behind d_chunk_word_off, as in the other pairs
    txt = header()
    cols = {k: int(v) for k, v in re.findall(r"^#define DRX_STACK_(\w+) +(\d+)\b", txt, flags=re.M)}
    assert cols == {"COUNT": 0, "SUM": 1, "SUMSQ": 2, "COLS": 3}
    for name, value in cols.items():
        assert getattr(_lib, "STACK_" + name) == value == getattr(dr, "STACK_" + name), name
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(\w+) (\d+)u\b", txt, flags=re.M)}
    assert defs["PATH_STACK"] == 32768 == _lib.PATH_STACK == dr.PATH_STACK
    # no two paths share a bit
    values = [v for k, v in defs.items() if k.startswith("PATH_")]
    assert len(set(values)) == len(values) and all(v & (v - 1) == 0 for v in values)
    for decl in ("drx_status drx_wave_stack(", "drx_status drx_wave_stack_with_wave_words(",
                 "after drx_wave_stack: ms = { header-chain walk, everything behind the walk, 0, whole call }"):
        assert decl in txt, decl


def test_a_null_plan():
    from deltarice_amd import _lib
    lib = _lib.load()
    assert lib.drx_wave_stack(None, None, 0, None, None, 1, 0, 1, None, None, 3) == 1
    assert lib.drx_wave_stack_with_wave_words(None, None, 0, None, None, None, 1, 0, 1, None, None, 3) == 1


@pytest.mark.parametrize("sideband", [False, True])
def test_what_the_python_entry_passes_on(sideband):
    import torch
    from deltarice_amd import _lib
    plan = _plan()
    words, off = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    ww = torch.zeros(3, dtype=torch.int32)
    kw = dict(wave_words=ww) if sideband else {}
    name = "drx_wave_stack_with_wave_words" if sideband else "drx_wave_stack"
    side = (ww.data_ptr(),) if sideband else ()

    def last():
        return plan.ctx.lib.calls[-1]

    # the default width covers the plan's longest waveform (100 samples) from the offset
    out = plan.wave_stack_async(words, off, offset=-5, **kw)
    assert out.shape == (105, _lib.STACK_COLS) and out.dtype == torch.int64
    assert last() == (name, (1, words.data_ptr(), 8, off.data_ptr()) + side + (None, 0, -5, 105, None, out.data_ptr(), _lib.STACK_COLS))
    # a strided column, a selection of either type, the caller's rows, in_words
    start = torch.zeros((3, 8), dtype=torch.int64)[:, 3]
    rows = torch.zeros((7, 3), dtype=torch.int64)
    for select in (torch.ones(3, dtype=torch.bool), torch.ones(3, dtype=torch.uint8)):
        assert plan.wave_stack_async(words, off, 7, start, 2, select, rows, in_words=5, **kw) is rows
        assert last() == (name, (1, words.data_ptr(), 5, off.data_ptr()) + side + (start.data_ptr(), 8, 2, 7, select.data_ptr(), rows.data_ptr(), 3))
    # no position: an empty result, and the library is not called
    n = len(plan.ctx.lib.calls)
    assert plan.wave_stack_async(words, off, 0, **kw).shape == (0, _lib.STACK_COLS)
    assert plan.wave_stack_async(words, off, offset=100, **kw).shape == (0, _lib.STACK_COLS)
    assert plan.wave_stack_async(words, off, offset=1000, **kw).shape == (0, _lib.STACK_COLS)
    assert len(plan.ctx.lib.calls) == n


def test_python_entry_refusals_and_a_closed_plan():
    import torch
    from deltarice_amd import DeltaRiceError
    plan = _plan()
    words, off = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    refused = {
        "width -1": dict(width=-1),
        "width 2^32": dict(width=1 << 32),
        "offset": dict(offset=1 << 63),
        "start an int": dict(start=5),
        "start dtype": dict(start=torch.zeros(3, dtype=torch.int32)),
        "start 2-D": dict(start=torch.zeros((3, 1), dtype=torch.int64)),
        "start waves": dict(start=torch.zeros(4, dtype=torch.int64)),
        "start device": dict(start=torch.zeros(3, dtype=torch.int64, device="meta")),
        "start stride 0": dict(start=torch.zeros(1, dtype=torch.int64).expand(3)),
        "select a list": dict(select=[1, 0, 1]),
        "select dtype": dict(select=torch.zeros(3, dtype=torch.int32)),
        "select 2-D": dict(select=torch.zeros((3, 1), dtype=torch.uint8)),
        "select waves": dict(select=torch.zeros(2, dtype=torch.uint8)),
        "select strided": dict(select=torch.zeros(6, dtype=torch.uint8)[::2]),
        "select device": dict(select=torch.zeros(3, dtype=torch.bool, device="meta")),
        "out too small": dict(width=2, out=torch.zeros(2 * 3 - 1, dtype=torch.int64)),
        "out dtype": dict(width=2, out=torch.zeros(6, dtype=torch.int32)),
        "out device": dict(width=2, out=torch.zeros(6, dtype=torch.int64, device="meta")),
        "words dtype": dict(words=torch.zeros(8, dtype=torch.int64)),
        "wave_words length": dict(wave_words=torch.zeros(2, dtype=torch.int32)),
    }
    for what, kw in refused.items():
        w = kw.pop("words", words)
        with pytest.raises(DeltaRiceError) as e:
            plan.wave_stack_async(w, off, **kw)
        assert e.value.status == 1, what
    assert plan.ctx.lib.calls == []
    # a closed plan, in both entries
    plan._h = None
    for call in (lambda: plan.wave_stack(None), lambda: plan.wave_stack_async(None, None)):
        with pytest.raises(DeltaRiceError) as e:
            call()
        assert e.value.status == 1
