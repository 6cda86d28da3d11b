"""CPU: the surface of drx_decode_window (exports, signatures, DRX_PATH_WINDOW, a NULL plan, the Python entry's refusals) and the
numpy model the GPU tests compare against (tests/decode_window_reference.py), held to a plain loop and to rows checked by hand."""
import os
import re

import numpy as np
import pytest

from decode_window_reference import windows, windows_loop
from plan_standin import plan as _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_signatures_and_path_constant():
    from deltarice_amd import _lib
    import deltarice_amd as dr
    lib = _lib.load()
    for name in ("drx_decode_window", "drx_decode_window_with_wave_words"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    plain, sideband = _lib.SIGNATURES["drx_decode_window"][1], _lib.SIGNATURES["drx_decode_window_with_wave_words"][1]
    assert len(plain) == 11 and len(sideband) == len(plain) + 1  # the side-band form has one argument more
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    assert re.search(r"^#define DRX_PATH_WINDOW 2048u\b", txt, flags=re.M)
    assert _lib.PATH_WINDOW == dr.PATH_WINDOW == 2048
    paths = {k: int(v) for k, v in re.findall(r"^#define DRX_(PATH_\w+) (\d+)u\b", txt, flags=re.M)}
    assert len(paths) == len(re.findall(r"^#define DRX_PATH_", txt, flags=re.M)) and len(set(paths.values())) == len(paths)
    for name, value in paths.items():
        assert getattr(_lib, name) == value, name
    for decl in ("drx_status drx_decode_window(", "drx_status drx_decode_window_with_wave_words("):
        assert decl in txt, decl


def test_a_null_plan_is_an_argument_error():
    from deltarice_amd import _lib
    lib = _lib.load()
    assert lib.drx_decode_window(None, None, 0, None, None, 0, 0, 16, 0, None, 16) == 1
    assert lib.drx_decode_window_with_wave_words(None, None, 0, None, None, None, 0, 0, 16, 0, None, 16) == 1


def test_python_entry_refusals():
    import torch
    from deltarice_amd import DeltaRiceError
    plan = _plan()
    words, off = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    good = torch.zeros(3, dtype=torch.int64)
    refused = {
        "start dtype": dict(start=torch.zeros(3, dtype=torch.int32), width=4),
        "start length": dict(start=torch.zeros(4, dtype=torch.int64), width=4),
        "start 2-D": dict(start=torch.zeros((3, 1), dtype=torch.int64), width=4),
        "start device": dict(start=torch.zeros(3, dtype=torch.int64, device="meta"), width=4),
        "out too small": dict(start=good, width=4, out=torch.zeros(11, dtype=torch.int16)),
        "out too small for the stride": dict(start=good, width=4, out_stride=6, out=torch.zeros(15, dtype=torch.int16)),
        "out dtype": dict(start=good, width=4, out=torch.zeros(12, dtype=torch.int32)),
        "out device": dict(start=good, width=4, out=torch.zeros(12, dtype=torch.int16, device="meta")),
        "stride below width": dict(start=good, width=4, out_stride=3),
        "width": dict(start=good, width=-1),
        "pad": dict(start=good, width=4, pad=40000),
        "words dtype": dict(start=good, width=4, words=torch.zeros(8, dtype=torch.int64)),
    }
    for what, kw in refused.items():
        w = kw.pop("words", words)
        with pytest.raises(DeltaRiceError) as e:
            plan.decode_window_async(w, off, **kw)
        assert e.value.status == 1, what
    # a closed plan, in both entries
    plan._h = None
    for call in (lambda: plan.decode_window(None, None, 4), lambda: plan.decode_window_async(None, None, None, 4)):
        with pytest.raises(DeltaRiceError):
            call()


def test_model_by_hand():
    # two chunks: 10 samples in waveforms of 4 (the last one of 2), then 7 samples in one waveform
    y = np.arange(100, 117).astype(np.int16)
    Ns, Ls = [10, 7], [4, 0]
    r = windows(y, Ns, Ls, None, -2, 5, -1)  # a negative start: two pads, then the first three samples
    assert r.tolist() == [[-1, -1, 100, 101, 102], [-1, -1, 104, 105, 106], [-1, -1, 108, 109, -1], [-1, -1, 110, 111, 112]]
    r = windows(y, Ns, Ls, [2, 3, 1, 5], 0, 4, 9)  # windows across the end; the short last waveform of chunk 0
    assert r.tolist() == [[102, 103, 9, 9], [107, 9, 9, 9], [109, 9, 9, 9], [115, 116, 9, 9]]
    r = windows(y, Ns, Ls, [4, -4, 2, 7], 0, 4, 9)  # wholly outside, on either side
    assert (r == 9).all()
    r = windows(y, Ns, Ls, [0, 0, 0, 0], 0, 7, 0)  # the whole waveform and more
    assert r[2].tolist() == [108, 109, 0, 0, 0, 0, 0] and r[3].tolist() == list(range(110, 117))
    for big in ((1 << 63) - 1, -(1 << 63)):  # the sum saturates (it does not wrap round into the waveform)
        assert (windows(y, Ns, Ls, [big, big, big, big // 2 - 1], big, 2, 5) == 5).all()
    assert windows(y, Ns, Ls, [(1 << 63) - 1, 0, 0, 0], -(1 << 63), 2, 5)[0].tolist() == [5, 100]  # (start -1)
    assert windows(y, Ns, Ls, 1, 1, 2, 0).tolist() == [[102, 103], [106, 107], [0, 0], [112, 113]]


@pytest.mark.parametrize("width", [1, 2, 5, 9])
def test_model_against_a_plain_loop(width):
    rng = np.random.default_rng(width)
    for Ns, Ls in (([20, 37], [4, 5]), ([64], [0]), ([3], [1]), ([512 * 2, 100 * 3 + 17, 55], [512, 100, 0])):
        y = rng.integers(-32768, 32768, sum(Ns)).astype(np.int16)
        W = sum(-(-N // (L or N)) for N, L in zip(Ns, Ls))
        starts = rng.integers(-12, 530, W)
        for st, offset in ((None, 0), (None, -3), (7, 0), (starts, 0), (starts, -4)):
            got, want = windows(y, Ns, Ls, st, offset, width, -7), windows_loop(y, Ns, Ls, st, offset, width, -7)
            assert got.dtype == np.int16 and got.shape == (W, width) and np.array_equal(got, want), (Ns, Ls, width, offset)
