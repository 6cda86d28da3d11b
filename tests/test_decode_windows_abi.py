"""CPU: the surface of drx_decode_windows (exports, signatures, DRX_PATH_WINDOWS, the debug flags and the DRX_WINDOWS_FORM_*
values, a NULL plan, the Python entry's refusals) and the numpy model the GPU tests compare against
(tests/decode_windows_reference.py), held to rows worked by hand and to a plain per-sample loop."""
import os
import re

import numpy as np
import pytest

from decode_windows_reference import extents, windows_multi, windows_multi_loop
from plan_standin import plan as _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def test_exports_signatures_and_constants():
    from deltarice_amd import _lib
    import deltarice_amd as dr
    lib = _lib.load()
    for name in ("drx_decode_windows", "drx_decode_windows_with_wave_words", "drx_plan_last_windows_form"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    plain, sideband = _lib.SIGNATURES["drx_decode_windows"][1], _lib.SIGNATURES["drx_decode_windows_with_wave_words"][1]
    assert len(plain) == 15 and len(sideband) == 16  # the side-band form has one argument more
    assert sideband[:4] == plain[:4] and sideband[5:] == plain[4:]  # ... behind d_chunk_word_off, as in the other pairs
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(\w+) (\d+)u\b", txt, flags=re.M)}
    assert defs["PATH_WINDOWS"] == 8192 == _lib.PATH_WINDOWS == dr.PATH_WINDOWS
    assert defs["DBG_WINDOWS_LANES"] == 1073741824 == _lib.DBG_WINDOWS_LANES
    assert defs["DBG_WINDOWS_ALL_FALLBACK"] == 2147483648 == _lib.DBG_WINDOWS_ALL_FALLBACK
    assert (defs["WINDOWS_FORM_LANES"], defs["WINDOWS_FORM_BLOCKS"], defs["WINDOWS_FORM_FALLBACK_ALL"]) == (1, 2, 4)
    assert (_lib.WINDOWS_FORM_LANES, _lib.WINDOWS_FORM_BLOCKS, _lib.WINDOWS_FORM_FALLBACK_ALL) == (1, 2, 4)
    # no two paths and no two debug flags share a bit
    for prefix in ("PATH_", "DBG_"):
        values = [v for k, v in defs.items() if k.startswith(prefix)]
        assert len(set(values)) == len(values) and all(v & (v - 1) == 0 for v in values), prefix
    for decl in ("drx_status drx_decode_windows(", "drx_status drx_decode_windows_with_wave_words(",
                 "uint32_t drx_plan_last_windows_form(const drx_plan *plan);", "after drx_decode_windows: ms = { header-chain walk,"):
        assert decl in txt, decl


def test_a_null_plan_is_an_argument_error():
    from deltarice_amd import _lib
    lib = _lib.load()
    assert lib.drx_decode_windows(None, None, 0, None, None, 1, 1, None, 1, 0, 1, 0, None, 1, 1) == 1
    assert lib.drx_decode_windows_with_wave_words(None, None, 0, None, None, None, 1, 1, None, 1, 0, 1, 0, None, 1, 1) == 1
    assert lib.drx_plan_last_windows_form(None) == 0


def test_the_listed_query():
    from deltarice_amd import _lib, codec
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    assert re.search(r"^uint32_t drx_plan_last_windows_listed\(const drx_plan \*plan\);", txt, flags=re.M)
    assert "drx_plan_last_windows_listed" in _lib.SIGNATURES
    assert hasattr(lib, "drx_plan_last_windows_listed") and lib.drx_plan_last_windows_listed(None) == 0
    assert callable(codec.Plan.last_windows_listed)


def test_python_entry_refusals():
    import torch
    from deltarice_amd import DeltaRiceError
    plan = _plan()
    words, off = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    good = torch.zeros((3, 2), dtype=torch.int64)
    refused = {
        "start None": dict(start=None),
        "start an int": dict(start=5),
        "start dtype": dict(start=torch.zeros((3, 2), dtype=torch.int32)),
        "start 1-D": dict(start=torch.zeros(3, dtype=torch.int64)),
        "start 3-D": dict(start=torch.zeros((3, 2, 1), dtype=torch.int64)),
        "start waves": dict(start=torch.zeros((4, 2), dtype=torch.int64)),
        "start device": dict(start=torch.zeros((3, 2), dtype=torch.int64, device="meta")),
        "start wave stride 0": dict(start=torch.zeros((1, 2), dtype=torch.int64).expand(3, 2)),
        "start window stride 0": dict(start=torch.zeros((3, 1), dtype=torch.int64).expand(3, 2)),
        "width -1": dict(start=good, width=-1),
        "width 2^32": dict(start=good, width=1 << 32),
        "pad": dict(start=good, pad=32768),
        "offset": dict(start=good, offset=1 << 63),
        "count too small": dict(start=good, count=torch.zeros(2, dtype=torch.int32)),
        "count dtype": dict(start=good, count=torch.zeros(3, dtype=torch.int64)),
        "count device": dict(start=good, count=torch.zeros(3, dtype=torch.int32, device="meta")),
        "rows overlap": dict(start=good, out_strides=(32, 15)),
        "waveforms overlap": dict(start=good, out_strides=(31, 16)),
        "out too small": dict(start=good, out=torch.zeros(3 * 2 * 16 - 1, dtype=torch.int16)),
        "out too small for its strides": dict(start=good, out=torch.zeros(2 * 40 + 20 + 16 - 1, dtype=torch.int16), out_strides=(40, 20)),
        "out dtype": dict(start=good, out=torch.zeros(96, dtype=torch.int32)),
        "out device": dict(start=good, out=torch.zeros(96, dtype=torch.int16, device="meta")),
        "words dtype": dict(start=good, words=torch.zeros(8, dtype=torch.int64)),
        "words device": dict(start=good, words=torch.zeros(8, dtype=torch.int32, device="meta")),
        "wave_words dtype": dict(start=good, wave_words=torch.zeros(3, dtype=torch.int64)),
        "wave_words length": dict(start=good, wave_words=torch.zeros(2, dtype=torch.int32)),
    }
    for what, kw in refused.items():
        w, start, width = kw.pop("words", words), kw.pop("start"), kw.pop("width", 16)
        with pytest.raises(DeltaRiceError) as e:
            plan.decode_windows_async(w, off, start, width, **kw)
        assert e.value.status == 1, what
    # no width and no window slot: empty results, and the library is not called (tests/test_codec_calls.py holds the stand-in's record to that)
    assert plan.decode_windows_async(words, off, good, 0).shape == (3, 2, 0)
    assert plan.decode_windows_async(words, off, torch.zeros((3, 0), dtype=torch.int64), 16).shape == (3, 0, 16)
    # a closed plan, in both entries
    plan._h = None
    for call in (lambda: plan.decode_windows(None, good, 16), lambda: plan.decode_windows_async(None, None, good, 16)):
        with pytest.raises(DeltaRiceError) as e:
            call()
        assert e.value.status == 1


def test_model_by_hand():
    # two chunks: 10 samples in waveforms of 4 (the last one of 2), then 7 samples in one waveform
    #            w0             w1            w2      w3
    y = np.array([5, 9, 1, 1,   1, 6, 6, 1,   7, 8,   0, 9, 9, 3, 0, 9, 0], np.int16)
    Ns, Ls = [10, 7], [4, 0]
    P = -7
    starts = np.array([[-2, 1, 9],    # in front of and across the start; across the end; behind the waveform
                       [0, 0, 2],     # coinciding windows
                       [1, -3, 0],    # the short last waveform of a chunk; a window wholly in front of it
                       [5, 2, 4]])    # an unsorted list
    r = windows_multi(y, Ns, Ls, starts, None, 0, 3, P)
    assert r.dtype == np.int16 and r.shape == (4, 3, 3)
    assert r[0].tolist() == [[P, P, 5], [9, 1, 1], [P, P, P]]
    assert r[1].tolist() == [[1, 6, 6], [1, 6, 6], [6, 1, P]]
    assert r[2].tolist() == [[8, P, P], [P, P, P], [7, 8, P]]
    assert r[3].tolist() == [[9, 0, P], [9, 3, 0], [0, 9, 0]]
    assert extents(Ns, Ls, starts, None, 0, 3).tolist() == [4, 4, 2, 7]
    # counts: a dead slot is all pad, a count above K leaves every slot live, a count of 0 none
    r = windows_multi(y, Ns, Ls, starts, [2, 7, 0, 1], 0, 3, P)
    assert r[0].tolist() == [[P, P, 5], [9, 1, 1], [P, P, P]] and r[1].tolist() == [[1, 6, 6], [1, 6, 6], [6, 1, P]]
    assert r[2].tolist() == [[P] * 3] * 3 and r[3].tolist() == [[9, 0, P], [P] * 3, [P] * 3]
    assert extents(Ns, Ls, starts, [2, 7, 0, 1], 0, 3).tolist() == [4, 4, 0, 7]
    # the offset moves every window
    assert windows_multi(y, Ns, Ls, starts, None, 1, 3, P)[3].tolist() == [[0, P, P], [3, 0, 9], [9, 0, P]]
    # start + offset saturates at both int64 ends (it does not wrap round into the waveform)
    far = np.array([[I64_MAX, I64_MIN]] * 4, np.int64)
    at_minus_1 = [[P, 5, 9], [P, 1, 6], [P, 7, 8], [P, 0, 9]]
    r = windows_multi(y, Ns, Ls, far, None, I64_MAX, 3, P)  # max + max stays max; min + max = -1
    assert (r[:, 0] == P).all() and r[:, 1].tolist() == at_minus_1
    r = windows_multi(y, Ns, Ls, far, None, I64_MIN, 3, P)  # max + min = -1; min + min stays min
    assert r[:, 0].tolist() == at_minus_1 and (r[:, 1] == P).all()
    r = windows_multi(y, Ns, Ls, far, None, 0, 3, P)
    assert (r == P).all() and extents(Ns, Ls, far, None, 0, 3).tolist() == [0, 0, 0, 0]
    r = windows_multi(y, Ns, Ls, np.array([[I64_MAX, I64_MIN + 1]] * 4), None, I64_MIN + 1, 3, P)  # max + (min + 1) = 0
    assert r[:, 0].tolist() == [[5, 9, 1], [1, 6, 6], [7, 8, P], [0, 9, 9]] and (r[:, 1] == P).all()


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_model_against_a_plain_loop(seed):
    rng = np.random.default_rng(seed)
    for Ns, Ls in (([20, 37], [4, 5]), ([64], [0]), ([3], [1]), ([50 * 2, 10 * 3 + 7, 55], [50, 10, 0])):
        y = rng.integers(-300, 300, sum(Ns)).astype(np.int16)
        W = sum(-(-N // (L or N)) for N, L in zip(Ns, Ls))
        for K, width, offset, pad in ((1, 5, 0, 0), (3, 7, -2, -1), (4, 1, 3, 9), (2, 70, -10, 32767), (5, 3, 0, -32768)):
            starts = rng.integers(-8, 60, (W, K))
            for counts in (None, rng.integers(0, K + 2, W)):
                got = windows_multi(y, Ns, Ls, starts, counts, offset, width, pad)
                want = windows_multi_loop(y, Ns, Ls, starts, counts, offset, width, pad)
                assert got.dtype == np.int16 and got.shape == (W, K, width)
                assert np.array_equal(got, want), (Ns, Ls, K, width, offset, pad)
