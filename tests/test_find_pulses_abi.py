"""CPU: the surface of drx_find_pulses (exports, signatures, DRX_PATH_PULSES, the DRX_PULSE_* columns, a NULL plan, the Python
entry's refusals) and the numpy model the GPU tests compare against (tests/find_pulses_reference.py), held to rows worked by
hand and to a plain per-sample loop."""
import os
import re

import numpy as np
import pytest

from find_pulses_reference import find_pulses, find_pulses_loop
from plan_standin import plan as _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def test_exports_signatures_and_constants():
    from deltarice_amd import _lib
    import deltarice_amd as dr
    lib = _lib.load()
    for name in ("drx_find_pulses", "drx_find_pulses_with_wave_words"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    plain, sideband = _lib.SIGNATURES["drx_find_pulses"][1], _lib.SIGNATURES["drx_find_pulses_with_wave_words"][1]
    assert len(plain) == 12 and len(sideband) == len(plain) + 1  # the side-band form has one argument more
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    assert re.search(r"^#define DRX_PATH_PULSES 4096u\b", txt, flags=re.M)
    assert _lib.PATH_PULSES == dr.PATH_PULSES == 4096
    paths = {k: int(v) for k, v in re.findall(r"^#define DRX_(PATH_\w+) (\d+)u\b", txt, flags=re.M)}
    assert len(paths) == len(re.findall(r"^#define DRX_PATH_", txt, flags=re.M)) and len(set(paths.values())) == len(paths)
    for name, value in paths.items():
        assert getattr(_lib, name) == value, name
    cols = {k: int(v) for k, v in re.findall(r"^#define DRX_(PULSE_\w+) (\d+)\b", txt, flags=re.M)}
    assert cols == dict(PULSE_START=0, PULSE_WIDTH=1, PULSE_PEAK=2, PULSE_ARGPEAK=3, PULSE_SUM=4, PULSE_COLS=5)
    for name, value in cols.items():
        assert getattr(_lib, name) == getattr(dr, name) == value, name
    for decl in ("drx_status drx_find_pulses(", "drx_status drx_find_pulses_with_wave_words(",
                 "after drx_find_pulses: ms = { header-chain walk, pulse kernel, 0, whole call }"):
        assert decl in txt, decl


def test_a_null_plan_is_an_argument_error():
    from deltarice_amd import _lib
    lib = _lib.load()
    assert lib.drx_find_pulses(None, None, 0, None, None, 0, 0, 1, 1, 4, None, None) == 1
    assert lib.drx_find_pulses_with_wave_words(None, None, 0, None, None, None, 0, 0, 1, 1, 4, None, None) == 1


def test_python_entry_refusals():
    import torch
    from deltarice_amd import DeltaRiceError
    plan = _plan()
    words, off = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    good = torch.zeros(3, dtype=torch.int64)
    refused = {
        "threshold dtype": dict(threshold=torch.zeros(3, dtype=torch.int32)),
        "threshold length": dict(threshold=torch.zeros(4, dtype=torch.int64)),
        "threshold 2-D": dict(threshold=torch.zeros((3, 1), dtype=torch.int64)),
        "threshold device": dict(threshold=torch.zeros(3, dtype=torch.int64, device="meta")),
        "threshold stride 0": dict(threshold=torch.zeros(1, dtype=torch.int64).expand(3)),
        "offset": dict(threshold=I64_MAX, offset=1),
        "polarity": dict(threshold=good, polarity=0),
        "min_width 0": dict(threshold=good, min_width=0),
        "min_width 2^32": dict(threshold=good, min_width=1 << 32),
        "max_pulses -1": dict(threshold=good, max_pulses=-1),
        "max_pulses 2^32": dict(threshold=good, max_pulses=1 << 32),
        "out too small": dict(threshold=good, max_pulses=4, out=torch.zeros(3 * 4 * 5 - 1, dtype=torch.int64)),
        "out dtype": dict(threshold=good, max_pulses=4, out=torch.zeros(60, dtype=torch.int32)),
        "out device": dict(threshold=good, max_pulses=4, out=torch.zeros(60, dtype=torch.int64, device="meta")),
        "count too small": dict(threshold=good, count=torch.zeros(2, dtype=torch.int32)),
        "count dtype": dict(threshold=good, count=torch.zeros(3, dtype=torch.int64)),
        "count device": dict(threshold=good, count=torch.zeros(3, dtype=torch.int32, device="meta")),
        "words dtype": dict(threshold=good, words=torch.zeros(8, dtype=torch.int64)),
        "words device": dict(threshold=good, words=torch.zeros(8, dtype=torch.int32, device="meta")),
        "wave_words dtype": dict(threshold=good, wave_words=torch.zeros(3, dtype=torch.int64)),
        "wave_words length": dict(threshold=good, wave_words=torch.zeros(2, dtype=torch.int32)),
    }
    for what, kw in refused.items():
        w = kw.pop("words", words)
        with pytest.raises(DeltaRiceError) as e:
            plan.find_pulses_async(w, off, **kw)
        assert e.value.status == 1, what
    # a closed plan, in both entries
    plan._h = None
    for call in (lambda: plan.find_pulses(None, 0), lambda: plan.find_pulses_async(None, None, 0)):
        with pytest.raises(DeltaRiceError) as e:
            call()
        assert e.value.status == 1


def test_model_by_hand():
    # two chunks: 10 samples in waveforms of 4 (the last one of 2), then 7 samples in one waveform
    #            w0             w1            w2      w3
    y = np.array([5, 9, 1, 1,   1, 6, 6, 1,   7, 8,   0, 9, 9, 3, 0, 9, 0], np.int16)
    Ns, Ls = [10, 7], [4, 0]
    n, p = find_pulses(y, Ns, Ls, 4, 1, 1, 2)
    assert n.dtype == np.int32 and p.dtype == np.int64 and p.shape == (4, 2, 5)
    assert n.tolist() == [1, 1, 1, 2]
    assert p[0].tolist() == [[0, 2, 9, 1, 14], [0] * 5]  # a run from sample 0
    assert p[1].tolist() == [[1, 2, 6, 1, 12], [0] * 5]  # a plateau: ARGPEAK is its first sample
    assert p[2].tolist() == [[0, 2, 8, 1, 15], [0] * 5]  # the short last waveform of a chunk, over from end to end
    assert p[3].tolist() == [[1, 2, 9, 1, 18], [5, 1, 9, 5, 9]]
    # strictness at y == t: 9 is not over 9, 1 is not under 1
    assert find_pulses(y, Ns, Ls, 9, 1, 1, 2)[0].tolist() == [0, 0, 0, 0]
    assert find_pulses(y, Ns, Ls, 1, -1, 1, 2)[0].tolist() == [0, 0, 0, 3]
    # negative polarity: PEAK is the minimum; a run to the last sample
    n, p = find_pulses(y, Ns, Ls, 4, -1, 1, 3)
    assert n.tolist() == [1, 2, 0, 3]
    assert p[0, 0].tolist() == [2, 2, 1, 2, 2] and p[1, :2].tolist() == [[0, 1, 1, 0, 1], [3, 1, 1, 3, 1]]
    assert p[3].tolist() == [[0, 1, 0, 0, 0], [3, 2, 0, 4, 3], [6, 1, 0, 6, 0]]
    # min_width drops a run without disturbing the numbering of the others; max_pulses cuts the row, not the count
    n, p = find_pulses(y, Ns, Ls, 4, 1, 2, 2)
    assert n.tolist() == [1, 1, 1, 1] and p[3].tolist() == [[1, 2, 9, 1, 18], [0] * 5]
    n, p = find_pulses(y, Ns, Ls, 4, -1, 2, 1)
    assert n.tolist() == [1, 0, 0, 1] and p[3, 0].tolist() == [3, 2, 0, 4, 3]
    n, p = find_pulses(y, Ns, Ls, 4, -1, 1, 1)
    assert n.tolist() == [1, 2, 0, 3] and p[3].tolist() == [[0, 1, 0, 0, 0]]
    n, p = find_pulses(y, Ns, Ls, 4, 1, 1, 0)  # the counting form
    assert n.tolist() == [1, 1, 1, 2] and p.shape == (4, 0, 5)
    # d_thr + thr saturates at both int64 ends (it does not wrap round to the other side of the samples)
    tab = np.array([I64_MAX, I64_MAX, I64_MIN, I64_MIN], np.int64)
    assert find_pulses(y, Ns, Ls, I64_MAX, 1, 1, 1, tab)[0].tolist() == [0, 0, 1, 1]  # max + max stays max; min + max = -1
    assert find_pulses(y, Ns, Ls, I64_MAX, -1, 1, 1, tab)[0].tolist() == [1, 1, 0, 0]  # ... and everything lies below it
    n, p = find_pulses(y, Ns, Ls, I64_MIN, 1, 1, 1, tab)  # max + min = -1: everything is over; min + min stays min: as well
    assert n.tolist() == [1, 1, 1, 1] and p[:, 0, 1].tolist() == [4, 4, 2, 7]
    # a per-waveform threshold
    assert find_pulses(y, Ns, Ls, 1, 1, 1, 1, np.array([7, 5, 6, 7]))[0].tolist() == [1, 0, 1, 2]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_model_against_a_plain_loop(seed):
    rng = np.random.default_rng(seed)
    for Ns, Ls in (([20, 37], [4, 5]), ([64], [0]), ([3], [1]), ([50 * 2, 10 * 3 + 7, 55], [50, 10, 0])):
        y = rng.integers(-4, 5, sum(Ns)).astype(np.int16)
        y[rng.integers(0, y.size, 3)] = [-32768, 32767, 0]
        W = sum(-(-N // (L or N)) for N, L in zip(Ns, Ls))
        tab = rng.integers(-3, 4, W)
        for thr, pol, mw, mp, tt in ((0, 1, 1, 3, None), (1, -1, 1, 2, None), (-1, 1, 2, 4, tab), (0, -1, 3, 1, tab), (-5, 1, 1, 2, None),
                                     (2, 1, 1, 0, tab), (32767, 1, 1, 1, None), (-32768, -1, 1, 1, None), (32767, -1, 1, 1, None)):
            got, want = find_pulses(y, Ns, Ls, thr, pol, mw, mp, tt), find_pulses_loop(y, Ns, Ls, thr, pol, mw, mp, tt)
            assert got[0].dtype == np.int32 and got[1].shape == (W, mp, 5)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (Ns, Ls, thr, pol, mw, mp)
