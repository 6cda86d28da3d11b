"""CPU: the surface of the selected-waveform decode (drx_decode_select): exported symbols, the binding's constant, and the
arithmetic of Plan.wave_lengths against a brute-force loop.  No compute calls (no GPU here)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_routes import BATCHES


def test_libraries_export_the_select_entry_points():
    from deltarice_amd import _lib
    lib = _lib.load()
    for n in ("drx_decode_select", "drx_decode_select_with_wave_words"):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert _lib.PATH_SELECT == 128
    h5io = os.path.join(os.path.dirname(_lib.LIB_PATH), "libdeltarice_h5io.so")
    assert os.path.exists(h5io), "run `make`"
    assert hasattr(C.CDLL(h5io), "drx_h5_read_rows")


def brute_force_lengths(Ns, Ls):
    out = []
    for N, L in zip(Ns, Ls):
        L = L if L > 0 else N
        left = N
        while left > 0:
            out.append(min(L, left))
            left -= L
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("Ns,Ls", [([7000 * 5 + 123] * 3, [7000] * 3), ([1000] * 2, [0] * 2), ([10], [3]), BATCHES["ragged"][:2]],
                         ids=["uniform-short-last", "whole-chunk", "tiny", "ragged"])
def test_wave_lengths_against_a_loop(Ns, Ls):
    torch = pytest.importorskip("torch")
    from deltarice_amd import DeltaRiceError
    from deltarice_amd.codec import wave_lengths
    want = brute_force_lengths(Ns, Ls)
    every = np.arange(want.size)
    assert np.array_equal(wave_lengths(Ns, Ls, every), want)
    pick = np.random.default_rng(7).integers(0, want.size, 50)  # any order, duplicates
    assert np.array_equal(wave_lengths(Ns, Ls, pick), want[pick])
    assert np.array_equal(wave_lengths(Ns, Ls, pick.tolist()), want[pick])
    assert np.array_equal(wave_lengths(Ns, Ls, torch.from_numpy(pick)), want[pick])
    assert np.array_equal(wave_lengths(Ns, Ls, every[::-1].astype(np.uint32)), want[::-1])
    assert wave_lengths(Ns, Ls, []).size == 0
    for bad in ([want.size], [-1], [0.5]):
        with pytest.raises(DeltaRiceError):
            wave_lengths(Ns, Ls, bad)
