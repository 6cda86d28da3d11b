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


def large_geometries():
    """{name: (chunk sample counts, WaveformLengths)} of the two geometries of test_gpu_large_batches.py whose waveform
    indices pass 2^31 // L and 2^32 // L"""
    from test_gpu_large_batches import UNIFORM, n_chunks_for
    out = {}
    for name in ("fused-7000", "packed-64"):
        W, L = UNIFORM[name][:2]
        n = n_chunks_for(W * L)
        out[name] = ([W * L] * n, [L] * n)
    return out


def length_of(Ns, Ls, g):
    """Samples of waveform g, chunk by chunk (brute_force_lengths() without the 10^7 waveforms in between)."""
    for N, L in zip(Ns, Ls):
        L = L if L > 0 else N
        W = -(-N // L)
        if g < W:
            return min(L, N - g * L)
        g -= W
    raise IndexError(g)


def boundary_indices(Ns, Ls):
    """Waveform indices on both sides of the waveforms that hold samples 2^31 and 2^32, and at the batch's end"""
    L = Ls[0]
    W = sum(-(-N // L) for N in Ns)
    assert W * L > 2 ** 32 + 2 * Ns[0]  # (two whole chunks behind the boundary: the rule of test_gpu_large_batches.py)
    idx = []
    for b in (2 ** 31 // L, 2 ** 32 // L):
        idx += [b - 2, b - 1, b, b + 1, b + 2]
    return idx + [W - 2, W - 1, 0], W


@pytest.mark.parametrize("name", ["fused-7000", "packed-64"])
def test_wave_lengths_past_2_31_and_2_32_samples(name):
    """Plan.wave_lengths where a waveform's first sample needs bit 31 or bit 32: indices as Python ints, int64 and uint32."""
    pytest.importorskip("torch")
    from deltarice_amd import DeltaRiceError
    from deltarice_amd.codec import Plan
    Ns, Ls = large_geometries()[name]
    idx, W = boundary_indices(Ns, Ls)
    want = np.array([length_of(Ns, Ls, g) for g in idx], dtype=np.int64)
    assert (want == Ls[0]).all()  # (whole waveforms only: what the loop says, spelled out)
    plan = object.__new__(Plan)  # the host arithmetic of a plan: no context, no handle
    plan._h, plan._chunk_samples, plan._wave_lens = None, np.asarray(Ns, dtype=np.int64), np.asarray(Ls, dtype=np.int64)
    for given in (idx, np.array(idx, dtype=np.int64), np.array(idx, dtype=np.uint32)):
        got = plan.wave_lengths(given)
        assert got.dtype == np.int64 and np.array_equal(got, want), type(given)
    for bad in ([W], np.array([W], dtype=np.uint32), np.array([2 ** 32 // Ls[0], W + 5], dtype=np.int64)):
        with pytest.raises(DeltaRiceError):
            plan.wave_lengths(bad)
