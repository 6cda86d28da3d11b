"""CPU: the surface of the encoded gather (drx_gather_encoded): exported symbols, the binding's constants, and the host-side
geometry of a gathered batch (gather_geometry: sample count and WaveformLength of every output chunk, and the lists it must
refuse) against a brute-force loop.  No compute calls (no GPU here)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_routes import BATCHES
from test_select_abi import boundary_indices, brute_force_lengths, large_geometries, length_of


def test_libraries_export_the_gather_entry_points():
    from deltarice_amd import _lib
    lib = _lib.load()
    for n in ("drx_gather_encoded", "drx_gather_encoded_with_wave_words"):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert _lib.PATH_GATHER == 256
    h5io = os.path.join(os.path.dirname(_lib.LIB_PATH), "libdeltarice_h5io.so")
    assert os.path.exists(h5io), "run `make`"
    assert hasattr(C.CDLL(h5io), "drx_h5_copy_rows")


def brute_force_gather(lens, sel, cw):
    """-> (N_c, L_c) of every output chunk, or the first entry that breaks the one-length rule."""
    N, L = [], []
    for c0 in range(0, len(sel), cw):
        ent = [int(lens[g]) for g in sel[c0:c0 + cw]]
        for j, n in enumerate(ent):
            if n > ent[0] or (n < ent[0] and j + 1 != len(ent)):
                return None, c0 + j
        N.append(sum(ent))
        L.append(ent[0])
    return (np.array(N, np.int64), np.array(L, np.int64)), None


CASES = {
    "uniform": ([7000 * 6] * 3, [7000] * 3),
    "short-last": ([7000 * 5 + 123] * 3, [7000] * 3),
    "whole-chunk": ([1000] * 4, [0] * 4),
    "ragged": BATCHES["ragged"][:2],
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("cw", [1, 2, 7, 10 ** 6])
def test_gather_geometry_against_a_loop(name, cw):
    pytest.importorskip("torch")
    from deltarice_amd import DeltaRiceError
    from deltarice_amd.codec import gather_geometry
    Ns, Ls = CASES[name]
    lens = brute_force_lengths(Ns, Ls)
    W = lens.size
    rng = np.random.default_rng(W + cw)
    lists = {"all": np.arange(W), "reversed": np.arange(W)[::-1], "random": rng.integers(0, W, 50),
             "by-length": np.argsort(-lens, kind="stable"), "one": np.array([W - 1]), "none": np.zeros(0, np.int64)}
    accepted = refused = 0
    for lname, sel in lists.items():
        want, bad = brute_force_gather(lens, sel.tolist(), cw)
        if want is None:
            with pytest.raises(DeltaRiceError) as e:
                gather_geometry(Ns, Ls, sel, cw)
            assert e.value.status == 1 and f"entry {bad} " in str(e.value), (lname, bad, str(e.value))
            refused += 1
        else:
            N, L = gather_geometry(Ns, Ls, sel, cw)
            assert np.array_equal(N, want[0]) and np.array_equal(L, want[1]), lname
            assert N.size == -(-sel.size // cw)
            accepted += 1
    assert accepted >= 2  # "one" and "none" at the least (cw = 1: every list)
    if name in ("short-last", "ragged") and 1 < cw < 10 ** 6:
        assert refused >= 1  # a short waveform in the middle of an output chunk


def test_gather_geometry_arguments():
    pytest.importorskip("torch")
    from deltarice_amd import DeltaRiceError
    from deltarice_amd.codec import gather_geometry
    Ns, Ls = CASES["uniform"]
    for cw in (0, -1):
        with pytest.raises(DeltaRiceError):
            gather_geometry(Ns, Ls, [0], cw)
    with pytest.raises(DeltaRiceError):
        gather_geometry(Ns, Ls, [18], 1)  # 18 waveforms: 0 ... 17
    with pytest.raises(DeltaRiceError):
        gather_geometry([2 ** 30] * 4, [0] * 4, [0, 1], 2)  # an output chunk of 2^31 samples
    N, L = gather_geometry([2 ** 30] * 4, [0] * 4, [0, 1], 1)
    assert N.tolist() == [2 ** 30] * 2 and L.tolist() == [2 ** 30] * 2


@pytest.mark.parametrize("name", ["fused-7000", "packed-64"])
@pytest.mark.parametrize("cw", [1, 3, 2000])
def test_gather_geometry_past_2_31_and_2_32_samples(name, cw):
    """gather_geometry of entries whose first sample needs bit 31 or bit 32, against the loop: indices as Python ints, int64
    and uint32."""
    pytest.importorskip("torch")
    from deltarice_amd import DeltaRiceError
    from deltarice_amd.codec import gather_geometry
    Ns, Ls = large_geometries()[name]
    idx, W = boundary_indices(Ns, Ls)
    lens = {g: length_of(Ns, Ls, g) for g in idx}
    want, bad = brute_force_gather(lens, idx, cw)
    assert bad is None
    assert int(want[0].sum()) == len(idx) * Ls[0]
    for given in (idx, np.array(idx, dtype=np.int64), np.array(idx, dtype=np.uint32)):
        N, L = gather_geometry(Ns, Ls, given, cw)
        assert N.dtype == np.int64 and L.dtype == np.int64
        assert np.array_equal(N, want[0]) and np.array_equal(L, want[1]), type(given)
    for out_of_range in ([0, W], np.array([W], dtype=np.uint32)):
        with pytest.raises(DeltaRiceError):
            gather_geometry(Ns, Ls, out_of_range, cw)
