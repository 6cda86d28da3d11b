"""CPU: the surface of drx_wave_stats (exports, constants, the Python entry's refusal of a closed plan) and the numpy reference
the GPU tests compare against (tests/wave_stats_reference.py), held to a plain Python loop on tiny inputs."""
import os
import re

import numpy as np
import pytest

from wave_stats_reference import wave_geometry, wave_stats, wave_stats_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ([512 * 40, 2048 * 9 + 17, 7000 * 30, 16384 * 4, 4321, 3333 * 21 + 1], [512, 2048, 7000, 16384, 0, 3333])  # test_gpu_routes' "ragged"


def test_exports_and_constants():
    from deltarice_amd import _lib
    import deltarice_amd as dr
    lib = _lib.load()
    for name in ("drx_wave_stats", "drx_wave_stats_with_wave_words"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["drx_wave_stats_with_wave_words"][1]) == len(_lib.SIGNATURES["drx_wave_stats"][1]) + 1
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(STAT_\w+) (\d+)\b", txt, flags=re.M)}
    assert len(defs) == len(re.findall(r"^#define DRX_STAT_", txt, flags=re.M)) == 9
    assert [defs[n] for n in ("STAT_MIN", "STAT_ARGMIN", "STAT_MAX", "STAT_ARGMAX", "STAT_SUM", "STAT_SUMSQ", "STAT_HEAD_SUM",
                              "STAT_HEAD_SUMSQ", "STAT_COLS")] == list(range(9))
    for name, value in defs.items():
        assert getattr(_lib, name) == value and getattr(dr, name) == value, name
    assert {n for n in dir(_lib) if n.startswith("STAT_")} == set(defs)
    assert re.search(r"^#define DRX_PATH_STATS 512u\b", txt, flags=re.M) and _lib.PATH_STATS == dr.PATH_STATS == 512


def test_wave_stats_on_a_closed_plan_raises():
    from deltarice_amd import DeltaRiceError, codec
    plan = object.__new__(codec.Plan)  # (no GPU here: a plan as close() leaves it)
    plan.ctx, plan._h = None, None
    for call in (lambda: plan.wave_stats(None), lambda: plan.wave_stats_async(None, None)):
        with pytest.raises(DeltaRiceError):
            call()


def test_geometry_of_the_reference():
    start, length = wave_geometry([10, 7, 5], [4, 0, 5])
    assert start.tolist() == [0, 4, 8, 10, 17] and length.tolist() == [4, 4, 2, 7, 5]
    start, length = wave_geometry(*RAGGED)
    assert start.size == 40 + 10 + 30 + 4 + 1 + 22 and int(start[-1] + length[-1]) == sum(RAGGED[0])
    assert length[49] == 17 and length[84] == 4321 and length[-1] == 1


@pytest.mark.parametrize("head", [0, 1, 3, 4, 5, (1 << 32) - 1])
def test_reference_against_a_plain_loop(head):
    rng = np.random.default_rng(head & 0xFFFF)
    cases = [
        (rng.integers(-3, 4, 57).astype(np.int16), [20, 37], [4, 5]),             # many ties; short last waveforms
        (rng.integers(-32768, 32768, 64).astype(np.int16), [64], [0]),            # the whole range, one waveform
        (np.array([-32768] * 6 + [32767] * 6, np.int16), [12], [3]),              # constant rows: every index ties
        (np.array([5], np.int16), [1], [0]),                                       # one waveform of one sample
        (np.array([7, -7, 7], np.int16), [3], [1]),                                # one-sample waveforms
        (np.array([1, 2, 2, 1, 1, 2, 2, 1, 0, 3, 3, 0], np.int16), [12], [4]),     # plateaus: the first one wins
    ]
    for x, Ns, Ls in cases:
        got, want = wave_stats(x, Ns, Ls, head), wave_stats_loop(x, Ns, Ls, head)
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (Ns, Ls, head)


def test_reference_on_the_ragged_geometry():
    Ns, Ls = RAGGED
    rng = np.random.default_rng(5)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    for head in (0, 100):
        assert np.array_equal(wave_stats(x, Ns, Ls, head), wave_stats_loop(x, Ns, Ls, head)), head


def test_reference_sums_do_not_wrap():
    x = np.full(70000, -32768, np.int16)
    r = wave_stats(x, [70000], [0], 100)
    assert r[0].tolist() == [-32768, 0, -32768, 0, -32768 * 70000, 70000 << 30, -32768 * 100, 100 << 30]
    assert r[0, 4] < -(1 << 31) and r[0, 5] > 1 << 46
