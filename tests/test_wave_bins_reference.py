"""CPU: the numpy model the GPU tests of drx_wave_bins compare against (tests/wave_bins_reference.py), held to rows worked by
hand, to a plain per-sample loop on tiny inputs, and to wave_stats_reference: the bins that cover a waveform merge to its SUM,
SUMSQ, MIN, MAX."""
import numpy as np
import pytest

from wave_bins_reference import EMPTY, default_n_bins, merge, wave_bins, wave_bins_loop
from wave_stats_reference import wave_geometry, wave_stats

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U32 = (1 << 32) - 1
RAGGED = ([512 * 40, 2048 * 9 + 17, 7000 * 30, 16384 * 4, 4321, 3333 * 21 + 1], [512, 2048, 7000, 16384, 0, 3333])  # test_gpu_routes' "ragged"


def same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    assert np.array_equal(got, want), what


def test_model_by_hand():
    # two chunks: 10 samples in waveforms of 4 (the last one of 2), then 7 samples in one waveform
    #             w0            w1            w2      w3
    y = np.array([5, 9, 1, 1,   1, 6, 6, 1,   7, 8,   0, 9, -9, 3, 0, 9, 0], np.int16)
    Ns, Ls = [10, 7], [4, 0]
    E = list(EMPTY)
    r = wave_bins(y, Ns, Ls, 3, 3)
    assert r.shape == (4, 3, 4)
    assert r[0].tolist() == [[15, 107, 1, 9], [1, 1, 1, 1], E]
    assert r[2].tolist() == [[15, 113, 7, 8], E, E]  # the short last waveform of a chunk
    assert r[3].tolist() == [[0, 162, -9, 9], [12, 90, 0, 9], [0, 0, 0, 0]]
    # per-waveform origins and an offset: bins in front of, across and behind the waveform
    r = wave_bins(y, Ns, Ls, 2, 3, start=np.array([-1, 3, 9, 5]), offset=-1)
    assert r[0].tolist() == [E, [14, 106, 5, 9], [2, 2, 1, 1]]  # a = -2
    assert r[1].tolist() == [[7, 37, 1, 6], E, E]               # a = 2
    assert r[2].tolist() == [E, E, E]                           # a = 8
    assert r[3].tolist() == [[9, 81, 0, 9], [0, 0, 0, 0], E]    # a = 4
    # start + offset saturates at both int64 ends (it does not wrap round into the waveform)
    far = np.array([I64_MAX, I64_MIN, I64_MAX, I64_MIN])
    assert (wave_bins(y, Ns, Ls, 2, 3, far, I64_MAX)[[0, 2]] == np.array(EMPTY)).all()  # max + max stays max
    assert wave_bins(y, Ns, Ls, 2, 3, far, I64_MAX)[1].tolist() == [[1, 1, 1, 1], [12, 72, 6, 6], [1, 1, 1, 1]]  # min + max = -1
    assert wave_bins(y, Ns, Ls, 2, 3, far, I64_MIN)[0].tolist() == [[5, 25, 5, 5], [10, 82, 1, 9], [1, 1, 1, 1]]  # max + min = -1
    assert (wave_bins(y, Ns, Ls, 2, 3, far, I64_MIN)[[1, 3]] == np.array(EMPTY)).all()  # min + min stays min
    assert (wave_bins(y, Ns, Ls, U32, 3, far, 0) == np.array(EMPTY)).all()
    # a bin of 2^32 - 1 from a_g = -(2^32 - 1) * 2 + 1: bin 1 ends at sample 1, bin 2 holds the rest
    r = wave_bins(y, Ns, Ls, U32, 3, None, -2 * U32 + 1)
    assert r[0].tolist() == [E, [5, 25, 5, 5], [11, 83, 1, 9]]


def test_seventy_thousand_minimal_samples_in_one_bin_do_not_wrap():
    y = np.full(70000, -32768, np.int16)
    r = wave_bins(y, [70000], [0], 1 << 31, 1)
    assert r.tolist() == [[[-32768 * 70000, (1 << 30) * 70000, -32768, -32768]]]
    assert r[0, 0, 0] < -(1 << 31) and r[0, 0, 1] > 1 << 46


def cases_of(n):
    """(bin, n_bins, origin column or None, offset) over a geometry whose longest waveform has n samples"""
    big = (1, 2, n // 3 + 1, n + 7)
    for bin in sorted({1, 3, max(n - 1, 1), n, n + 1, U32}):
        full = -(-n // bin)
        for n_bins in sorted({1, max(full // 2, 1), full, full + 5} if bin != 1 else {1, n // 2 + 1, n + 40}):
            yield bin, n_bins, None, 0
    for a in (-5, 0, n - 1, n):
        for bin in (1, 3, n):
            yield bin, big[2], ("const", a), 0
    for a, off in ((I64_MAX, I64_MAX), (I64_MAX, 1), (I64_MAX, -I64_MAX), (-I64_MAX, -I64_MAX), (-I64_MAX, -1), (-I64_MAX, I64_MAX),
                   (I64_MIN, -1), (I64_MIN, I64_MAX)):
        yield 3, big[3], ("const", a), off
    yield 3, big[2], "random", -2
    yield 1, big[3], "random", 1


DATA = {
    "noise": lambda rng, n: rng.normal(0, 300, n).astype(np.int16),
    "ties": lambda rng, n: rng.integers(-1, 2, n).astype(np.int16),
    "constant": lambda rng, n: np.full(n, 7, np.int16),
    "full range": lambda rng, n: rng.integers(-32768, 32768, n).astype(np.int16),
    "extremes": lambda rng, n: np.where(np.arange(n) & 1, 32767, -32768).astype(np.int16),
}


@pytest.mark.parametrize("data", list(DATA))
def test_model_against_a_plain_loop(data):
    rng = np.random.default_rng(len(data))
    for Ns, Ls in (([20, 37], [4, 5]), ([64], [0]), ([3], [1]), ([1], [0]), ([50 * 2, 10 * 3 + 7, 55], [50, 10, 0])):
        y = DATA[data](rng, sum(Ns))
        length = wave_geometry(Ns, Ls)[1]
        W, n = length.size, int(length.max())
        for bin, n_bins, start, offset in cases_of(n):
            if start == "random":
                start = rng.integers(-8, n + 8, W)
            elif start is not None:
                start = np.full(W, start[1], dtype=object)
            what = (data, Ns, Ls, bin, n_bins, None if start is None else list(start)[:3], offset)
            same(wave_bins(y, Ns, Ls, bin, n_bins, start, offset), wave_bins_loop(y, Ns, Ls, bin, n_bins, start, offset), what)


def test_model_against_a_plain_loop_on_the_ragged_geometry():
    Ns, Ls = RAGGED
    rng = np.random.default_rng(5)
    y = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    W = wave_geometry(Ns, Ls)[1].size
    start = rng.integers(-300, 16384 + 300, W)
    for bin, n_bins, st, offset in ((1000, default_n_bins(Ns, Ls, 1000) + 5, None, 0), (250, 8, start, -500)):
        same(wave_bins(y, Ns, Ls, bin, n_bins, st, offset), wave_bins_loop(y, Ns, Ls, bin, n_bins, st, offset), (bin, n_bins, offset))


@pytest.mark.parametrize("bin", [1, 7, 512, 1000, 16384, 1 << 31])
def test_the_covering_bins_merge_to_wave_stats(bin):
    Ns, Ls = RAGGED
    y = np.random.default_rng(bin % 97).normal(0, 400, sum(Ns)).astype(np.int16)
    n_bins = default_n_bins(Ns, Ls, bin)
    assert n_bins == -(-16384 // bin)
    want = wave_stats(y, Ns, Ls, 0)[:, [4, 5, 0, 2]]  # SUM, SUMSQ, MIN, MAX
    same(merge(wave_bins(y, Ns, Ls, bin, n_bins)), want, bin)
    same(merge(wave_bins(y, Ns, Ls, bin, n_bins + 3, offset=-2 * bin)), want, bin)  # two empty bins in front, one more behind
    # and any split of the bins merges to the same
    r = wave_bins(y, Ns, Ls, bin, n_bins)
    if n_bins >= 2:
        halves = np.stack((merge(r[:, :n_bins // 2]), merge(r[:, n_bins // 2:])), axis=1)
        same(merge(halves), want, bin)
