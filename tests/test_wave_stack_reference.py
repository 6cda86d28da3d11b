"""CPU: the numpy model the GPU tests of drx_wave_stack compare against (tests/wave_stack_reference.py), held to rows worked by
hand, to a plain per-sample loop on tiny inputs, and to wave_stats_reference: the whole-waveform stack sums to the waveforms'
SUMs, and its COUNT column is the number of waveforms longer than the position."""
import numpy as np
import pytest

from test_wave_bins_reference import DATA, RAGGED
from wave_stack_reference import default_width, wave_stack, wave_stack_loop
from wave_stats_reference import wave_geometry, wave_stats

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    assert np.array_equal(got, want), what


def test_model_by_hand():
    # two chunks: 10 samples in waveforms of 4 (the last one of 2), then 7 samples in one waveform
    #             w0            w1            w2      w3
    y = np.array([5, 9, 1, 1,   1, 6, 6, 1,   7, 8,   0, 9, -9, 3, 0, 9, 0], np.int16)
    Ns, Ls = [10, 7], [4, 0]
    assert default_width(Ns, Ls) == 7 and default_width(Ns, Ls, 3) == 4 and default_width(Ns, Ls, -2) == 9 and default_width(Ns, Ls, 7) == 0
    r = wave_stack(y, Ns, Ls, 7)
    assert r.tolist() == [[4, 13, 75], [4, 32, 262], [3, -2, 118], [3, 5, 11], [1, 0, 0], [1, 9, 81], [1, 0, 0]]
    assert wave_stack(y, Ns, Ls, 9)[7:].tolist() == [[0, 0, 0]] * 2  # positions nobody reaches
    assert wave_stack(y, Ns, Ls, 2).tolist() == r[:2].tolist()
    # per-waveform origins and an offset: a = -2, 2, 8, 4
    st = np.array([-1, 3, 9, 5])
    assert wave_stack(y, Ns, Ls, 3, st, -1).tolist() == [[2, 6, 36], [2, 10, 82], [2, 5, 25]]
    assert wave_stack(y, Ns, Ls, 3, st, -1, select=[1, 0, 1, 1]).tolist() == [[1, 0, 0], [1, 9, 81], [2, 5, 25]]
    assert wave_stack(y, Ns, Ls, 3, st, -1, select=[0, 0, 0, 0]).tolist() == [[0, 0, 0]] * 3
    assert wave_stack(y, Ns, Ls, 0).shape == (0, 3)
    # start + offset saturates at both int64 ends (it does not wrap round into the waveform)
    far = np.array([I64_MAX, I64_MIN, I64_MAX, I64_MIN])
    assert wave_stack(y, Ns, Ls, 3, far, I64_MAX).tolist() == [[0, 0, 0], [2, 1, 1], [2, 15, 117]]  # min + max = -1: w1 and w3
    assert wave_stack(y, Ns, Ls, 3, far, I64_MIN).tolist() == [[0, 0, 0], [2, 12, 74], [2, 17, 145]]  # max + min = -1: w0 and w2
    assert not wave_stack(y, Ns, Ls, 3, far, 0).any()


def test_seventy_thousand_minimal_samples_do_not_wrap():
    y = np.full(70000, -32768, np.int16)
    r = wave_stack(y, [70000], [1], 1)
    assert r.tolist() == [[70000, -32768 * 70000, (1 << 30) * 70000]]
    assert r[0, 1] < -(1 << 31) and r[0, 2] > 1 << 46


def cases_of(n, W, rng):
    """(width, start, offset, select) over a geometry of W waveforms whose longest has n samples"""
    for width in sorted({0, 1, n // 2 + 1, n - 1, n, n + 1, n + 9}):
        if width >= 0:
            yield width, None, 0, None
    for a in (-5, 0, n - 1, n):
        yield n + 3, np.full(W, a, dtype=object), 0, None
    for a, off in ((I64_MAX, I64_MAX), (I64_MAX, 1), (I64_MAX, -I64_MAX), (-I64_MAX, -I64_MAX), (-I64_MAX, -1), (-I64_MAX, I64_MAX),
                   (I64_MIN, -1), (I64_MIN, I64_MAX)):
        yield n + 7, np.full(W, a, dtype=object), off, None
    start = rng.integers(-8, n + 8, W)
    one = np.zeros(W, np.uint8)
    one[W // 2] = 1
    for select in (None, np.ones(W, np.uint8), np.zeros(W, np.uint8), one, rng.integers(0, 2, W).astype(np.uint8)):
        yield n // 3 + 1, start, -2, select
        yield n + 7, start, 1, select
        yield n, None, 0, select


@pytest.mark.parametrize("data", list(DATA))
def test_model_against_a_plain_loop(data):
    rng = np.random.default_rng(len(data))
    for Ns, Ls in (([20, 37], [4, 5]), ([64], [0]), ([3], [1]), ([1], [0]), ([50 * 2, 10 * 3 + 7, 55], [50, 10, 0])):
        y = DATA[data](rng, sum(Ns))
        length = wave_geometry(Ns, Ls)[1]
        W, n = length.size, int(length.max())
        for width, start, offset, select in cases_of(n, W, rng):
            what = (data, Ns, Ls, width, None if start is None else list(start)[:3], offset, None if select is None else select.tolist()[:5])
            same(wave_stack(y, Ns, Ls, width, start, offset, select), wave_stack_loop(y, Ns, Ls, width, start, offset, select), what)


def test_model_against_a_plain_loop_on_the_ragged_geometry():
    Ns, Ls = RAGGED
    rng = np.random.default_rng(5)
    y = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    W = wave_geometry(Ns, Ls)[1].size
    start = rng.integers(-300, 16384 + 300, W)
    select = rng.integers(0, 2, W).astype(np.uint8)
    for width, st, offset, sel in ((default_width(Ns, Ls) + 5, None, 0, None), (300, start, -64, select)):
        same(wave_stack(y, Ns, Ls, width, st, offset, sel), wave_stack_loop(y, Ns, Ls, width, st, offset, sel), (width, offset))


@pytest.mark.parametrize("sigma", [10, 400])
def test_the_whole_waveform_stack_against_wave_stats(sigma):
    Ns, Ls = RAGGED
    y = np.random.default_rng(sigma).normal(0, sigma, sum(Ns)).astype(np.int16)
    length = wave_geometry(Ns, Ls)[1]
    width = default_width(Ns, Ls)
    assert width == 16384
    r = wave_stack(y, Ns, Ls, width)
    stats = wave_stats(y, Ns, Ls, 0)
    assert int(r[:, 1].sum()) == int(stats[:, 4].sum()) and int(r[:, 2].sum()) == int(stats[:, 5].sum())
    same(r[:, 0], (length[None, :] > np.arange(width)[:, None]).sum(axis=1).astype(np.int64), "COUNT[j] = waveforms longer than j")
    # results of two halves of the batch add
    half = (np.arange(length.size) < length.size // 2).astype(np.uint8)
    same(wave_stack(y, Ns, Ls, width, select=half) + wave_stack(y, Ns, Ls, width, select=1 - half), r, "halves add")
