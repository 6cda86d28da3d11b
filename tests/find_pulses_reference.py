"""What drx_find_pulses must return, in numpy, from the samples themselves:
find_pulses(y, Ns, Ls, thr, polarity, min_width, max_pulses, thr_tab=None) -> (count int32 [waves], pulses int64 [waves, max_pulses, 5]).

Waveform g has the threshold t_g = (thr_tab[g] if thr_tab is not None else 0) + thr, the sum saturating at the int64 ends.
Sample i is over when polarity > 0 and y[i] > t_g, or polarity < 0 and y[i] < t_g; a run is a maximal range [s, e) of consecutive
over samples of one waveform, a pulse a run with e - s >= min_width, numbered by s.  count[g]: all pulses of waveform g.  Slot
p < min(count[g], max_pulses) of row g: (s, e - s, the run's extreme in the polarity's direction, its first place, the run's sum);
every other slot zero.  The geometry is geometry() of tests/test_gpu_select.py (which imports without a GPU);
tests/test_find_pulses_abi.py holds find_pulses() to a plain loop and checks rows by hand."""
import numpy as np

from test_gpu_select import geometry

START, WIDTH, PEAK, ARGPEAK, SUM, COLS = 0, 1, 2, 3, 4, 5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def thresholds(W, thr, thr_tab=None):
    """t_g as int64: the saturating sum"""
    tab = np.zeros(W, np.int64) if thr_tab is None else np.asarray(thr_tab, np.int64)
    assert tab.shape == (W,)
    return np.array([min(max(int(v) + int(thr), I64_MIN), I64_MAX) for v in tab], np.int64).reshape(W)


def runs_of(y, Ns, Ls, thr, polarity, thr_tab=None, geom=None):
    """Every run of the batch, in order: (waveform, s, e) as int64 arrays, and the flat position of every run's first sample."""
    first, length, _ = geom if geom is not None else geometry(Ns, Ls)
    # (any threshold beyond the int16 range compares as its nearest neighbour outside it: the large batches stay in int32)
    t = np.repeat(np.clip(thresholds(first.size, thr, thr_tab), -32769, 32768).astype(np.int32), length)
    v = np.asarray(y, np.int16).astype(np.int32)
    over = v > t if polarity > 0 else v < t
    prev = np.concatenate([[False], over[:-1]])
    prev[first] = False  # a run may begin at sample 0, and does not come over from the waveform before
    nxt = np.concatenate([over[1:], [False]])
    nxt[first + length - 1] = False  # a run still open at the last sample ends there
    a = np.flatnonzero(over & ~prev)
    b = np.flatnonzero(over & ~nxt) + 1
    g = np.searchsorted(first, a, side="right") - 1
    return g, a - first[g], b - first[g], a


def find_pulses(y, Ns, Ls, thr, polarity, min_width, max_pulses, thr_tab=None, geom=None):
    assert polarity != 0 and min_width >= 1 and max_pulses >= 0
    first, length, _ = geom if geom is not None else geometry(Ns, Ls)
    W = first.size
    g, s, e, a = runs_of(y, Ns, Ls, thr, polarity, thr_tab, (first, length, None))
    keep = e - s >= min_width
    g, s, e, a = g[keep], s[keep], e[keep], a[keep]
    count = np.bincount(g, minlength=W).astype(np.int64)
    out = np.zeros((W, max_pulses, COLS), np.int64)
    if g.size and max_pulses:
        rank = np.arange(g.size) - (np.cumsum(count) - count)[g]  # the pulse's number inside its waveform
        fits = rank < max_pulses
        g, s, e, a, rank = g[fits], s[fits], e[fits], a[fits], rank[fits]
        v = np.concatenate([np.asarray(y, np.int16), np.zeros(1, np.int16)])  # (a sentinel: reduceat takes no index == size)
        w = e - s
        bounds = np.stack([a, a + w], axis=1).reshape(-1)
        peak = (np.maximum if polarity > 0 else np.minimum).reduceat(v, bounds)[::2].astype(np.int64)
        total = np.add.reduceat(v, bounds, dtype=np.int64)[::2]
        run_of = np.repeat(np.arange(g.size), w)  # of every sample of every kept run
        pos = np.repeat(a, w) + (np.arange(w.sum()) - np.repeat(np.cumsum(w) - w, w))
        at_peak = np.where(v[pos] == peak[run_of], pos, v.size)
        arg = np.minimum.reduceat(at_peak, np.cumsum(w) - w) - a + s
        out[g, rank] = np.stack([s, w, peak, arg, total], axis=1)
    return count.astype(np.int32), out


def find_pulses_loop(y, Ns, Ls, thr, polarity, min_width, max_pulses, thr_tab=None):
    """The same as plain Python, one sample at a time (for tiny inputs)."""
    first, length, _ = geometry(Ns, Ls)
    W = first.size
    count, out = np.zeros(W, np.int32), np.zeros((W, max_pulses, COLS), np.int64)
    for g in range(W):
        t = (0 if thr_tab is None else int(thr_tab[g])) + int(thr)
        t = min(max(t, I64_MIN), I64_MAX)
        yy = [int(v) for v in y[first[g]:first[g] + length[g]]]
        i, n = 0, len(yy)
        while i < n:
            if not (yy[i] > t if polarity > 0 else yy[i] < t):
                i += 1
                continue
            s = i
            while i < n and (yy[i] > t if polarity > 0 else yy[i] < t):
                i += 1
            if i - s >= min_width:
                if count[g] < max_pulses:
                    run = yy[s:i]
                    pk = max(run) if polarity > 0 else min(run)
                    out[g, count[g]] = [s, i - s, pk, s + run.index(pk), sum(run)]
                count[g] += 1
    return count, out
