"""What drx_wave_bins must return, in numpy, from the samples themselves:
(x, Ns, Ls, bin, n_bins, start, offset) -> int64 [W, n_bins, 4].

x: the int16 samples of the batch, chunk after chunk; chunk c holds Ns[c] samples in waveforms of Ls[c] (0 or less: the whole
chunk), its last one possibly shorter.  Waveform g has the origin a = start[g] + offset, the sum saturating at the int64 ends
(start None: 0); bin b holds the samples with index in [a + b * bin, a + (b + 1) * bin) and in [0, len).  Columns in the order
of DRX_BIN_*: sum, sum of squares, min, max; a bin without a sample is EMPTY = (0, 0, 32767, -32768).  The origin and the bin
ends are Python integers (nothing wraps); per waveform the bins that receive a sample are consecutive, so every column is a
reduceat or a difference of running sums over the covered stretch.  wave_bins_loop() is the same thing written as a plain loop
over samples, against which tests/test_wave_bins_reference.py holds it on tiny inputs."""
import numpy as np

from wave_stats_reference import wave_geometry

COLS = 4
EMPTY = (0, 0, 32767, -32768)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def origin(start, g, offset):
    """a_g as a Python int: start[g] + offset, saturating at the int64 ends."""
    a = int(offset) + (0 if start is None else int(start[g]))
    return min(max(a, I64_MIN), I64_MAX)


def default_n_bins(Ns, Ls, bin, offset=0):
    """Enough bins to cover the longest waveform from `offset` (what Plan.wave_bins takes for n_bins=None)."""
    longest = int(wave_geometry(Ns, Ls)[1].max())
    return max(0, -(-(longest - int(offset)) // int(bin)))


def wave_bins(x, Ns, Ls, bin, n_bins, start=None, offset=0):
    x = np.asarray(x, dtype=np.int16).reshape(-1).astype(np.int64)
    first, length = wave_geometry(Ns, Ls)
    assert first.size and int(first[-1] + length[-1]) == x.size and (length > 0).all()
    bin, n_bins = int(bin), int(n_bins)
    assert bin >= 1 and n_bins >= 0
    out = np.empty((first.size, n_bins, COLS), dtype=np.int64)
    out[:] = np.array(EMPTY, dtype=np.int64)
    s1 = np.concatenate(([0], np.cumsum(x)))
    s2 = np.concatenate(([0], np.cumsum(x * x)))
    for g in range(first.size):
        at, n = int(first[g]), int(length[g])
        a = origin(start, g, offset)
        lo, hi = max(a, 0), min(a + n_bins * bin, n)
        if lo >= hi:
            continue
        b0, b1 = (lo - a) // bin, (hi - 1 - a) // bin
        edges = np.array([min(max(a + b * bin, lo), hi) for b in (b0, b1 + 1)], dtype=np.int64)
        if b1 > b0:  # (the ends between b0 and b1 lie inside [lo, hi))
            edges = np.concatenate((edges[:1], (a + b0 * bin) + np.arange(1, b1 - b0 + 1, dtype=np.int64) * bin, edges[1:]))
        assert (np.diff(edges) > 0).all()
        e = at + edges
        out[g, b0:b1 + 1, 0] = s1[e[1:]] - s1[e[:-1]]
        out[g, b0:b1 + 1, 1] = s2[e[1:]] - s2[e[:-1]]
        y = x[at + lo:at + hi]
        out[g, b0:b1 + 1, 2] = np.minimum.reduceat(y, edges[:-1] - lo)
        out[g, b0:b1 + 1, 3] = np.maximum.reduceat(y, edges[:-1] - lo)
    return out


def wave_bins_loop(x, Ns, Ls, bin, n_bins, start=None, offset=0):
    """The same by a plain loop over waveforms and samples (tiny inputs only; n_bins rows are held in a dict until the end)."""
    x = [int(v) for v in np.asarray(x, dtype=np.int16).reshape(-1)]
    rows, at, g = [], 0, 0
    for N, L in zip(Ns, Ls):
        L = L if L > 0 else N
        for i in range(0, N, L):
            y = x[at + i:at + min(i + L, N)]
            a = origin(start, g, offset)
            acc = {}
            for j, v in enumerate(y):
                if j < a:
                    continue
                b = (j - a) // bin
                if b >= n_bins:
                    continue
                r = acc.setdefault(b, list(EMPTY))
                r[0] += v
                r[1] += v * v
                r[2] = min(r[2], v)
                r[3] = max(r[3], v)
            rows.append(acc)
            g += 1
        at += N
    out = np.empty((len(rows), n_bins, COLS), dtype=np.int64)
    out[:] = np.array(EMPTY, dtype=np.int64)
    for g, acc in enumerate(rows):
        for b, r in acc.items():
            out[g, b] = r
    return out


def merge(rows):
    """int64 [..., n, 4] -> [..., 4]: neighbouring bins merged -- add, add, min, max, with no special case for an empty bin."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.stack((rows[..., 0].sum(-1), rows[..., 1].sum(-1), rows[..., 2].min(-1), rows[..., 3].max(-1)), axis=-1)
