"""What drx_wave_stats must return, in numpy, from the samples themselves: (x, Ns, Ls, head) -> int64 [W, 8].

x: the int16 samples of the batch, chunk after chunk; chunk c holds Ns[c] samples in waveforms of Ls[c] (0 or less: the whole
chunk), its last one possibly shorter.  Columns in the order of DRX_STAT_*: min, argmin, max, argmax, sum, sum of squares, head
sum, head sum of squares; first occurrences; the head window is the first min(head, len) samples.  Vectorised over the batch
(the waveforms tile x without gaps, so every column is a reduceat or a difference of running sums); wave_stats_loop() is the
same thing written as plain Python, against which tests/test_wave_stats_abi.py holds it on tiny inputs."""
import numpy as np

COLS = 8


def wave_geometry(Ns, Ls):
    """-> (first sample, length) of every waveform, int64 each."""
    start, length, at = [], [], 0
    for N, L in zip(Ns, Ls):
        N, L = int(N), int(L)
        L = L if L > 0 else N
        s = np.arange(0, N, L, dtype=np.int64)
        start.append(at + s)
        length.append(np.minimum(L, N - s))
        at += N
    return np.concatenate(start), np.concatenate(length)


def wave_stats_heads(x, Ns, Ls, heads):
    """-> one int64 [W, 8] per entry of heads (the columns that do not depend on the window are computed once)."""
    x = np.asarray(x, dtype=np.int16).reshape(-1).astype(np.int64)
    start, length = wave_geometry(Ns, Ls)
    assert start.size and int(start[-1] + length[-1]) == x.size and (length > 0).all()
    base = np.zeros((start.size, COLS), dtype=np.int64)
    pos = np.arange(x.size, dtype=np.int64)
    for col, red in ((0, np.minimum), (2, np.maximum)):
        ext = red.reduceat(x, start)
        hit = np.where(x == np.repeat(ext, length), pos, np.int64(x.size))
        base[:, col] = ext
        base[:, col + 1] = np.minimum.reduceat(hit, start) - start
    s1 = np.concatenate(([0], np.cumsum(x)))
    s2 = np.concatenate(([0], np.cumsum(x * x)))
    base[:, 4] = s1[start + length] - s1[start]
    base[:, 5] = s2[start + length] - s2[start]
    out = []
    for head in heads:
        h = np.minimum(np.int64(head), length)
        r = base.copy()
        r[:, 6] = s1[start + h] - s1[start]
        r[:, 7] = s2[start + h] - s2[start]
        out.append(r)
    return out


def wave_stats(x, Ns, Ls, head):
    return wave_stats_heads(x, Ns, Ls, [head])[0]


def wave_stats_loop(x, Ns, Ls, head):
    """The same by a plain loop over waveforms and samples (tiny inputs only)."""
    x = [int(v) for v in np.asarray(x, dtype=np.int16).reshape(-1)]
    rows, at = [], 0
    for N, L in zip(Ns, Ls):
        L = L if L > 0 else N
        for i in range(0, N, L):
            y = x[at + i:at + min(i + L, N)]
            mn = mx = y[0]
            amn = amx = 0
            s = ss = hs = hss = 0
            for j, v in enumerate(y):
                if v < mn:
                    mn, amn = v, j
                if v > mx:
                    mx, amx = v, j
                s += v
                ss += v * v
                if j < head:
                    hs += v
                    hss += v * v
            rows.append([mn, amn, mx, amx, s, ss, hs, hss])
        at += N
    return np.array(rows, dtype=np.int64)
