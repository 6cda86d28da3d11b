"""What drx_decode_windows must return, in numpy, from the samples themselves:
windows_multi(y, Ns, Ls, starts, counts, offset, width, pad) -> int16 [waves, K, width].

Slot p of waveform g is live when p < min(counts[g], K) (counts None: every slot).  A live row holds y_g[a + j] for j in
[0, width) where 0 <= a + j < len_g and pad elsewhere, a = starts[g, p] + offset (saturating); a row that is not live is all pad.
Built on windows() of tests/decode_window_reference.py, a slot at a time; tests/test_decode_windows_abi.py holds it to a plain
loop and checks rows by hand."""
import numpy as np

from decode_window_reference import windows
from test_gpu_select import geometry


def windows_multi(y, Ns, Ls, starts, counts, offset, width, pad, geom=None):
    geom = geom if geom is not None else geometry(Ns, Ls)
    W = geom[0].size
    starts = np.asarray(starts, np.int64).reshape(W, -1)
    K = starts.shape[1]
    out = np.full((W, K, width), pad, np.int16)
    live = np.full(W, K, np.int64) if counts is None else np.minimum(np.asarray(counts, np.int64), K)
    for p in range(K):
        rows = windows(y, Ns, Ls, starts[:, p], offset, width, pad, geom)
        out[:, p] = np.where((p < live)[:, None], rows, np.int16(pad))
    return out


def windows_multi_loop(y, Ns, Ls, starts, counts, offset, width, pad):
    """The same as plain Python, one sample at a time (for tiny inputs)."""
    first, length, _ = geometry(Ns, Ls)
    W = first.size
    starts = np.asarray(starts, np.int64).reshape(W, -1)
    K = starts.shape[1]
    out = np.full((W, K, width), pad, np.int16)
    for g in range(W):
        for p in range(K if counts is None else min(int(counts[g]), K)):
            a = min(max(int(starts[g, p]) + int(offset), -(1 << 63)), (1 << 63) - 1)
            for j in range(width):
                if 0 <= a + j < length[g]:
                    out[g, p, j] = y[first[g] + a + j]
    return out


def extents(Ns, Ls, starts, counts, offset, width):
    """e_g of every waveform: the largest min(a + width, len_g) over its live windows that hold a sample, or 0."""
    first, length, _ = geometry(Ns, Ls)
    W = first.size
    starts = np.asarray(starts, np.int64).reshape(W, -1)
    e = np.zeros(W, np.int64)
    for g in range(W):
        for p in range(starts.shape[1] if counts is None else min(int(counts[g]), starts.shape[1])):
            a = min(max(int(starts[g, p]) + int(offset), -(1 << 63)), (1 << 63) - 1)
            if a < length[g] and a + width > 0:
                e[g] = max(e[g], min(a + width, int(length[g])))
    return e
