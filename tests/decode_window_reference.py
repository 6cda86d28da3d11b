"""What drx_decode_window must return, in numpy, from the samples themselves:
windows(y, Ns, Ls, starts, offset, width, pad) -> int16 [waves, width].

Row g holds y_g[a_g + j] for j in [0, width) where 0 <= a_g + j < len_g, and pad elsewhere; a_g = starts[g] + offset
(starts None: 0; an int: the same for every waveform).  The geometry is geometry() of tests/test_gpu_select.py (which imports
without a GPU); tests/test_decode_window_abi.py holds windows() to a plain loop and checks a few rows by hand."""
import numpy as np

from test_gpu_select import geometry


def windows(y, Ns, Ls, starts, offset, width, pad, geom=None):
    first, length, _ = geom if geom is not None else geometry(Ns, Ls)
    W = first.size
    a = np.zeros(W, np.int64) if starts is None else np.broadcast_to(np.asarray(starts, np.int64), (W,))
    a = np.clip(a.astype(object) + int(offset), -(1 << 63), (1 << 63) - 1).astype(np.int64) if a.size else a  # the sum saturates
    a = np.clip(a, -(1 << 40), 1 << 40)  # (far outside any waveform either way: the index arithmetic below stays in int64)
    idx = a[:, None] + np.arange(width, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < length[:, None])
    src = np.where(inside, first[:, None] + idx, 0)
    y = np.asarray(y, np.int16)
    rows = y[src] if y.size else np.zeros(src.shape, np.int16)
    return np.where(inside, rows, np.int16(pad)).astype(np.int16)


def windows_loop(y, Ns, Ls, starts, offset, width, pad):
    """The same as plain Python, one sample at a time (for tiny inputs)."""
    first, length, _ = geometry(Ns, Ls)
    out = np.full((first.size, width), pad, np.int16)
    for g in range(first.size):
        a = (0 if starts is None else int(starts) if np.isscalar(starts) else int(starts[g])) + int(offset)
        for j in range(width):
            if 0 <= a + j < length[g]:
                out[g, j] = y[first[g] + a + j]
    return out
