"""What drx_wave_stack must return, in numpy, from the samples themselves:
(y, Ns, Ls, width, start, offset, select) -> int64 [width, 3].

y: the int16 samples of the batch, chunk after chunk; chunk c holds Ns[c] samples in waveforms of Ls[c] (0 or less: the whole
chunk), its last one possibly shorter.  Waveform g has the origin a = start[g] + offset, the sum saturating at the int64 ends
(start None: 0), and is selected when select is None or select[g] != 0.  Position j, 0 <= j < width, receives y_g[a + j] from
every selected g with 0 <= a + j < len_g.  Columns in the order of DRX_STACK_*: how many, their sum, the sum of their squares; a
position nobody reaches is (0, 0, 0).  The origin is a Python integer (nothing wraps).  wave_stack() adds a slice per waveform;
wave_stack_loop() is the same thing written as a plain loop over samples, against which tests/test_wave_stack_reference.py holds
it on tiny inputs."""
import numpy as np

from wave_bins_reference import origin
from wave_stats_reference import wave_geometry

COLS = 3


def default_width(Ns, Ls, offset=0):
    """The positions that some waveform reaches from `offset` with origins 0 (what Plan.wave_stack takes for width=None)."""
    longest = int(wave_geometry(Ns, Ls)[1].max())
    return max(0, longest - int(offset))


def wave_stack(y, Ns, Ls, width, start=None, offset=0, select=None):
    y = np.asarray(y, dtype=np.int16).reshape(-1).astype(np.int64)
    first, length = wave_geometry(Ns, Ls)
    assert first.size and int(first[-1] + length[-1]) == y.size and (length > 0).all()
    width = int(width)
    assert width >= 0
    out = np.zeros((width, COLS), dtype=np.int64)
    for g in range(first.size):
        if select is not None and not select[g]:
            continue
        at, n = int(first[g]), int(length[g])
        a = origin(start, g, offset)
        lo, hi = max(a, 0), min(a + width, n)  # the samples that land inside [0, width)
        if lo >= hi:
            continue
        v = y[at + lo:at + hi]
        out[lo - a:hi - a, 0] += 1
        out[lo - a:hi - a, 1] += v
        out[lo - a:hi - a, 2] += v * v
    return out


def wave_stack_loop(y, Ns, Ls, width, start=None, offset=0, select=None):
    """The same by a plain loop over waveforms and samples (tiny inputs only)."""
    y = [int(v) for v in np.asarray(y, dtype=np.int16).reshape(-1)]
    rows = [[0, 0, 0] for _ in range(width)]
    at, g = 0, 0
    for N, L in zip(Ns, Ls):
        L = L if L > 0 else N
        for i in range(0, N, L):
            if select is None or select[g]:
                a = origin(start, g, offset)
                for idx, v in enumerate(y[at + i:at + min(i + L, N)]):
                    j = idx - a
                    if 0 <= j < width:
                        rows[j][0] += 1
                        rows[j][1] += v
                        rows[j][2] += v * v
            g += 1
        at += N
    return np.array(rows, dtype=np.int64).reshape(width, COLS)
