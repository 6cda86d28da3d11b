"""The prediction filter, stated a second time (a helper module of the tests, not a conftest).

The oracle (oracle/deltarice_oracle.c) and the device code state the filter with one expression; this module states it
again, from the reference's source lines and not from the oracle, in Python / numpy-int64 integers:

  forward   src/deltaRice.c:64-74    out = x[i]*f[0]; out += x[i-j]*f[j] for 1 <= j < n_taps, i-j >= 0; `out` is a short,
                                      so every partial sum wraps to int16 (:51-63, the [1,-1] branch, is the same arithmetic)
  inverse   src/deltaRice.c:91-101   temp = d[i]; temp -= y[i-j]*f[j] likewise, a short; temp = temp / f[0], C's division
                                      (towards zero) of the promoted short by the int, stored to a short again
  words     src/deltaRice.c:207-241  zig-zag, code length q+1+k or 8+1+16, 32-bit words, the last one padded

A product x*f[j] overflows C's int once |f[j]| > 65536; there the reference is undefined and the project's definition is
the reading modulo 2^16, which exact Python integers give without a special case.

`forward` and `inverse` take one waveform, or several of one length along the last axis.  `forward_literal` and
`inverse_literal` are the source lines one operation at a time; tests/test_filter_reference.py holds the array forms to them.
FILTERS and DATA are the one table tests/test_filter_reference.py and tests/test_gpu_filter_domain.py both draw from.
"""
import hashlib

import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def wrap16(v):
    """What storing to a `short` keeps (two's complement), of a Python int or an int64 array."""
    return ((v + 32768) & 0xFFFF) - 32768


def is_delta(taps):
    return len(taps) == 2 and taps[0] == 1 and taps[1] == -1  # checkIfDeltaFilter, :38-46


def forward_literal(x, taps):
    x = [int(v) for v in x]
    out = []
    for i in range(len(x)):
        o = wrap16(x[i] * taps[0])                      # :67
        for j in range(1, len(taps)):                   # :68
            if i - j >= 0:                              # :69
                o = wrap16(o + x[i - j] * taps[j])      # :70
        out.append(o)                                   # :72
    return np.array(out, np.int16)


def inverse_literal(d, taps):
    d = [int(v) for v in d]
    y = []
    for i in range(len(d)):
        t = d[i]                                        # :94
        for j in range(1, len(taps)):                   # :95
            if i - j >= 0:                              # :96
                t = wrap16(t - y[i - j] * taps[j])      # :97
        q = abs(t) // abs(taps[0])                      # :99, towards zero
        t = wrap16(-q if (t < 0) != (taps[0] < 0) else q)
        y.append(t)                                     # :100
    return np.array(y, np.int16)


def forward(x, taps):
    """Residuals of the waveform(s) x (last axis: time).  Tap by tap in the source's order, every partial sum wrapped; all i at
    once, which is exact: a product is below 2^46 and a wrapped partial sum below 2^15."""
    x = np.asarray(x).astype(np.int64)
    n = x.shape[-1]
    out = wrap16(x * int(taps[0]))
    for j in range(1, min(len(taps), n)):
        out[..., j:] = wrap16(out[..., j:] + x[..., :n - j] * int(taps[j]))
    return out.astype(np.int16)


def inverse(d, taps):
    """Samples the residuals d decode to (last axis: time); serial in time, as the source is.  The wrapped difference of :97
    is taken once per sample instead of once per tap: wrapping is reduction modulo 2^16, which commutes with the additions, and
    the exact sum of at most 63 products below 2^46 fits int64 (held to inverse_literal by the tests)."""
    d = np.asarray(d).astype(np.int64)
    n, nt = d.shape[-1], len(taps)
    f = np.array([int(t) for t in taps[1:]], np.int64)[::-1]  # f[-j] = taps[j]
    lead = int(taps[0])
    y = np.zeros(d.shape, np.int64)
    for i in range(n):
        t = d[..., i]
        m = min(i, nt - 1)
        if m:
            t = t - (y[..., i - m:i] * f[nt - 1 - m:]).sum(axis=-1)
        t = wrap16(t)
        q = np.abs(t) // abs(lead)
        y[..., i] = wrap16(np.where((t < 0) != (lead < 0), -q, q))
    return y.astype(np.int16)


def code_bits(d, k):
    """Bits of each residual's code (:207-228): q + 1 + k, or 8 + 1 + 16 once q = z >> k reaches 8."""
    d = np.asarray(d).astype(np.int64)
    z = np.where(d < 0, -2 * d - 1, 2 * d)              # :208-211
    q = z >> k                                          # :212
    return np.where(q < 8, q + 1 + k, 25)               # :215-228


def words(d, k):
    """n_i of one waveform's residuals (:229-241)."""
    return int((int(code_bits(d, k).sum()) + 31) // 32)


def waveforms(n, L):
    """(first sample, length) of every waveform of a chunk of n samples (:399-403, :420-425); L <= 0: the whole chunk."""
    L = n if L <= 0 else L
    return [(s, min(L, n - s)) for s in range(0, n, L)]


def chunk_residuals(x, L, taps):
    """Residuals of a whole chunk: the waveforms of one length at once, a shorter last one on its own."""
    x = np.asarray(x).reshape(-1)
    n = x.size
    L = n if L <= 0 else L
    full = n // L
    out = np.empty(n, np.int16)
    if full:
        out[:full * L] = forward(x[:full * L].reshape(full, L), taps).reshape(-1)
    if n > full * L:
        out[full * L:] = forward(x[full * L:], taps)
    return out


def chunk_decoded(d, L, taps):
    d = np.asarray(d).reshape(-1)
    n = d.size
    L = n if L <= 0 else L
    full = n // L
    out = np.empty(n, np.int16)
    if full:
        out[:full * L] = inverse(d[:full * L].reshape(full, L), taps).reshape(-1)
    if n > full * L:
        out[full * L:] = inverse(d[full * L:], taps)
    return out


def chunk_wave_words(d, L, k):
    """n_i of every waveform of a chunk whose residuals are d."""
    d = np.asarray(d).reshape(-1)
    return [words(d[s:s + n], k) for s, n in waveforms(d.size, L)]


def opts_of(m, L, taps):
    """compression_opts of a filter (negative taps as HDF5's unsigned cd_values carry them)."""
    return (m, L, len(taps)) + tuple(int(t) & 0xFFFFFFFF for t in taps)


# ---- the table ---------------------------------------------------------------------------------------------------------

N_TAPS = (1, 2, 3, 4, 5, 6, 8, 16, 33, 63, 64)
LEADS = (1, -1, 2, -3, 32767, -32767)
MAGNITUDES = (3, 200, 32767)

NAMED = {
    "delta0": (1, -1, 0),                        # not checkIfDeltaFilter's filter (three taps), yet the delta plan's bytes
    "delta00": (1, -1, 0, 0),
    "identity_mod": (1, 65536),                  # the identity modulo 2^16
    "lead_65537": (65537, -1),                   # a lead that is 1 modulo 2^16 and is not 1: lossy on decode
    "lead_m65535": (-65535, 3, 3),
    "i32_extremes": (1, I32_MAX, I32_MIN, 65536, -65537),
    "half_range": (-1, 65535, 32768, -32768),
    "lead_i32min": (I32_MIN, 1, 1),
    "lead_i32max": (I32_MAX, -1),
    "lead_m2": (-2, 1),                          # C's division by a negative divisor that is no unit (:99)
    "lead_m7": (-7, 3, 3),
    "mixed7": (3, -70000, 70001, 5, 5, 5, 9),
}


def _seeded():
    rng = np.random.default_rng(20261017)
    out = {}
    for a, nt in enumerate(N_TAPS):
        for b, lead in enumerate(LEADS):
            mag = MAGNITUDES[(a + b) % 3]        # every (n_taps, lead) once, every (n_taps, magnitude) twice
            rest = [int(v) for v in rng.integers(-mag, mag + 1, nt - 1)]
            if nt > 1 and rest[-1] == 0:
                rest[-1] = mag                   # the last tap counts: n_taps is what it says
            if nt == 2 and lead == 1 and rest == [-1]:
                rest = [-2]                      # (not the delta filter: that one is not this table's subject)
            out[f"t{nt}_lead{lead}_mag{mag}"] = (lead,) + tuple(rest)
    return out


FILTERS = {**_seeded(), **NAMED}                 # name -> taps


def lossless(taps):
    return abs(taps[0]) == 1


def _steps(rng, n):  # as tests/test_gpu_parity.make_data: rare huge jumps -> isolated escapes
    x = rng.normal(0, 3, n)
    x[rng.integers(0, n, max(1, n // 500))] += rng.choice([-30000, 30000])
    return x.clip(-32768, 32767).astype(np.int16)


def _alternating(rng, n):
    x = np.full(n, -32768, np.int16)
    x[1::2] = 32767
    return x


DATA = {
    "uniform": lambda rng, n: rng.integers(-32768, 32768, n).astype(np.int16),
    "gauss50": lambda rng, n: rng.normal(0, 50, n).astype(np.int16),
    "rails_low": lambda rng, n: np.full(n, -32768, np.int16),
    "rails_high": lambda rng, n: np.full(n, 32767, np.int16),
    "rails_alternating": _alternating,
    "steps": _steps,
}


def make_data(kind, n, seed=0):
    return DATA[kind](np.random.default_rng((sum(map(ord, kind)), n, seed)), n)


# ---- the cases ---------------------------------------------------------------------------------------------------------

def shapes(n_taps):
    """(WaveformLength, chunk samples, RiceParameter) of the cases every filter is run at: three waveforms with a short last
    one; waveforms shorter than any filter but the one-tap ones; waveforms one short of the filter (L < n_taps) with a short
    last one; waveforms of exactly the filter's length; and the first length past the 64-entry history."""
    return [(1000, 2500, 8), (3, 31, 2), (max(n_taps - 1, 1), 4 * n_taps + 1, 256), (n_taps, 3 * n_taps, 32768), (65, 200, 32)]


def cases(name):
    """(kind, L, n, m, x) of every case of one filter."""
    for L, n, m in shapes(len(FILTERS[name])):
        for kind in DATA:
            yield kind, L, n, m, make_data(kind, n)


def in_reference_domain(taps, L, n, wave_words):
    """Where the reference's compiled code (its OpenMP build) is defined at all, SURVEY.md Appendix B: no product
    input[i-j]*filt[j] overflows an int (B14; |tap| <= 32767 suffices), L >= 4 W (B5), and -- B5 to the byte, which a short last
    waveform needs -- header and payload of every waveform lie inside the staging buffer of 2*nbytes + W + 1 bytes
    (src/deltaRice.c:411-412) when written at word i*(L+1) + 1 (:421-424).  wave_words: n_i of the chunk's waveforms."""
    W = -(-n // L)
    if max(abs(t) for t in taps) > 32767 or (W > 1 and L < 4 * W):
        return False
    return all(4 * (i * (L + 1) + 2 + n_i) <= 4 * n + W + 1 for i, n_i in enumerate(wave_words))


def digests(name, encode, decode):
    """One filter's entry of ref_filters.json, from any encoder / decoder: over its cases inside the reference's domain."""
    taps = FILTERS[name]
    hx, hw, hy = hashlib.sha256(), hashlib.sha256(), hashlib.sha256()
    n_cases = n_words = 0
    for kind, L, n, m, x in cases(name):
        k = m.bit_length() - 1
        if not in_reference_domain(taps, L, n, chunk_wave_words(chunk_residuals(x, L, taps), L, k)):
            continue
        opts = opts_of(m, L, taps)
        w = encode(x, opts)
        hx.update(x.tobytes())
        hw.update(w.tobytes())
        hy.update(decode(w, opts).tobytes())
        n_cases += 1
        n_words += int(w.size)
    if not n_cases:
        return None
    return {"filter": name, "taps": list(taps), "n_cases": n_cases, "n_words": n_words, "sha256_input": hx.hexdigest(),
            "sha256_words": hw.hexdigest(), "sha256_decoded": hy.hexdigest()}
