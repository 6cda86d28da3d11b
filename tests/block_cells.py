"""The cells over which the block forms of drx_wave_stats, drx_find_pulses, drx_decode_windows and drx_transcode /
drx_estimate_words_encoded are held to their references (tests/test_gpu_block_forms_parameters.py), and a CPU model of the
block geometry that says which template instantiation a cell runs (tests/test_block_cells_model.py asserts what the table
claims; tests/test_blk_rule_host.py pins the model to the C++).  A plain helper module: numpy and the oracle, no GPU.

A cell is (k, WaveformLength, data kind): a uniform plan of 2 chunks x 3 waveforms at RiceParameter 2^k, the last waveform of
each chunk a third shorter, samples of one of KINDS.  A block of the scheme is `lanes` x `words per lane` stream words:
  lanes           nt_for_len(WaveformLength, k)                       (csrc/drx_blocks.h:66-70, with blk_words() :64 and
                                                                      blk_segw_plan() :42)
  words per lane  blk_segw_bits10(320 * in_words / total_samples)     (csrc/drx_blocks.h:43; blk_bits10(), csrc/drx_blocks.hip:212,
                                                                      over the call's in_words and the plan's samples)
  lane share      blk_lane_cap(words per lane) samples staged         (csrc/drx_blocks.h:44)
and each of the four forms has one instantiation of its kernel per (lanes, words per lane) pair: 3 x 4 = 12."""
import functools

import numpy as np

from test_gpu_select import geometry, header_table


# --------------------------------------------------------------------------- the geometry rules, mirrored
def blk_segw_plan(k):  # drx_blocks.h:42
    return 11 if k <= 4 else (15 if k <= 7 else 19)


def blk_segw_bits10(b10):  # drx_blocks.h:43
    return 19 if b10 >= 117 else (15 if b10 >= 82 else (11 if b10 >= 54 else 9))


def blk_lane_cap(segw):  # drx_blocks.h:44
    return 76 if segw <= 11 else (68 if segw == 15 else 60)


def blk_words(nt, k):  # drx_blocks.h:64
    return nt * blk_segw_plan(k)


def nt_for_len(wave_len, k):  # drx_blocks.h:66-70
    typ_words = (wave_len * (2 * k + 7)) >> 6
    return 64 if typ_words <= blk_words(64, k) else (128 if typ_words <= blk_words(128, k) else 256)


def blk_bits10(in_words, total_samples):  # drx_blocks.hip:212
    return 320 * in_words // total_samples if total_samples else 65


# --------------------------------------------------------------------------- the data kinds
KINDS = ("matched", "quiet", "zeros", "uniform", "steps", "stretch")


def sigma_of(k, kind):
    """The scale of a cell's samples: what its pulse thresholds are multiples of."""
    return {"matched": max(0.7, 2.0 ** k / 2), "stretch": max(0.7, 2.0 ** k / 2), "quiet": 1.0, "zeros": 0.0, "uniform": 8000.0,
            "steps": 3.0}[kind]


def gauss(rng, sigma, n):
    return np.clip(rng.normal(0, sigma, n), -32768, 32767).astype(np.int16)


def samples(k, L, kind, Ns, Ls):
    """The int16 samples of a cell over the plan (Ns, Ls); a shorter last waveform is a prefix of the full one's samples."""
    full = [3 * L] * len(Ns)
    rng = np.random.default_rng([k, L, KINDS.index(kind)])
    n = sum(full)
    if kind in ("matched", "stretch", "quiet"):
        x = gauss(rng, sigma_of(k, kind), n)
    elif kind == "zeros":
        x = np.zeros(n, np.int16)
    elif kind == "uniform":
        x = rng.integers(-32768, 32768, n).astype(np.int16)  # deltas all over 17 bits: next to every code an escape
    elif kind == "steps":
        x = gauss(rng, 3, n)
        x[np.arange(n) % 1500 < 40] += 8000  # pulses, and escapes among short codes
    if kind == "stretch":  # a zero stretch over the middle third of every waveform
        start, length, _ = geometry(full, Ls)
        for s, l in zip(start, length):
            x[s + l // 3:s + 2 * l // 3] = 0
    parts, at = [], 0
    for N, F in zip(Ns, full):
        parts.append(x[at:at + N])
        at += F
    return np.ascontiguousarray(np.concatenate(parts))


# --------------------------------------------------------------------------- a cell's stream and its measured class
class Cell:
    """One cell; last: the length of each chunk's last waveform (None: a third shorter than the others)."""

    def __init__(self, k, L, kind, last=None):
        self.k, self.L, self.kind, self.m = k, L, kind, 1 << k
        self.last = L - L // 3 if last is None else last
        assert 1 <= self.last <= L
        self.Ns, self.Ls = [2 * L + self.last] * 2, [L] * 2
        self.sigma = sigma_of(k, kind)

    @property
    def id(self):
        return f"k{self.k}-L{self.L}-{self.kind}"

    def x(self):
        return samples(self.k, self.L, self.kind, self.Ns, self.Ls)

    def __repr__(self):
        return f"Cell({self.k}, {self.L}, {self.kind!r}, last={self.last})"


def encode(O, cell, x=None, taps=None):
    """(words, chunk offsets, n_i of every waveform) of the oracle's stream of the cell."""
    x = cell.x() if x is None else x
    ftaps = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()
    words, offs, at = [], [0], 0
    for N, L in zip(cell.Ns, cell.Ls):
        w = O.encode_chunk(x[at:at + N], (cell.m, L) + ftaps)
        words.append(w)
        offs.append(offs[-1] + w.size)
        at += N
    words, offs = np.concatenate(words), np.array(offs, np.int64)
    return words, offs, header_table(words, offs, cell.Ns, cell.Ls)


def code_lengths(x, cell):
    """The code length of every sample that has a predecessor in its waveform (a delta's zig-zag value z at parameter k:
    z >> k < 8: that many zeros, a one, k bits; else the 25-bit escape), and the waveform of each."""
    start, length, _ = geometry(cell.Ns, cell.Ls)
    d = np.diff(x.astype(np.int64)).astype(np.int16).astype(np.int64)  # (the delta wraps in 16 bits)
    z = ((d << 1) ^ (d >> 15)) & 0xFFFF
    q = z >> cell.k
    bits = np.where(q < 8, q + 1 + cell.k, 25)
    inner = np.ones(x.size, bool)
    inner[start] = False
    wave = np.repeat(np.arange(start.size), length)
    return bits[inner[1:]], wave[1:][inner[1:]]


def measure(O, cell):
    """What the cell's stream makes the kernels do: a dict of k, L, kind, lanes, sw (words per lane), cap, bits (per sample),
    B (words per block), n_i, passes (True: some lane provably holds more codes than its share), lengths (distinct code lengths)."""
    x = cell.x()
    words, offs, n_i = encode(O, cell, x)
    total = int(sum(cell.Ns))
    sw = blk_segw_bits10(blk_bits10(int(offs[-1]), total))
    lanes, cap = nt_for_len(cell.L, cell.k), blk_lane_cap(sw)
    bits, wave = code_lengths(x, cell)
    # the code-length rule above against the oracle's headers: the first code of a waveform takes k + 1 to 25 bits
    inner = np.bincount(wave, weights=bits, minlength=n_i.size).astype(np.int64)
    assert ((inner + cell.k + 1 <= 32 * n_i.astype(np.int64)) & (inner + 25 > 32 * (n_i.astype(np.int64) - 1))).all(), cell
    # A code belongs to the lane in whose sw words it starts, and a waveform of n_i words has ceil(n_i / sw) lanes: some lane
    # holds at least samples / lanes codes.  A zero stretch of S samples costs k + 1 bits a sample and touches at most
    # ceil(S (k + 1) / (32 sw)) + 1 lanes: some lane of those holds at least S over that many.
    n_lanes = int((-(-n_i.astype(np.int64) // sw)).sum())
    most = total / n_lanes
    if cell.kind == "stretch":
        S = 2 * cell.L // 3 - cell.L // 3
        most = max(most, S / (-(-S * (cell.k + 1) // (32 * sw)) + 1))
    return dict(k=cell.k, L=cell.L, kind=cell.kind, lanes=lanes, sw=sw, cap=cap, bits=32.0 * int(offs[-1]) / total, B=lanes * sw,
                n_i=n_i, passes=most > cap, most=most, lengths=np.unique(bits).size)


# --------------------------------------------------------------------------- the table
# matched data at every k where the 64- and 128-lane blocks are (L = 3000) and where the 256-lane blocks are (L = 20 000), and
# at the k that move the class at 6000
_TABLE = [(k, 3000, "matched") for k in range(16)]
_TABLE += [(k, 6000, "matched") for k in (0, 1, 4, 7, 9, 12)] + [(k, 20000, "matched") for k in range(16)]
# a RiceParameter that does not suit the data: short codes under a large k, one bit per sample, escapes throughout
_TABLE += [(4, 3000, "quiet"), (12, 3000, "quiet"), (2, 6000, "quiet"), (0, 20000, "quiet"), (8, 20000, "quiet")]
_TABLE += [(0, 3000, "zeros"), (15, 3000, "zeros"), (0, 6000, "zeros"), (1, 6000, "zeros"), (0, 20000, "zeros"), (3, 20000, "zeros")]
_TABLE += [(0, 3000, "uniform"), (13, 3000, "uniform"), (2, 6000, "uniform"), (1, 20000, "uniform"), (5, 20000, "uniform")]
_TABLE += [(2, 3000, "steps"), (3, 6000, "steps"), (1, 20000, "steps"), (4, 20000, "steps")]
# (a zero costs k + 1 bits: at k <= 2 the lanes inside the stretch hold more codes than their share, and a block's staging passes
# begin and end inside a waveform of noise; at a larger k the stretch is a change of code length and no more, as measure() says)
_TABLE += [(1, 3000, "stretch"), (2, 6000, "stretch"), (2, 20000, "stretch"), (5, 3000, "stretch"), (10, 3000, "stretch"),
           (6, 6000, "stretch"), (11, 6000, "stretch"), (8, 20000, "stretch")]
CELLS = [Cell(*c) for c in _TABLE]
assert len({c.id for c in CELLS}) == len(CELLS)


# --------------------------------------------------------------------------- where a payload ends in its last block
# (the last two: the cells of 64 and of 128 lanes whose waveforms are longer than a block, so that every residue is met there too)
RESIDUE_CELLS = [(3, 20000, "matched"), (0, 6000, "matched"), (11, 3000, "matched"), (3, 20000, "zeros"), (6, 3000, "matched"),
                 (9, 6000, "matched")]


def residues(B):
    """n mod B of the last waveform's payload words n: the block's border, the words behind it that a block keeps in front
    (kBlkPre = 8) and behind (kBlkTail = 4) of its own, and one word short of the border."""
    return (0, 1, 3, 4, 5, 8, 9, B - 1)


@functools.lru_cache(maxsize=None)
def residue_cells(O, k, L, kind):
    """{residue: Cell or None} -- for every residue r of the cell's block size a length of the chunks' last waveform at which
    the payload of chunk 0's last waveform has n words with n mod B == r, or None where no length from 1 to L gives one.
    n(l) grows by at most one word per sample (a code has at most 25 bits), so every n up to n(L) is met, and bisection finds
    it; the largest such n is taken.  B is that of the table's cell; residue_of() takes it again from the stream that results
    (the last length moves the stream's bits per sample a little), and the model test asserts that it did not move."""
    base = Cell(k, L, kind)
    full = Cell(k, L, kind, last=L).x()

    def n_of(l):  # payload words of chunk 0's last waveform at length l: the header of a chunk that holds it alone
        return int(O.encode_chunk(full[2 * L:2 * L + l], (base.m, L))[1])

    found = {}
    B, top = measure(O, base)["B"], n_of(L)
    for r in residues(B):
        name = "B-1" if r == B - 1 else r
        found[name] = None
        n = top - (top - r) % B if top >= r else 0
        if n < 1:
            continue
        lo, hi = 1, L  # the smallest l with n_of(l) >= n
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (mid + 1, hi) if n_of(mid) < n else (lo, mid)
        found[name] = Cell(k, L, kind, last=lo)
    return found


def residue_of(O, cell):
    """(n mod B, B, (lanes, sw)) of chunk 0's last waveform in the cell's own stream"""
    got = measure(O, cell)
    return int(got["n_i"][2]) % got["B"], got["B"], (got["lanes"], got["sw"])
