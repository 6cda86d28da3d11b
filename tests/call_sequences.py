"""Sequences of calls on plans and contexts, and what the oracle says each call must give (a helper module of the tests, not a
conftest; no GPU is needed to import or run it).

A drx_plan carries state from one call to the next -- the look-back / granule / estimate scratch, the n_i and offset tables,
the status word, the code length the last encode measured, the gather's resume key, the selection scratch -- and a drx_ctx
carries the side stream, the cached one-chunk plan and its staging buffers.  tests/test_gpu_call_sequences.py drives the
schedules made here through the library; tests/test_call_sequences_model.py holds the schedules and their expectations to
the oracle alone.

A schedule is a list of Step.  A step names an operation, the plan it runs on, the arguments drawn for it and, for every
buffer the call writes, a KEY of the expected content; resolve(key) turns a key into arrays, all of them from oracle.oracle
(the 16 sizes of drx_estimate_words: from tests/filter_reference.py) and cached per (geometry, filter, dataset).

Geometries (most below 1 M samples; `iir` has 3.1 M, the fewest that reach its route; every one but the whole-chunk batch,
whose chunks are one waveform each by definition, has a shorter last waveform in a chunk):
  short   3 chunks of 1000 waveforms of 100 samples: every encoder by flag (the persistent ones through FORCE_STREAM and
          FORCE_STREAM_SEGS), the block-parallel walk, the walk inside the lanes launch, the LDS walk.  RiceParameter 2: zeros take 2
          bits a sample and full-range samples 25, so consecutive encodes differ 12-fold in code length.
  mid     4 chunks of 36 waveforms of 7000: the chunk-wide walk, the block decoder, k_encode_fused / k_encode_stream; RiceParameter 2
          again: a waveform of zeros is 438 words, a full-range one 5469, more than a ring of the persistent encoder (2496).
  long    2 chunks of 10 waveforms of 24 000: pieces and segment encoders, block and long decoders.
  ragged  six chunks, WaveformLengths 512, 2048, 7000, 16384, whole-chunk and 3333, with 81 and 73 waveforms in the two
          short-waveform chunks (bw_walk_pays() wants 35 a walked chunk): both parallel walks, forked, and a lanes launch behind each.
  whole   3 chunks of one waveform of 65 537 samples (WaveformLength -1): still a batch the long decoder takes.
  iir     2 chunks of 768 waveforms of 2048 samples.  The block decoder takes a batch of waveforms of at least 2048 samples
          (blocks_batch()), a four-tap filter inside it only where a launch has as many waveforms as resident workgroups
          (launch_decode_blocks(): 256 x 6 = 1536 at 128 lanes a block, which is what general filters run at for this length):
          1536 x 2048 is the smallest batch that reaches DRX_PATH_IIR_FUSED, and DRX_DBG_IIR_SEPARATE gives DRX_PATH_IIR on it.
"""
import functools
import zlib
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import numpy as np

import filter_reference as F
from deltarice_amd import _lib as D
from oracle import oracle as O

FILTERS = {
    "delta": None,
    "fir4": (1, -1, 1, -1),
    "fir3": (-1, 2, -1),
    "fir5": (1, -1, 1, -1, 1),
    "lead2": F.FILTERS["lead_m2"],  # (-2, 1): lossy on decode, the expected samples are the oracle's decode
    "taps64": F.FILTERS[next(n for n in F.FILTERS if n.startswith("t64_lead1_"))],
}
DATASETS = ("zeros", "gauss10", "gauss400", "uniform")


class Geometry(NamedTuple):
    Ns: tuple
    Ls: tuple            # 0: the whole chunk
    m: int
    filters: tuple       # what set_filter draws from on this geometry (the first: what a new plan gets)


GEOMETRIES = {
    "short": Geometry((100 * 1000 + 37,) * 3, (100,) * 3, 2, ("delta", "fir4", "fir3", "fir5", "lead2", "taps64")),
    "mid": Geometry((7000 * 36 - 3000,) * 4, (7000,) * 4, 2, ("delta", "fir4", "fir5")),
    "long": Geometry((24000 * 10 - 7777,) * 2, (24000,) * 2, 8, ("delta", "fir3", "lead2")),
    "ragged": Geometry((512 * 80 + 100, 2048 * 72 + 17, 7000 * 30, 16384 * 4, 4321, 3333 * 21 + 1), (512, 2048, 7000, 16384, 0, 3333), 8,
                       ("delta", "fir4", "lead2")),
    "whole": Geometry((65537,) * 3, (0,) * 3, 8, ("delta", "fir3")),
    "iir": Geometry((768 * 2048 - 1000,) * 2, (2048,) * 2, 8, ("fir4", "delta")),
}

# (encode_impl, decode_impl, debug_flags): the values tests/test_gpu_routes.py and tests/test_gpu_parity.py use
FLAGS = (0, D.DBG_NO_LONG_PATHS, D.DBG_LONG_NOT_BLOCKS, D.DBG_NO_PARALLEL_WALKS, D.DBG_NO_PIECES, D.DBG_FORCE_SEGMENTS,
         D.DBG_FORCE_PIECES, D.DBG_NO_WIDE_FUSED, D.DBG_RAGGED_ONE_LANES_LAUNCH, D.DBG_FORCE_STREAM, D.DBG_IIR_SEPARATE,
         D.DBG_FORCE_STREAM_SEGS, D.DBG_WALK_BY_SCAN, D.DBG_WALK_BY_CHAINS,
         D.DBG_NO_LONG_PATHS | D.DBG_FORCE_STREAM, D.DBG_NO_LONG_PATHS | D.DBG_FORCE_STREAM_SEGS,
         D.DBG_NO_LONG_PATHS | D.DBG_NO_PIECES | D.DBG_FORCE_STREAM, D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_CHAINS,
         D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_SCAN)
DEFAULT_CFG = (2, 8, 0)

OPS = ("encode", "encode_small", "decode", "decode_sideband", "decode_corrupt", "select", "gather", "gather_size_only",
       "gather_after_sizing", "gather_after_sizing_other_list", "gather_small", "estimate", "set_filter", "set_flags",
       "read_wave_words", "host_filter")
ERROR_OPS = ("encode_small", "decode_corrupt", "gather_small")
SEL_SIZES = (1, 3, 64, 5000)
SEL_SAMPLES = 4_000_000   # a selection's rows, samples (fewer entries of long waveforms)
GATHER_SAMPLES = 400_000  # a gathered batch, samples

# the one-chunk host path: (samples, WaveformLength (0: whole chunk), RiceParameter, filter); no two alike in all of geometry, k, taps
HOST_CASES = ((20 * 700, 700, 8, "delta"), (64 * 300 + 5, 64, 4, "fir4"), (3 * 16384 + 99, 16384, 16, "delta"), (150001, 0, 8, "delta"),
              (9 * 1000, 1000, 4, "fir5"), (600 * 512 + 7, 512, 8, "delta"), (40 * 7000, 7000, 32, "lead2"), (20 * 700, 700, 8, "fir3"),
              (20 * 700, 700, 2, "delta"))


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def make_data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, np.int16)
    if kind == "uniform":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.normal(0, {"gauss10": 10, "gauss400": 400}[kind], n).astype(np.int16)


def opts_of(m, L, taps):
    """compression_opts of one chunk (WaveformLength -1 where a filter follows a whole-chunk waveform)."""
    if taps is None:
        return (m, L) if L else (m,)
    return (m, L if L else -1, len(taps)) + tuple(int(t) & 0xFFFFFFFF for t in taps)


def waves(Ns, Ls):
    """-> (first sample, length, chunk) of every waveform of a batch."""
    start, length, chunk, at = [], [], [], 0
    for c, (N, L) in enumerate(zip(Ns, Ls)):
        L = L if L else N
        s = np.arange(0, N, L, dtype=np.int64)
        start.append(at + s)
        length.append(np.minimum(L, N - s))
        chunk.append(np.full(s.size, c, np.int64))
        at += N
    return np.concatenate(start), np.concatenate(length), np.concatenate(chunk)


def walk_chunk(w, n_samples, L):
    """The oracle's header walk of one encoded chunk (src/deltaRice.c:320-325 as oracle/deltarice_oracle.c states it): n_i of
    every waveform, or None where the chunk is not n_samples samples whose chain of n_i ends at the chunk's end."""
    if w.size < 2 or int(w[0]) != n_samples:
        return None
    L = L if L else n_samples
    at, out = 1, []
    for _ in range(-(-n_samples // L)):
        if at >= w.size:
            return None
        n = int(w[at])
        out.append(n)
        at += n + 1
    return np.array(out, np.uint32) if at == w.size else None


class Expect:
    """What the oracle gives for one (geometry, filter, dataset); everything computed once, on first use."""

    def __init__(self, Ns, Ls, m, taps, ds, seed):
        self.Ns, self.Ls, self.m, self.taps, self.ds = tuple(Ns), tuple(Ls), m, taps, ds
        self.x = make_data(ds, sum(Ns), seed)
        self.start, self.length, self.chunk = waves(Ns, Ls)
        self.at = np.concatenate([[0], np.cumsum(Ns)])
        self.wave_base = np.concatenate([[0], np.cumsum([-(-N // (L if L else N)) for N, L in zip(Ns, Ls)])])

    def chunk_x(self, c):
        return self.x[self.at[c]:self.at[c + 1]]

    @functools.cached_property
    def chunk_words(self):
        return [O.encode_chunk(self.chunk_x(c), opts_of(self.m, L, self.taps)) for c, L in enumerate(self.Ls)]

    @functools.cached_property
    def words(self):
        return np.concatenate(self.chunk_words)

    @functools.cached_property
    def off(self):
        return np.concatenate([[0], np.cumsum([w.size for w in self.chunk_words])]).astype(np.int64)

    @functools.cached_property
    def table(self):
        t = [walk_chunk(w, N, L) for w, N, L in zip(self.chunk_words, self.Ns, self.Ls)]
        assert all(v is not None for v in t), "the oracle's own stream fails its header walk"
        return np.concatenate(t)

    @functools.cached_property
    def decoded(self):
        if self.taps is None or abs(self.taps[0]) == 1:
            return self.x
        return np.concatenate([O.decode_chunk(w, opts_of(self.m, L, self.taps)) for w, L in zip(self.chunk_words, self.Ls)])

    @functools.cached_property
    def estimate(self):
        """(16 sizes, k = 0 is defined) as tests/test_gpu_filter_domain.py::test_estimate_words takes them from the helper
        module: F.chunk_residuals, and F.words' rule -- F.code_bits summed over a waveform, rounded up to words -- for all the
        waveforms of a chunk at once and in 32-bit integers (16 passes over up to 3 M residuals: F.code_bits' int64 arrays take
        four times as long; tests/test_call_sequences_model.py holds waveforms of every chunk to F.words itself)."""
        taps = self.taps if self.taps is not None else (1, -1)
        sizes, zmax = [0] * 16, 0
        for c, (N, L) in enumerate(zip(self.Ns, self.Ls)):
            d = F.chunk_residuals(self.chunk_x(c), L, taps).astype(np.int32)
            first = np.arange(0, N, L if L else N)
            z = np.where(d < 0, -2 * d - 1, 2 * d)              # src/deltaRice.c:208-211
            zmax = max(zmax, int(z.max()))
            for k in range(16):
                q = z >> k                                      # :212
                bits = np.where(q < 8, q + (1 + k), 25)         # :215-228
                n_i = (np.add.reduceat(bits, first, dtype=np.int64) + 31) // 32
                sizes[k] += 1 + int((n_i + 1).sum())
        return sizes, zmax < 32768

    @functools.lru_cache(maxsize=None)
    def gather(self, idx, cw):
        """(words, offsets, n_i) of the batch made of the waveforms idx, cw to a chunk: encode_chunk of the concatenated
        waveforms under each output chunk's first length, as tests/fuzz_parity.py builds `want`."""
        out, tab = [], []
        for c0 in range(0, len(idx), cw):
            part = idx[c0:c0 + cw]
            Lg = int(self.length[part[0]])
            xs = np.concatenate([self.x[self.start[g]:self.start[g] + self.length[g]] for g in part])
            w = O.encode_chunk(xs, opts_of(self.m, Lg, self.taps))
            out.append(w)
            tab.append(walk_chunk(w, xs.size, Lg))
        return (np.concatenate(out), np.concatenate([[0], np.cumsum([w.size for w in out])]).astype(np.int64), np.concatenate(tab))

    def corrupt(self, kind, c, i):
        """The stream with ONE header changed: n_i of waveform i of chunk c plus one, or chunk c's sample count plus one."""
        w = self.words.copy()
        o = int(self.off[c])
        if kind == "total":
            w[o] += 1
        else:
            w[o + 1 + int((self.table[self.wave_base[c]:self.wave_base[c] + i].astype(np.int64) + 1).sum())] += 1
        return w


@functools.lru_cache(maxsize=None)
def expect(geom, filt, ds):
    G = GEOMETRIES[geom]
    return Expect(G.Ns, G.Ls, G.m, FILTERS[filt], ds, _seed(geom, ds))


@functools.lru_cache(maxsize=None)
def host_expect(case, ds):
    N, L, m, filt = HOST_CASES[case]
    return Expect((N,), (L,), m, FILTERS[filt], ds, _seed("host", case, ds))


def host_opts(case):
    N, L, m, filt = HOST_CASES[case]
    return opts_of(m, L, FILTERS[filt])


# ---------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Step:
    op: str
    plan: int = -1               # index into the schedule's plans (-1: a call on the context)
    geom: str = ""
    filt: str = ""               # the plan's filter when the call is made
    cfg: tuple = DEFAULT_CFG     # the context's (encode_impl, decode_impl, debug_flags) when the call is made
    ds: Optional[str] = None     # the dataset the call works on
    args: dict = field(default_factory=dict)
    status: int = 0              # what drx_plan_finish must report for this call
    total: Optional[int] = None  # ... and the word count it must report (encodes, gathers)
    finish: bool = True          # finish and check behind the call (False: a chain's last step does it)
    # buffers the call writes: name -> (check, key); check "exact": the payload is resolve(key) and the guards are intact,
    # "guards": the guards are intact (the payload is undefined), "intact": not one word of the buffer was written
    out: dict = field(default_factory=dict)
    host: Optional[tuple] = None  # key of what the call returns to the host (estimate, read_wave_words, host_filter)

    def label(self):
        a = {k: (v if not isinstance(v, tuple) or len(v) < 8 else f"<{len(v)} entries>") for k, v in self.args.items()}
        return f"{self.op} on plan {self.plan} ({self.geom}, {self.filt}, cfg {self.cfg}), dataset {self.ds}, {a}"


def resolve(key):
    """The arrays behind a key of Step.out / Step.host / a step's inputs."""
    kind = key[0]
    if kind == "host":
        _, case, ds, reverse = key
        e = host_expect(case, ds)
        return e.decoded if reverse else e.words
    if kind == "estimate":
        return expect(*key[1:]).estimate
    e = expect(*key[1:4])
    if kind in ("x", "words", "off", "decoded"):
        return getattr(e, kind)
    if kind == "table":
        return e.table.view(np.int32)
    if kind == "corrupt":
        return e.corrupt(*key[4:])
    if kind == "rows":      # (first sample, length) of every row, into "decoded"
        idx = np.array(key[4], np.int64)
        return e.start[idx], e.length[idx]
    if kind == "masked_table":  # (n_i table, mask of the entries that are defined): the chunks the list touches
        mask = np.ones(e.table.size, bool) if key[4] is None else np.isin(e.chunk, np.unique(e.chunk[np.array(key[4], np.int64)]))
        return e.table, mask
    if kind == "gdecoded":  # what the gathered batch decodes to: the entries' decoded samples, in list order
        return np.concatenate([e.decoded[e.start[g]:e.start[g] + e.length[g]] for g in key[4]])
    w, off, tab = e.gather(key[4], key[5])
    return {"gwords": w, "goff": off, "gtable": tab.view(np.int32)}[kind]


class Model:
    """The state the schedules' steps depend on, and one method per operation that draws a step's arguments and states what
    the call must give.  Deterministic from the seed."""

    def __init__(self, geoms, seed):
        self.rng = np.random.default_rng(_seed("model", seed, *geoms))
        self.geoms = list(geoms)
        self.filt = [GEOMETRIES[g].filters[0] for g in geoms]
        self.cfg = DEFAULT_CFG
        self.last_ds = [None] * len(geoms)      # the dataset of the plan's last call that took one
        self.tables = [None] * len(geoms)       # (dataset, filter, list or None): what the plan's n_i table holds, or None
        self.host_prev = None
        self.steps = []

    # -- drawing --
    def other_ds(self, p, ds=None):
        if ds is None:
            ds = str(self.rng.choice([d for d in DATASETS if d != self.last_ds[p]]))
        self.last_ds[p] = ds
        return ds

    def sel_list(self, p, size=None):
        e = expect(self.geoms[p], "delta", "zeros")
        size = int(self.rng.choice(SEL_SIZES)) if size is None else size
        size = min(size, max(1, SEL_SAMPLES // int(e.length.max())))
        idx = self.rng.integers(0, e.start.size, size)
        if size >= 3:
            idx[size // 2] = idx[0]  # (a duplicate)
        return tuple(int(v) for v in idx)

    def gather_list(self, p, size=None, avoid=None):
        """A list under the one-length-per-output-chunk rule: waveforms of one length, any chunking; now and then a shorter
        last waveform of a chunk as the list's last entry."""
        e = expect(self.geoms[p], "delta", "zeros")
        while True:
            Lg = int(e.length[self.rng.integers(0, e.start.size)])
            same = np.nonzero(e.length == Lg)[0]
            n = int(self.rng.choice(SEL_SIZES)) if size is None else size
            n = min(n, max(1, GATHER_SAMPLES // Lg))
            idx = self.rng.choice(same, n)
            shorter = np.nonzero(e.length < Lg)[0]
            if shorter.size and n > 1 and size is None and self.rng.random() < 0.5:
                idx[-1] = self.rng.choice(shorter)
            cw = int(self.rng.integers(1, n + 1))
            idx = tuple(int(v) for v in idx)
            if idx != avoid:
                return idx, cw

    def add(self, op, p=-1, finish=True, **kw):
        s = Step(op, p, self.geoms[p] if p >= 0 else "", self.filt[p] if p >= 0 else "", self.cfg, finish=finish, **kw)
        self.steps.append(s)
        return s

    def key(self, kind, p, ds, *more):
        return (kind, self.geoms[p], self.filt[p], ds) + more

    # -- the operations --
    def encode(self, p, ds=None, finish=True, small=False):
        ds = self.other_ds(p, ds)
        e = expect(self.geoms[p], self.filt[p], ds)
        self.tables[p] = None if small else (ds, self.filt[p], None)
        if small:  # capacity = needed - 5: status 3, the total still the oracle's, nothing behind the capacity
            return self.add("encode_small", p, finish, ds=ds, status=3, total=int(e.words.size), args={"cap": int(e.words.size) - 5},
                            out={"words": ("guards", None), "off": ("guards", None)})
        return self.add("encode", p, finish, ds=ds, total=int(e.words.size),
                        out={"words": ("exact", self.key("words", p, ds)), "off": ("exact", self.key("off", p, ds))})

    def encode_small(self, p, ds=None, finish=True):
        return self.encode(p, ds, finish, small=True)

    def decode(self, p, ds=None, finish=True, sideband=False, src=None):
        ds = self.other_ds(p, ds)
        self.tables[p] = (ds, self.filt[p], None)
        return self.add("decode_sideband" if sideband else "decode", p, finish, ds=ds, args={"src": src},
                        out={"samples": ("exact", self.key("decoded", p, ds))})

    def decode_sideband(self, p, ds=None, finish=True):
        return self.decode(p, ds, finish, sideband=True)

    def decode_corrupt(self, p, ds=None, finish=True):
        ds = self.other_ds(p, ds)
        e = expect(self.geoms[p], self.filt[p], ds)
        c = int(self.rng.integers(0, len(e.Ns)))
        i = int(self.rng.integers(0, e.wave_base[c + 1] - e.wave_base[c]))
        kind = "total" if self.rng.random() < 0.4 else "n_plus"
        self.tables[p] = None
        return self.add("decode_corrupt", p, finish, ds=ds, status=4, args={"kind": kind, "chunk": c, "wave": i},
                        out={"samples": ("guards", None)})

    def select(self, p, ds=None, finish=True, size=None, sideband=None, src=None):
        ds = self.other_ds(p, ds)
        idx = self.sel_list(p, size)
        sideband = bool(self.rng.integers(0, 2)) if sideband is None else sideband
        self.tables[p] = (ds, self.filt[p], idx)
        return self.add("select", p, finish, ds=ds, args={"idx": idx, "sideband": sideband, "src": src},
                        out={"rows": ("exact", self.key("rows", p, ds, idx))})

    def _gather(self, op, p, ds, finish, idx, cw, sideband, src=None, **args):
        e = expect(self.geoms[p], self.filt[p], ds)
        w, _, _ = e.gather(idx, cw)
        self.tables[p] = (ds, self.filt[p], idx)
        out = {"goff": ("exact", self.key("goff", p, ds, idx, cw)), "gtable": ("exact", self.key("gtable", p, ds, idx, cw))}
        status = 0
        if op == "gather_small":  # not one word written
            out, status = {"gwords": ("intact", None), "goff": ("guards", None), "gtable": ("guards", None)}, 3
            args["cap"] = max(1, int(w.size) - 5)
            self.tables[p] = None
        elif op != "gather_size_only":
            out["gwords"] = ("exact", self.key("gwords", p, ds, idx, cw))
        return self.add(op, p, finish, ds=ds, status=status, total=int(w.size),
                        args=dict(idx=idx, cw=cw, sideband=sideband, src=src, **args), out=out)

    def gather(self, p, ds=None, finish=True, size=None, sideband=None, src=None, op="gather", same_as=None):
        """same_as: an earlier gather step of the plan whose stream, list, chunking and side-band this one repeats."""
        if same_as is not None:
            a = same_as.args
            return self._gather(op, p, self.other_ds(p, same_as.ds), finish, a["idx"], a["cw"], a["sideband"], a["src"])
        ds = self.other_ds(p, ds)
        idx, cw = self.gather_list(p, size)
        sideband = bool(self.rng.integers(0, 2)) if sideband is None else sideband
        return self._gather(op, p, ds, finish, idx, cw, sideband, src)

    def gather_decode(self, p, src, finish=True):
        """The batch of the gather step `src` (an index into the schedule), made again by Plan.gather_encoded and decoded
        through the Gathered's plan(): the result's geometry, the source plan's RiceParameter and the filter Plan.set_filter set."""
        g = self.steps[src]
        return self.add("gather_decode", p, finish, ds=g.ds, args={"src": None, "of": src, "idx": g.args["idx"], "cw": g.args["cw"]},
                        out={"samples": ("exact", self.key("gdecoded", p, g.ds, g.args["idx"])),
                             "gwords": ("exact", self.key("gwords", p, g.ds, g.args["idx"], g.args["cw"]))})

    def gather_size_only(self, p, ds=None, finish=True, **kw):
        return self.gather(p, ds, finish, op="gather_size_only", **kw)

    def gather_after_sizing(self, p, ds=None, finish=True):
        """A sizing call, then the call with the same arguments: the resume path."""
        return self.gather(p, ds, finish, op="gather_after_sizing")

    def gather_after_sizing_other_list(self, p, ds=None, finish=True):
        """A sizing call with one list, then the call with another of the same length and chunking: it must not resume."""
        ds = self.other_ds(p, ds)
        e = expect(self.geoms[p], "delta", "zeros")
        while True:  # (a length that more than one waveform has: there is another list)
            first, cw = self.gather_list(p, int(self.rng.choice((3, 64))))
            same = np.nonzero(e.length == e.length[first[0]])[0]
            if same.size > 1 and len(first) > 1:
                break
        while True:
            idx = tuple(int(v) for v in self.rng.choice(same, len(first)))
            if idx != first:
                break
        return self._gather("gather_after_sizing_other_list", p, ds, finish, idx, cw, bool(self.rng.integers(0, 2)), sized=first)

    def gather_small(self, p, ds=None, finish=True):
        return self.gather(p, ds, finish, op="gather_small")

    def estimate(self, p, ds=None):
        ds = self.other_ds(p, ds)
        return self.add("estimate", p, ds=ds, host=("estimate", self.geoms[p], self.filt[p], ds))

    def set_filter(self, p, name=None):
        names = GEOMETRIES[self.geoms[p]].filters
        if name is None:
            name = names[(names.index(self.filt[p]) + 1) % len(names)]
        s = self.add("set_filter", p, args={"name": name})
        self.filt[p] = name
        return s

    def set_flags(self, p=-1, cfg=None):
        if cfg is None:
            cfg = (int(self.rng.integers(0, 3)), int(self.rng.choice((8, 8, 7, 0))), int(FLAGS[self.rng.integers(0, len(FLAGS))]))
        self.cfg = tuple(cfg)
        return self.add("set_flags", -1, args={"cfg": self.cfg})

    def read_wave_words(self, p):
        """The n_i table of the plan's last call: of every waveform behind an encode or a decode, of the touched chunks behind a
        selection or a gather; behind an error, a plan's first call included, the call must succeed and its content is open."""
        t = self.tables[p]
        key = ("masked_table", self.geoms[p], t[1], t[0], t[2]) if t else None
        return self.add("read_wave_words", p, host=key, args={"defined": t is not None})

    def host_filter(self, p=-1, corrupt=None):
        """One chunk through ctx.filter_chunk, never the geometry, k and taps of the last such step; corrupt: a stream with one
        header changed first (status 4), then the good one."""
        case = int(self.rng.choice([c for c in range(len(HOST_CASES)) if c != self.host_prev]))
        self.host_prev = case
        ds = str(self.rng.choice(DATASETS))
        N, L, m, filt = HOST_CASES[case]
        reverse = bool(self.rng.integers(0, 2))
        corrupt = (self.rng.random() < 0.25) if corrupt is None else corrupt
        args = {"case": case, "reverse": reverse}
        if corrupt:
            args["reverse"] = reverse = True
            W = -(-N // (L if L else N))
            args["corrupt"] = ("total", 0, 0) if (L and N % L == 0 and self.rng.random() < 0.5) else ("n_plus", 0, int(self.rng.integers(0, W)))
        return self.add("host_filter", -1, ds=ds, args=args, host=("host", case, ds, reverse))

    def do(self, op, p, **kw):
        return getattr(self, op)(p, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------------------------------------------------

def pairs(geom):
    """Every ordered pair (A, B) of operations on ONE plan of the geometry, one pair after the other: B works on another
    dataset than A wherever both take one (Model.other_ds).  -> (plans' geometries, steps, [(index of A, index of B)])."""
    M = Model([geom], "pairs")
    where = []
    for a in OPS:
        for b in OPS:
            M.do(a, 0)
            M.do(b, 0)
            where.append((len(M.steps) - 2, len(M.steps) - 1))
    return M.geoms, M.steps, where


SESSION_GEOMS = {0: ("short", "ragged", "long"), 1: ("mid", "whole", "short")}


def session(seed, n_steps=300):
    """A random walk over three plans of different geometry on one context, interleaved.  Every "error, then a good call of
    every other kind on the same plan" transition occurs: those pairs and eight more of every operation are dealt like a deck,
    a step on another plan now and then between the two of a pair; random operations fill the rest."""
    geoms = SESSION_GEOMS.get(seed, tuple(sorted(GEOMETRIES)[(seed + i) % len(GEOMETRIES)] for i in range(3)))
    M = Model(geoms, ("session", seed))
    good = [o for o in OPS if o not in ERROR_OPS]
    deck = [(e, g) for e in ERROR_OPS for g in good] + [(o,) for o in OPS if o not in ERROR_OPS for _ in range(8)]
    deck = [deck[i] for i in M.rng.permutation(len(deck))]
    while len(M.steps) < n_steps:
        block = deck.pop() if deck else (str(M.rng.choice(OPS)),)
        p = int(M.rng.integers(0, 3))
        M.do(block[0], p)
        if len(block) == 2:
            if M.rng.random() < 0.5:  # (another plan's call in between: the transition is the plan's, not the context's)
                M.do(str(M.rng.choice([o for o in good if o not in ("set_flags", "host_filter")])), (p + 1 + int(M.rng.integers(0, 2))) % 3)
            M.do(block[1], p)
    return M.geoms, M.steps


def async_chains():
    """Chains of 4 to 8 calls with no finish between them, every result in a buffer of its own; then one finish per plan
    (op "finish": the status and the total of the plan's LAST call), and every buffer of the chain is checked.
    args["src"]: the chain's step whose output the call reads (None: the oracle's stream).  -> [(name, geometries, steps)]."""
    chains = []

    def chain(name, geoms, build):
        M = Model(geoms, ("chain", name))
        build(M)
        last = {}
        for s in M.steps:
            if s.plan >= 0 and s.op not in ("set_filter", "estimate", "read_wave_words"):
                last[s.plan] = s
        for p, s in sorted(last.items()):
            M.add("finish", p, status=s.status, total=s.total)
        assert 4 <= sum(s.plan >= 0 and s.op != "finish" for s in M.steps) <= 8, name
        chains.append((name, M.geoms, M.steps))

    def pipeline(M, a, b):  # (every call reads what an earlier call of the chain wrote)
        M.encode(a, "gauss10", finish=False)
        M.decode(b, "gauss10", finish=False, src=0)
        M.encode(a, "uniform", finish=False)
        M.select(b, "uniform", finish=False, size=64, sideband=False, src=2)
        M.gather(a, "uniform", finish=False, size=64, sideband=False, src=2)
    chain("encode-decode-encode-select-gather", ["mid"], lambda M: pipeline(M, 0, 0))
    # ... the same chain, its calls alternating between two plans of one geometry: one plan's output is the other's input
    chain("the same chain alternating between two plans", ["mid", "mid"], lambda M: pipeline(M, 0, 1))

    def alternating(M):
        M.encode(0, "gauss10", finish=False)
        M.encode(1, "uniform", finish=False)
        M.decode(0, "gauss10", finish=False, src=0)
        M.decode(1, "uniform", finish=False, src=1)
        M.encode(0, "zeros", finish=False)
        M.select(1, "uniform", finish=False, size=64, sideband=False, src=1)
        M.select(0, "zeros", finish=False, size=64, sideband=True, src=4)
        M.gather(1, "uniform", finish=False, size=64, sideband=False, src=1)
    chain("two pipelines interleaved on two plans", ["short", "mid"], alternating)

    def regrow(M):
        M.select(0, "gauss10", finish=False, size=5000, sideband=False)
        M.select(0, "gauss400", finish=False, size=3, sideband=False)
        M.select(0, "zeros", finish=False, size=6000, sideband=True)
        M.gather(0, "uniform", finish=False, size=5000, sideband=False)
    chain("selection scratch regrows with a call in flight", ["short"], regrow)

    def two_ragged(M):
        M.decode(0, "gauss10", finish=False)
        M.decode(1, "gauss400", finish=False)
        M.decode(0, "uniform", finish=False)
        M.decode(1, "zeros", finish=False)
    chain("ragged decodes back to back on two plans", ["ragged", "ragged"], two_ragged)

    # (a device-side error of a call that was never finished is not kept, include/deltarice_hip.h: the finish reports the
    # chain's last call -- which must not inherit the error either)
    def lost_capacity(M):
        M.encode(0, "gauss10", finish=False)
        M.decode(0, "gauss10", finish=False, src=0)
        M.encode_small(0, "uniform", finish=False)
        M.encode(0, "zeros", finish=False)
    chain("a capacity error, then an encode, no finish between", ["short"], lost_capacity)

    def lost_corrupt(M):
        M.encode(0, "gauss10", finish=False)
        M.decode_corrupt(0, "gauss10", finish=False)
        M.decode(0, "gauss400", finish=False)
        M.decode_sideband(0, "zeros", finish=False)
    chain("a damaged stream, then decodes, no finish between", ["mid"], lost_corrupt)

    def scan_users(M):  # (d_scan: the encoders' look-back, the fused lane decoder's granules, the estimate's sums)
        M.set_flags(cfg=(2, 8, D.DBG_NO_PARALLEL_WALKS | D.DBG_FORCE_STREAM))
        M.encode(0, "uniform", finish=False)
        M.decode(0, "gauss10", finish=False)
        M.estimate(0, "gauss400")
        M.encode(0, "zeros", finish=False)
        M.set_flags(cfg=(2, 8, D.DBG_NO_PARALLEL_WALKS | D.DBG_FORCE_STREAM_SEGS))
        M.encode(0, "gauss400", finish=False)
        M.decode(0, "gauss400", finish=False, src=len(M.steps) - 1)
        M.set_flags(cfg=DEFAULT_CFG)
    chain("the three users of the look-back scratch", ["short"], scan_users)

    def sizing(M):
        M.gather_after_sizing(0, "gauss10", finish=False)
        M.gather_size_only(0, "uniform", finish=False)
        M.gather(0, "gauss400", finish=False)
        M.gather_after_sizing_other_list(0, "zeros", finish=False)
        M.decode_sideband(0, "uniform", finish=False)
    chain("sizing calls and what follows them", ["long"], sizing)

    # A sizing call, then a call that rewrites the plan's tables from OTHER data, then the gather with the sizing call's very
    # arguments (the uploaded stream is one tensor: the pointers match too): it must not resume from tables that are no longer
    # the sizing call's.  drx_plan_set_filter ends a resume as well, but rewrites no table: no result can show that.
    def stale_resume(M, between):
        for op in between:
            sized = M.gather_size_only(0, finish=False, size=64)
            M.do(op, 0, finish=False)
            M.gather(0, finish=False, same_as=sized)
    chain("a sizing call, an encode or a decode, then the same gather", ["mid"], lambda M: stale_resume(M, ("encode", "decode")))
    chain("a sizing call, a side-band decode or a selection, then the same gather", ["ragged"], lambda M: stale_resume(M, ("decode_sideband", "select")))
    return chains


# (encode_impl, debug_flags) under which the `short` geometry takes each encoder DRX_ENC_* 1 ... 6 (route_encode(), drx_api_encode.hip)
TOUR_ENCODERS = {1: (0, 0), 2: (2, D.DBG_NO_PIECES), 3: (1, D.DBG_NO_LONG_PATHS | D.DBG_NO_PIECES | D.DBG_FORCE_STREAM), 4: (2, 0),
                 5: (2, D.DBG_FORCE_STREAM), 6: (2, D.DBG_FORCE_STREAM_SEGS)}
# (plan of the tour, context settings, DRX_PATH_* bits the decode must report): the decoders `short` does not reach
TOUR_PATHS = ((1, (2, 8, 0), D.PATH_BLOCKS), (1, (2, 8, D.DBG_LONG_NOT_BLOCKS), D.PATH_LONG),
              (2, (2, 8, 0), D.PATH_BLOCKS | D.PATH_IIR_FUSED), (2, (2, 8, D.DBG_IIR_SEPARATE), D.PATH_BLOCKS | D.PATH_IIR),
              (0, (2, 0, 0), D.PATH_SIMPLE))


def route_tour():
    """On one plan of `short`: every encoder, followed once by each of another encoder, a decode with the walk inside the
    launch, a decode behind a parallel walk and drx_estimate_words -- what the module's route coverage asks of the schedules,
    in one place; then the decoders `short` does not reach, on plans of `long` and `iir` (whose first filter has four taps).
    Step.args["enc"] of an encode: the DRX_ENC_* it must take; args["path"] of a decode: its DRX_PATH_* bits."""
    M = Model(["short", "long", "iir"], "tour")
    encs = sorted(TOUR_ENCODERS)

    def enc(e):
        M.set_flags(cfg=(TOUR_ENCODERS[e][0], 8, TOUR_ENCODERS[e][1]))
        M.encode(0).args["enc"] = e
    for e in encs:
        enc(e)
        enc(encs[(encs.index(e) + 1) % len(encs)])
        enc(e)
        M.set_flags(cfg=(2, 8, D.DBG_NO_PARALLEL_WALKS))
        M.decode(0).args["walk"] = "fused"
        enc(e)
        M.set_flags(cfg=DEFAULT_CFG)
        M.decode(0).args["walk"] = "parallel"
        enc(e)
        M.estimate(0)
    for p, cfg, path in TOUR_PATHS:
        M.set_flags(cfg=cfg)
        M.decode(p).args["path"] = path
    M.set_flags(cfg=DEFAULT_CFG)
    return M.geoms, M.steps


def host_sequence(seed, n_steps=24):
    """host_filter steps alone, every fourth one with a damaged stream first."""
    M = Model([], ("host", seed))
    for i in range(n_steps):
        M.host_filter(corrupt=(i % 4 == 3))
    return M.steps


FILTER_CYCLE = ("delta", "fir4", "fir5", "taps64", "lead2", "delta", "fir4")


def filter_cycle():
    """One plan of `short` through FILTER_CYCLE: behind every Plan.set_filter an encode, a decode, a side-band decode, a
    selection, a gather, the gathered batch decoded through Gathered.plan(), and an estimate, each on other data."""
    M = Model(["short"], "filters")
    for name in FILTER_CYCLE:
        M.set_filter(0, name)
        M.encode(0)
        M.decode(0)
        M.decode_sideband(0)
        M.select(0, size=64)
        M.gather(0, size=64)
        M.gather_decode(0, len(M.steps) - 1)
        M.estimate(0)
    return M.geoms, M.steps


def scratch_growth():
    """One plan of `short` through the scratch that a later call may need larger (Buffers::reserve(), csrc/drx_api.h), each
    time smaller, larger, smaller: the selection's staging pair (a list of 1, of 3000, of 1: the first pair holds some 4 KB);
    the gather's scratch beside it, regrown by a SIZING call whose gather then resumes; and a sizing call, a larger selection
    -- which fills the staging pair with its own list -- then the gather the sizing call was for, which must not resume."""
    M = Model(["short"], "growth")
    for n in (1, 3000, 1):
        M.select(0, size=n, sideband=False)
    M.gather(0, size=1)
    M.gather(0, size=3000, op="gather_after_sizing")
    M.gather(0, size=3)
    sized = M.gather_size_only(0, size=64)
    M.select(0, size=5000)
    M.gather(0, same_as=sized)
    return M.geoms, M.steps
