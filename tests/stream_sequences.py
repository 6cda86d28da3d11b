"""Sequences of the calls that READ an encoded batch without decoding it to memory -- wave_stats, wave_bins, decode_window,
decode_windows, find_pulses, transcode, refilter and the two estimates from the stream -- among themselves and among the
operations of tests/call_sequences.py, and what each call must give (a helper module of the tests, not a conftest; no GPU is
needed to import or run it).

These calls rewrite the plan's header tables on every call (by the walk or from a side-band), four of them have a block form
that shares the block decoder's scratch and takes a scratch of its own at the first call that takes the form, find_pulses
regrows a staging buffer, the re-coding calls and the estimates share one scratch, and every kernel begins by reading the
plan's status word.  So every step here works on OTHER data than the plan's previous step: a table, a block summary or a
fallback list left by the call before is then not what this call computes, and a stale read shows.

StreamModel adds one method per operation to call_sequences.Model; the expectations are the numpy references of tests/
(wave_stats_reference, wave_bins_reference, decode_window_reference, decode_windows_reference, find_pulses_reference) applied
to Expect.decoded -- the ORACLE's decode, so a lossy lead is handled -- and the oracle's encode_chunk for the re-coding calls.
Every step also names the form the call must report (expected_form()): the table of the forms, written down by hand from
blocks_batch() / blocks_form_batch() and the lane rates of BlkFormRule, not asked of the library."""
import functools

import numpy as np

import call_sequences as CS
from call_sequences import FILTERS, GEOMETRIES, _seed, expect, opts_of, walk_chunk
from decode_window_reference import windows
from decode_windows_reference import windows_multi
from deltarice_amd import _lib as D
from find_pulses_reference import find_pulses
from oracle import oracle as O
from wave_bins_reference import default_n_bins, wave_bins
from wave_stats_reference import wave_stats_heads

READERS = ("wave_stats", "wave_bins", "decode_window", "decode_windows", "find_pulses", "transcode", "refilter")
NEW_OPS = READERS + ("transcode_size_only", "transcode_after_sizing", "estimate_encoded", "estimate_refiltered",
                     "reader_corrupt_header", "reader_payload_off_by_a_word", "transcode_small")
ERROR_OPS = ("reader_corrupt_header", "reader_payload_off_by_a_word", "transcode_small")
OLD_OPS = tuple(o for o in CS.OPS if o != "host_filter")
ALL_OPS = NEW_OPS + OLD_OPS
PAIR_GEOMS = ("short", "ragged", "long")

THR = {"zeros": -1, "gauss10": 15, "gauss400": 600, "uniform": 20000}  # x polarity: all of a waveform of zeros is one pulse
TARGETS = ("delta", "fir3", "fir4", "lead2", "fir5")
M2 = (2, 8, 32, 32768)
TABLE_SEEDS = 3  # random int64 tables (origins, starts, counts) come from this many seeds per geometry: the references are cached

# ---------------------------------------------------------------------------------------------------------------------
# the forms, by hand
# ---------------------------------------------------------------------------------------------------------------------
# `short` (100 samples) and `ragged` (its shortest WaveformLength is 512, below 2048) take the lane form of every call.  `long`
# has 20 waveforms of 24 000 samples -- one round of blocks against more than 1 ms of lanes -- and `whole` 3 of 65 537: under
# the delta filter they take the block form of wave_stats, find_pulses, decode_windows and transcode; under any other filter
# only transcode (and estimate_words_encoded, which is its sizes pass) stays on blocks: its rule has any_filter set.
# DRX_DBG_NO_LONG_PATHS, DRX_DBG_LONG_NOT_BLOCKS and the call's own *_LANES flag keep a batch on lanes; *_ALL_FALLBACK adds
# FALLBACK_ALL to the block form's word.  wave_bins has no block form.  refilter is always LANES | REFILTER.
BLOCK_GEOMS = ("long", "whole")
FORM_FLAGS = {  # family -> (the flag that keeps it on lanes, the flag that lists every waveform)
    "stats": (D.DBG_STATS_LANES, D.DBG_STATS_ALL_FALLBACK),
    "pulses": (D.DBG_PULSES_LANES, D.DBG_PULSES_ALL_FALLBACK),
    "windows": (D.DBG_WINDOWS_LANES, D.DBG_WINDOWS_ALL_FALLBACK),
    "transcode": (D.DBG_TRANSCODE_LANES, D.DBG_TRANSCODE_ALL_FALLBACK),
}
LANES, BLOCKS, FALLBACK_ALL = 1, 2, 4
PATH_OF = {"stats": D.PATH_STATS, "bins": D.PATH_BINS, "window": D.PATH_WINDOW, "windows": D.PATH_WINDOWS, "pulses": D.PATH_PULSES,
           "transcode": D.PATH_TRANSCODE, "refilter": D.PATH_TRANSCODE}
OBSERVED = set()  # (geometry, filter, call family, form word) the GPU runner saw, all of them asserted against expected_form()


def refilter_form(src, dst):
    """test_gpu_refilter.form_of: REFILTER_SERIAL wherever the pair of filters is not the fast kernels'."""
    from test_gpu_refilter import form_of
    return form_of(src, dst if dst is not None else (1, -1))


def expected_form(family, geom, filt, flags, target=None):
    if family == "bins":
        return LANES
    if family == "window":
        return None  # (drx_decode_window reports no form)
    if family == "refilter":
        return refilter_form(FILTERS[filt], FILTERS[target])
    lanes_flag, all_flag = FORM_FLAGS[family]
    blocks = (geom in BLOCK_GEOMS and not flags & (D.DBG_NO_LONG_PATHS | D.DBG_LONG_NOT_BLOCKS | lanes_flag) and
              (filt == "delta" or family == "transcode"))
    return (BLOCKS | (FALLBACK_ALL if flags & all_flag else 0)) if blocks else LANES


# ---------------------------------------------------------------------------------------------------------------------
# expectations
# ---------------------------------------------------------------------------------------------------------------------
def geom_of(e):
    return (e.start, e.length, e.chunk)


@functools.lru_cache(maxsize=None)
def i64_table(geom, seed, cols, pad):
    """int64 [W, cols]: per waveform, values from -pad to the waveform's length + pad (cols 0: [W])."""
    e = expect(geom, "delta", "zeros")
    rng = np.random.default_rng(_seed("table", geom, seed, cols, pad))
    t = rng.integers(-pad, e.length[:, None] + pad, (e.length.size, max(cols, 1)))
    return t if cols else t[:, 0].copy()


@functools.lru_cache(maxsize=None)
def count_table(geom, seed, n_win):
    """int32 [W]: 0 ... n_win + 1 (a count above n_win means n_win)."""
    W = expect(geom, "delta", "zeros").length.size
    return np.random.default_rng(_seed("counts", geom, seed, n_win)).integers(0, n_win + 2, W).astype(np.int32)


def end_starts(geom, width):
    """int64 [W]: windows that hold every waveform's last sample (what a payload a word off needs to be noticed)."""
    return expect(geom, "delta", "zeros").length - max(1, width // 2)


def table(key):
    """The array behind a table key of a step's arguments (None: no table)."""
    if key is None:
        return None
    kind = key[0]
    if kind == "i64":
        return i64_table(*key[1:])
    if kind == "counts":
        return count_table(*key[1:])
    if kind == "ends":
        return end_starts(*key[1:])
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def _stats(geom, filt, ds, head):
    e = expect(geom, filt, ds)
    return wave_stats_heads(e.decoded, e.Ns, e.Ls, [head])[0]


@functools.lru_cache(maxsize=None)
def _pulses(geom, filt, ds, thr, pol, min_width, max_pulses):
    e = expect(geom, filt, ds)
    return find_pulses(e.decoded, e.Ns, e.Ls, thr, pol, min_width, max_pulses, None, geom_of(e))


@functools.lru_cache(maxsize=None)
def _recoded(geom, filt, ds, target, m2):
    """(words, offsets, n_i) of the batch re-coded at m2: target None: the oracle's encode of x under the plan's taps -- the
    residuals do not depend on m, so this is exact for every filter; else the encode of the DECODED samples under the target."""
    e = expect(geom, filt, ds)
    taps, y = (e.taps, e.x) if target is None else (FILTERS[target], e.decoded)
    chunks = [O.encode_chunk(y[e.at[c]:e.at[c + 1]], opts_of(m2, L, taps)) for c, L in enumerate(e.Ls)]
    tab = [walk_chunk(w, N, L) for w, N, L in zip(chunks, e.Ns, e.Ls)]
    return np.concatenate(chunks), np.concatenate([[0], np.cumsum([w.size for w in chunks])]).astype(np.int64), np.concatenate(tab)


@functools.lru_cache(maxsize=None)
def _estimate_refiltered(geom, filt, ds, target):
    """Expect.estimate of the target filter over the decoded samples."""
    e = expect(geom, filt, ds)
    t = CS.Expect(e.Ns, e.Ls, e.m, FILTERS[target], ds, 0)
    t.x = e.decoded
    return t.estimate


@functools.lru_cache(maxsize=None)
def damaged_stream(geom, filt, ds, c, i, by):
    """tests/test_gpu_lane_reader_verdicts.py::damaged: waveform i of chunk c a word shorter (its last word cut) or longer (a
    zero word appended), its header word and the chunk offsets mended -> (words, offsets, n_i table)."""
    e = expect(geom, filt, ds)
    at = int(e.off[c]) + 1 + int((e.table[e.wave_base[c]:e.wave_base[c] + i].astype(np.int64) + 1).sum())
    n = int(e.words[at])
    assert n == int(e.table[e.wave_base[c] + i])
    payload = e.words[at + 1:at + 1 + n]
    payload = payload[:-1] if by < 0 else np.concatenate([payload, [np.uint32(0)]])
    w = np.concatenate([e.words[:at], [np.uint32(n + by)], payload, e.words[at + 1 + n:]]).astype(np.uint32)
    off = e.off.copy()
    off[c + 1:] += by
    tab = e.table.copy()
    tab[e.wave_base[c] + i] = n + by
    return w, off, tab


def damage_by(e, c, i, rng):
    """-1 or +1, such that the mended header is one every walk accepts: (1 + k) to 25 bits a sample."""
    g = int(e.wave_base[c]) + i
    L, n, k = int(e.length[g]), int(e.table[g]), e.m.bit_length() - 1
    lo, hi = (L * (1 + k) + 31) // 32, (L * 25 + 31) // 32
    ok = [by for by in (-1, 1) if lo <= n + by <= hi]
    return int(rng.choice(ok)) if ok else 0  # (0: a waveform so short that it has one possible n_i -- no victim)


def resolve(key):
    """The arrays behind the keys of this module's steps, flat as the output buffers are; every other key: call_sequences.resolve."""
    kind = key[0]
    if kind == "estimate_refiltered":
        return _estimate_refiltered(*key[1:])
    if kind not in ("stats", "bins", "win", "wins", "pcount", "pulses", "wins_at_pulses", "bins_at_argmax", "rwords", "roff", "rtable",
                    "dwords", "doff", "dtable"):
        return CS.resolve(key)
    geom, filt, ds = key[1:4]
    e = expect(geom, filt, ds)
    if kind == "stats":
        return _stats(geom, filt, ds, key[4]).reshape(-1)
    if kind == "bins":
        bin, n_bins, start, offset = key[4:]
        return wave_bins(e.decoded, e.Ns, e.Ls, bin, n_bins, table(start), offset).reshape(-1)
    if kind == "bins_at_argmax":  # the origin is the ARGMAX column of the statistics of the same batch
        bin, n_bins, offset = key[4:]
        return wave_bins(e.decoded, e.Ns, e.Ls, bin, n_bins, _stats(geom, filt, ds, 0)[:, D.STAT_ARGMAX], offset).reshape(-1)
    if kind == "win":
        width, start, offset, pad = key[4:]
        return windows(e.decoded, e.Ns, e.Ls, table(start), offset, width, pad, geom_of(e)).reshape(-1)
    if kind == "wins":
        width, start, count, offset, pad = key[4:]
        return windows_multi(e.decoded, e.Ns, e.Ls, table(start), table(count), offset, width, pad, geom_of(e)).reshape(-1)
    if kind == "wins_at_pulses":  # the starts are the START column of the pulse records of the same batch, the counts its counts
        width, offset, pad = key[4:7]
        n, p = _pulses(geom, filt, ds, *key[7:])
        return windows_multi(e.decoded, e.Ns, e.Ls, p[:, :, D.PULSE_START], n, offset, width, pad, geom_of(e)).reshape(-1)
    if kind in ("pcount", "pulses"):
        n, p = _pulses(geom, filt, ds, *key[4:])
        return n if kind == "pcount" else p.reshape(-1)
    if kind in ("dwords", "doff", "dtable"):
        w, off, tab = damaged_stream(geom, filt, ds, *key[4:])
        return {"dwords": w, "doff": off, "dtable": tab.view(np.int32)}[kind]
    w, off, tab = _recoded(geom, filt, ds, *key[4:])
    return {"rwords": w, "roff": off, "rtable": tab.view(np.int32)}[kind]


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
class StreamModel(CS.Model):
    """call_sequences.Model with the calls that read the stream.  Every reader draws side-band or walk at random, works on
    another dataset than the plan's previous step, and leaves the plan's n_i table the whole source table."""

    def reader(self, op, family, p, ds, finish, sideband, src, args, out, total=None, target=None, host=None):
        sideband = bool(self.rng.integers(0, 2)) if sideband is None else sideband
        self.tables[p] = (ds, self.filt[p], None)
        form = expected_form(family, self.geoms[p], self.filt[p], self.cfg[2], target)
        s = self.add(op, p, finish, ds=ds, total=total, out=out, host=host,
                     args=dict(args, sideband=sideband, src=src, family=family, form=form, path=PATH_OF[family]))
        return s

    def seed(self):
        return int(self.rng.integers(0, TABLE_SEEDS))

    def longest(self, p):
        return int(expect(self.geoms[p], "delta", "zeros").length.max())

    # -- the readers --
    def wave_stats(self, p, ds=None, finish=True, sideband=None, src=None, head=None):
        ds = self.other_ds(p, ds)
        head = int(self.rng.choice((0, 100))) if head is None else head
        return self.reader("wave_stats", "stats", p, ds, finish, sideband, src, {"head": head}, {"stats": ("exact", self.key("stats", p, ds, head))})

    def wave_bins(self, p, ds=None, finish=True, sideband=None, src=None, bin=None, argmax_of=None):
        """argmax_of: a wave_stats step of the schedule whose ARGMAX column, as it lies in memory, is the origin."""
        ds = self.other_ds(p, ds)
        G = GEOMETRIES[self.geoms[p]]
        L = self.longest(p)
        bin = int(self.rng.choice((1, 16, 17, 250, L))) if bin is None else bin
        offset = int(self.rng.choice((0, -7, 5)))
        full = default_n_bins(G.Ns, G.Ls, bin, offset)
        if full > 2000:  # (a row per sample of a long waveform: its first 40)
            full = 40
        n_bins = full if self.rng.random() < 0.5 else max(full * 2 // 5, 1)  # the default, or one that stops mid-waveform
        if argmax_of is not None:
            key = self.key("bins_at_argmax", p, ds, bin, n_bins, offset)
            start = None
        else:
            start = ("i64", self.geoms[p], self.seed(), 0, 50) if self.rng.random() < 0.5 else None
            key = self.key("bins", p, ds, bin, n_bins, start, offset)
        return self.reader("wave_bins", "bins", p, ds, finish, sideband, src,
                           {"bin": bin, "n_bins": n_bins, "start": start, "offset": offset, "argmax_of": argmax_of}, {"bins": ("exact", key)})

    def decode_window(self, p, ds=None, finish=True, sideband=None, src=None):
        ds = self.other_ds(p, ds)
        width = int(self.rng.choice((8, 24, 100)))
        start = ("i64", self.geoms[p], self.seed(), 0, 50) if self.rng.random() < 0.5 else None
        offset, pad = int(self.rng.choice((0, -5, 33))), int(self.rng.choice((0, -3)))
        return self.reader("decode_window", "window", p, ds, finish, sideband, src, {"width": width, "start": start, "offset": offset, "pad": pad},
                           {"win": ("exact", self.key("win", p, ds, width, start, offset, pad))})

    def decode_windows(self, p, ds=None, finish=True, sideband=None, src=None, pulses_of=None):
        """pulses_of: a find_pulses step of the schedule whose START column and counts, as they lie in memory, are the windows."""
        ds = self.other_ds(p, ds)
        width, offset, pad = int(self.rng.choice((8, 24, 100))), int(self.rng.choice((0, -5))), int(self.rng.choice((0, -3)))
        if pulses_of is not None:
            a = self.steps[pulses_of].args
            n_win, start, count = a["max_pulses"], None, None
            key = self.key("wins_at_pulses", p, ds, width, offset, pad, a["thr"], a["polarity"], a["min_width"], a["max_pulses"])
        else:
            n_win = int(self.rng.choice((1, 3)))
            start = ("i64", self.geoms[p], self.seed(), n_win, 50)
            count = ("counts", self.geoms[p], self.seed(), n_win) if self.rng.random() < 0.5 else None
            key = self.key("wins", p, ds, width, start, count, offset, pad)
        return self.reader("decode_windows", "windows", p, ds, finish, sideband, src,
                           {"width": width, "n_win": n_win, "start": start, "count": count, "offset": offset, "pad": pad, "pulses_of": pulses_of},
                           {"wins": ("exact", key)})

    def find_pulses(self, p, ds=None, finish=True, sideband=None, src=None, max_pulses=None):
        ds = self.other_ds(p, ds)
        pol = int(self.rng.choice((1, -1)))
        thr, mw = pol * THR[ds], int(self.rng.choice((1, 3)))
        mp = int(self.rng.choice((0, 1, 4, 64))) if max_pulses is None else max_pulses
        out = {"pcount": ("exact", self.key("pcount", p, ds, thr, pol, mw, mp))}
        if mp:
            out["pulses"] = ("exact", self.key("pulses", p, ds, thr, pol, mw, mp))
        return self.reader("find_pulses", "pulses", p, ds, finish, sideband, src, {"thr": thr, "polarity": pol, "min_width": mw, "max_pulses": mp}, out)

    def draw_m2(self, p, ds):
        ms = M2 + ((1,) if expect(self.geoms[p], self.filt[p], ds).estimate[1] else ())  # (k = 0 only while every zig-zag value is below 32768)
        return int(self.rng.choice(ms))

    def transcode(self, p, ds=None, finish=True, sideband=None, src=None, op="transcode", same_as=None):
        """same_as: an earlier transcode_size_only step of the plan, whose dataset, parameter and side-band this call repeats."""
        if same_as is not None:
            ds, m2, sideband = self.other_ds(p, same_as.ds), same_as.args["m2"], same_as.args["sideband"]
        else:
            ds = self.other_ds(p, ds)
            m2 = self.draw_m2(p, ds)
        k = (self.geoms[p], self.filt[p], ds, None, m2)
        out = {"toff": ("exact", ("roff",) + k), "ttable": ("exact", ("rtable",) + k)}
        args = {"m2": m2, "total_key": ("rwords",) + k}  # (Step.total is the size of that array: the runner asks for it, not the model)
        if op == "transcode_small":  # capacity = needed - 5: status 3, the total still the oracle's, not one word written
            out = {"twords": ("intact", None), "toff": ("guards", None), "ttable": ("guards", None)}
            args["cap_short_by"] = 5
        elif op != "transcode_size_only":
            out["twords"] = ("exact", ("rwords",) + k)
        s = self.reader(op, "transcode", p, ds, finish, sideband, src, args, out)
        if op == "transcode_small":
            s.status = 3
            self.tables[p] = None
        return s

    def transcode_size_only(self, p, ds=None, finish=True, **kw):
        return self.transcode(p, ds, finish, op="transcode_size_only", **kw)

    def transcode_after_sizing(self, p, ds=None, finish=True, **kw):
        return self.transcode(p, ds, finish, op="transcode_after_sizing", **kw)

    def transcode_small(self, p, ds=None, finish=True, **kw):
        return self.transcode(p, ds, finish, op="transcode_small", **kw)

    def refilter(self, p, ds=None, finish=True, sideband=None, src=None):
        ds = self.other_ds(p, ds)
        target = str(self.rng.choice(TARGETS))
        m2 = int(self.rng.choice(M2))
        k = (self.geoms[p], self.filt[p], ds, target, m2)
        return self.reader("refilter", "refilter", p, ds, finish, sideband, src, {"target": target, "m2": m2, "total_key": ("rwords",) + k},
                           {"twords": ("exact", ("rwords",) + k), "toff": ("exact", ("roff",) + k), "ttable": ("exact", ("rtable",) + k)},
                           target=target)

    def estimate_encoded(self, p, ds=None, finish=True, sideband=None):
        ds = self.other_ds(p, ds)
        return self.reader("estimate_encoded", "transcode", p, ds, True, sideband, None, {}, {}, host=("estimate", self.geoms[p], self.filt[p], ds))

    def estimate_refiltered(self, p, ds=None, finish=True, sideband=None):
        ds = self.other_ds(p, ds)
        target = str(self.rng.choice(TARGETS))
        return self.reader("estimate_refiltered", "refilter", p, ds, True, sideband, None, {"target": target}, {}, target=target,
                           host=("estimate_refiltered", self.geoms[p], self.filt[p], ds, target))

    # -- the readers on streams that must be refused --
    def bad_reader(self, op, p, ds, finish, reader, damage):
        """One of READERS on a damaged stream: status 4, the outputs' guards intact (their payload is undefined).  Its windows
        hold every waveform's last sample: a window reads no payload beyond its last code."""
        reader = str(self.rng.choice(READERS)) if reader is None else reader
        n0 = len(self.steps)
        s = getattr(self, reader)(p, ds, finish)
        assert len(self.steps) == n0 + 1
        s.args.update(reader=reader, damage=damage)
        if reader == "decode_window":
            s.args.update(start=("ends", s.geom, s.args["width"]), offset=0)
        if reader == "decode_windows":
            s.args.update(n_win=1, start=("ends", s.geom, s.args["width"]), count=None, offset=0)
        s.op, s.status, s.total = op, 4, None
        s.args.pop("total_key", None)
        s.out = {name: ("guards", None) for name in s.out}
        self.tables[p] = None
        return s

    def reader_corrupt_header(self, p, ds=None, finish=True, reader=None):
        ds = self.other_ds(p, ds)
        e = expect(self.geoms[p], self.filt[p], ds)
        c = int(self.rng.integers(0, len(e.Ns)))
        i = int(self.rng.integers(0, e.wave_base[c + 1] - e.wave_base[c]))
        kind = "total" if self.rng.random() < 0.4 else "n_plus"
        s = self.bad_reader("reader_corrupt_header", p, ds, finish, reader, ("corrupt", kind, c, i))
        s.args["sideband"] = False  # (a header is the walk's to read)
        return s

    def reader_payload_off_by_a_word(self, p, ds=None, finish=True, reader=None):
        ds = self.other_ds(p, ds)
        e = expect(self.geoms[p], self.filt[p], ds)
        by = 0
        while not by:
            c = int(self.rng.integers(0, len(e.Ns)))
            i = int(self.rng.integers(0, e.wave_base[c + 1] - e.wave_base[c]))
            by = damage_by(e, c, i, self.rng)
        return self.bad_reader("reader_payload_off_by_a_word", p, ds, finish, reader, ("payload", c, i, by))


# ---------------------------------------------------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------------------------------------------------
def pair_ops(a):
    """The operations B that follow A in stream_pairs: every one where A is new, the new ones where it is not."""
    return ALL_OPS if a in NEW_OPS else NEW_OPS


@functools.lru_cache(maxsize=None)
def stream_pairs(geom):
    """Every ordered pair (A, B) on ONE plan of the geometry where at least one of the two is an operation of this module, both
    from NEW_OPS and call_sequences.OPS without host_filter; the error operations are As too, so B must start clean.
    -> {A: (plans' geometries, steps, [(index of A, index of B)])}: a plan per A, so that the GPU test runs by (geometry, A)."""
    out = {}
    for a in ALL_OPS:
        M = StreamModel([geom], ("stream pairs", a))
        where = []
        for b in pair_ops(a):
            M.do(a, 0)
            M.do(b, 0)
            where.append((len(M.steps) - 2, len(M.steps) - 1))
        if any(s.op == "set_flags" for s in M.steps):
            M.set_flags(cfg=CS.DEFAULT_CFG)
        out[a] = (M.geoms, M.steps, where)
    return out


def stream_chains():
    """Chains with no finish between calls, every result in a buffer of its own, one finish per plan at the end.
    -> [(name, geometries, steps)]"""
    chains = []

    def chain(name, geoms, build):
        M = StreamModel(geoms, ("stream chain", name))
        build(M)
        last = {}
        for s in M.steps:
            if s.plan >= 0 and s.op not in ("set_filter", "estimate", "read_wave_words", "estimate_encoded", "estimate_refiltered"):
                last[s.plan] = s
        for p, s in sorted(last.items()):
            M.add("finish", p, status=s.status, total=s.total, args={"total_key": s.args.get("total_key")} if s.status == 0 else {})
        chains.append((name, M.geoms, M.steps))

    def blocks(M):  # (under the delta filter every one of these but wave_bins takes d_blk)
        M.decode(0, "gauss10", finish=False)
        M.wave_stats(0, "uniform", finish=False)
        M.find_pulses(0, "gauss400", finish=False)
        M.decode_windows(0, "zeros", finish=False)
        M.transcode(0, "gauss10", finish=False)
        M.wave_bins(0, "uniform", finish=False)
    chain("the block forms and the block decoder back to back", ["long"], blocks)

    def staging(M):
        for ds, mp in (("uniform", 1), ("gauss400", 64), ("gauss10", 2)):
            M.find_pulses(0, ds, finish=False, max_pulses=mp)
    chain("the pulse staging regrows with a call in flight", ["long"], staging)

    def pipeline(M, geom_is_long):  # (every call's arguments lie on the device, written by an earlier call of the chain)
        M.encode(0, "gauss400", finish=False)
        M.find_pulses(0, "gauss400", finish=False, sideband=False, src=0, max_pulses=4)
        M.decode_windows(0, "gauss400", finish=False, sideband=False, src=0, pulses_of=1)
        M.wave_stats(0, "gauss400", finish=False, sideband=False, src=0, head=0)
        M.wave_bins(0, "gauss400", finish=False, sideband=False, src=0, bin=250 if geom_is_long else 16, argmax_of=3)
    chain("the pipeline on device-side arguments, few long waveforms", ["long"], lambda M: pipeline(M, True))
    chain("the pipeline on device-side arguments, many short waveforms", ["short"], lambda M: pipeline(M, False))

    def lost_damage(M, first):
        M.reader_payload_off_by_a_word(0, "gauss10", finish=False, reader=first)
        M.wave_bins(0, "uniform", finish=False)
        M.find_pulses(0, "gauss400", finish=False)
        M.transcode(0, "zeros", finish=False)
    chain("a payload a word off, then three good readers (lanes)", ["short"], lambda M: lost_damage(M, "wave_stats"))
    chain("a payload a word off, then three good readers (blocks)", ["long"], lambda M: lost_damage(M, "wave_stats"))

    def stale_resume(M, sideband):
        for op in ("wave_stats", "find_pulses", "transcode"):
            sized = M.gather_size_only(0, finish=False, size=64)
            M.do(op, 0, finish=False, sideband=sideband)
            M.gather(0, finish=False, same_as=sized)
    chain("a gather's sizing call, a reader by the walk, then the same gather", ["ragged"], lambda M: stale_resume(M, False))
    chain("a gather's sizing call, a reader by the side-band, then the same gather", ["long"], lambda M: stale_resume(M, True))

    def sizing(M):
        sized = M.transcode_size_only(0, "gauss10", finish=False)
        M.wave_stats(0, "uniform", finish=False)
        M.refilter(0, "gauss400", finish=False)
        M.transcode(0, finish=False, same_as=sized)
    chain("a transcode's sizing call, statistics and a refilter, then the transcode", ["long"], sizing)
    chain("a transcode's sizing call, statistics and a refilter, then the transcode (lanes)", ["ragged"], sizing)
    return chains


SESSION_READERS = ("wave_stats", "wave_bins", "decode_window", "decode_windows", "find_pulses", "transcode", "transcode_after_sizing", "refilter",
                   "estimate_encoded", "estimate_refiltered")
LONG_CYCLE = ("delta", "fir3", "lead2", "delta")


def stream_filter_cycle():
    """`long` through LONG_CYCLE and `short` through call_sequences.FILTER_CYCLE: every reader behind every set_filter, on other
    data each, the forms asserted as they flip."""
    M = StreamModel(["long", "short"], "stream filters")
    for p, cycle in ((0, LONG_CYCLE), (1, CS.FILTER_CYCLE)):
        for name in cycle:
            M.set_filter(p, name)
            for op in SESSION_READERS:
                M.do(op, p)
    return M.geoms, M.steps


FORMS = {"stats": "wave_stats", "pulses": "find_pulses", "windows": "decode_windows", "transcode": "transcode"}


def stream_form_scratch(family):
    """A NEW plan of `long`: the form's first call runs under its *_LANES flag, so the form's scratch does not exist behind it;
    then flags 0 (the call that allocates), *_ALL_FALLBACK, DRX_DBG_NO_LONG_PATHS and 0 again, each call on other data."""
    M = StreamModel(["long"], ("form scratch", family))
    lanes_flag, all_flag = FORM_FLAGS[family]
    for flags in (lanes_flag, 0, all_flag, D.DBG_NO_LONG_PATHS, 0):
        M.set_flags(cfg=(2, 8, flags))
        M.do(FORMS[family], 0)
        if family == "transcode":
            M.estimate_encoded(0)
    M.set_flags(cfg=CS.DEFAULT_CFG)
    return M.geoms, M.steps


SESSION_GEOMS = {0: ("short", "long", "ragged"), 1: ("short", "long", "whole")}


def stream_session(seed, n_steps=300):
    """call_sequences.session over the operations of both modules: every "error of this module, then a good call of every other
    kind on the same plan" transition, eight more of every operation of this module, dealt like a deck; random operations of
    both modules fill the rest."""
    geoms = SESSION_GEOMS[seed]
    M = StreamModel(geoms, ("stream session", seed))
    good = [o for o in ALL_OPS if o not in ERROR_OPS + CS.ERROR_OPS]
    deck = [(e, g) for e in ERROR_OPS for g in good] + [(o,) for o in NEW_OPS if o not in ERROR_OPS for _ in range(8)]
    deck = [deck[i] for i in M.rng.permutation(len(deck))]
    while len(M.steps) < n_steps:
        block = deck.pop() if deck else (str(M.rng.choice(ALL_OPS)),)
        p = int(M.rng.integers(0, 3))
        M.do(block[0], p)
        if len(block) == 2:
            if M.rng.random() < 0.5:
                M.do(str(M.rng.choice([o for o in good if o != "set_flags"])), (p + 1 + int(M.rng.integers(0, 2))) % 3)
            M.do(block[1], p)
    M.set_flags(cfg=CS.DEFAULT_CFG)
    return M.geoms, M.steps
