"""GPU: drx_decode_windows, the lane and serial forms -- K windows of `width` samples per waveform at per-window starts, parsed
from the encoded stream.

The streams are the oracle's (oracle.encode_chunk), the expected rows numpy's over the oracle's input
(tests/decode_windows_reference.py; for a filter whose lead is not +-1, over the oracle's decode of that stream), the
comparison torch.equal.  Every cell asserts DRX_PATH_WINDOWS alone, plan.finish() == 0 and the form, through the walk and
through the side-band."""
import itertools

import numpy as np
import pytest

from decode_windows_reference import extents, windows_multi
from deltarice_amd import _lib as D
from test_gpu_lane_reader_verdicts import M as VERDICT_M, SHAPES as VERDICT_SHAPES, VICTIMS, damaged
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, header_table  # noqa: F401  (Stream builds its side-band with header_table)
from test_gpu_wave_stats import FILTERS, samples_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS = D.WINDOWS_FORM_LANES, D.WINDOWS_FORM_BLOCKS
# the batches of the route table that take the block form: few long waveforms under the delta filter, and the 800 waveforms of
# 7000 samples of "wide-fused", which leave most of the chip's lanes idle
BLOCK_BATCHES = {"long-2", "long-40", "whole-chunk", "wide-fused"}


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.set_option("debug_flags", 0)
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def dev(ctx, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(ctx.device)


SENTINELS = (0x5A5A, -1)  # what an output holds before a call: alternating, and never the call's pad
_calls = itertools.count()


def prefilled(ctx, shape, pad):
    """An int16 output of `shape`, every element a sentinel that differs from `pad`: the rows must not depend on what they held."""
    s = SENTINELS[next(_calls) % 2]
    if s == int(pad):
        s = SENTINELS[0] if s == SENTINELS[1] else SENTINELS[1]
    assert s != int(pad)
    return torch.full(tuple(shape), s, dtype=torch.int16, device=ctx.device)


def check(ctx, st, y, cases, form=LANES, flags=0, sidebands=(False, True), what="", listed=None):
    """Every (starts [W, K], counts or None, offset, width, pad) x {walk, side-band} on st against numpy over the samples y, into
    a pre-filled output.  listed: what plan.last_windows_listed() must say behind every call (a number, or a predicate).
    Returns the rows of every call, in order."""
    geom = (st.start, st.length, st.chunk)
    gots = []
    ctx.set_option("debug_flags", flags)
    try:
        for starts, counts, offset, width, pad in cases:
            want = torch.from_numpy(windows_multi(y, st.Ns, st.Ls, starts, counts, offset, width, pad, geom)).to(ctx.device)
            sd, cd = dev(ctx, starts, np.int64), dev(ctx, counts, np.int32)
            for sideband in sidebands:
                cell = (what, flags, tuple(np.shape(starts)), counts is not None, offset, width, pad, sideband)
                out = prefilled(ctx, want.shape, pad)
                got = st.plan.decode_windows(st.enc, sd, width, count=cd, offset=offset, pad=pad, out=out, wave_words=st.table if sideband else None)
                assert got.data_ptr() == out.data_ptr() or got.numel() == 0, cell
                assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.finish() == 0, cell
                assert st.plan.last_windows_form() == form, (cell, st.plan.last_windows_form())
                if listed is not None:
                    n = st.plan.last_windows_listed()
                    assert listed(n) if callable(listed) else n == listed, (cell, "listed", n)
                assert got.dtype == torch.int16 and got.shape == want.shape, cell
                if not torch.equal(got, want):
                    bad = torch.nonzero((got != want).flatten(1).any(dim=1)).flatten()
                    g = int(bad[0])
                    p = int(torch.nonzero((got[g] != want[g]).any(dim=1)).flatten()[0])
                    j = int(torch.nonzero(got[g, p] != want[g, p]).flatten()[0])
                    raise AssertionError((cell, f"{bad.numel()} waveforms differ; waveform {g} slot {p} from column {j}",
                                          np.asarray(starts)[g, max(p - 2, 0):p + 3].tolist(), got[g, p, j:j + 8].tolist(), want[g, p, j:j + 8].tolist()))
                gots.append(got)
    finally:
        ctx.set_option("debug_flags", 0)
    return gots


def random_starts(rng, st, K, lo=-50, hi=50):
    """K starts per waveform from [lo, len + hi)"""
    return rng.integers(lo, st.length[:, None] + hi, (st.length.size, K))


def random_counts(rng, W, K):
    """counts in 0 .. K + 1 with a 0 and a K + 1 among them"""
    c = rng.integers(0, K + 2, W)
    c[0], c[-1] = 0, K + 1
    return c


# --------------------------------------------------------------------------- 1. every batch of the route table
@pytest.mark.parametrize("name", list(BATCHES))
def test_windows_every_batch(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        counts = random_counts(rng, st.length.size, 3)
        assert (counts == 0).any() and (counts == 4).any()
        check(ctx, st, samples_of(O, st, x, m, taps), [(random_starts(rng, st, 3), counts, 0, 64, -1)],
              BLOCKS if name in BLOCK_BATCHES else LANES, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. group and round edges
EDGE_STARTS = (-5, 0, 1, 15, 16, 17, 63, 64, 65, 199, 200, 250)


@pytest.fixture(scope="module")
def edges(ctx, O):
    Ns, Ls = [130 * 200 + 37] * 3, [200] * 3  # 131 waveforms per chunk: lanes in two chunks, the last waveform of 37 samples
    x = np.random.default_rng(2).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    yield st, x
    st.plan.close()


@pytest.mark.parametrize("width", [1, 2, 15, 16, 17, 64, 65, 201])
def test_windows_group_and_round_edges(ctx, edges, width):
    st, x = edges
    W = st.length.size
    rng = np.random.default_rng(width)
    # a sorted triple of the edge starts per waveform (repeats allowed), every start in some triple
    triples = np.sort(rng.choice(EDGE_STARTS, (W, 3)), axis=1)
    triples[:len(EDGE_STARTS) // 3] = np.array(EDGE_STARTS).reshape(-1, 3)
    assert set(triples.reshape(-1).tolist()) == set(EDGE_STARTS) and (np.diff(triples, axis=1) >= 0).all()
    check(ctx, st, x, [(triples, None, 0, width, 0x1234), (triples, random_counts(rng, W, 3), 0, width, -2)], what=("edges", width))


# --------------------------------------------------------------------------- 3. order and overlap
@pytest.fixture(scope="module")
def long_rows(ctx, O):
    Ns, Ls = [130 * 7000] * 2, [7000] * 2
    x = np.random.default_rng(3).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    yield st, x
    st.plan.close()


def test_windows_order_and_overlap(ctx, long_rows):
    st, x = long_rows
    W, L = st.length.size, 7000
    rng = np.random.default_rng(31)
    base = np.sort(rng.integers(-100, L + 100, (W, 5)), axis=1)
    lists = {
        "reversed": (base[:, ::-1], 200),
        "shuffled": (rng.permuted(base, axis=1), 200),
        "duplicates": (base[:, [0, 0, 2, 2, 2]], 200),
        "coinciding, unsorted": (base[:, [3, 1, 3, 1, 3]], 200),
        "nested and overlapping": (base[:, :1] + np.array([0, 10, 11, 150, 199])[None, :], 200),
        "mixed parities": (base | (np.arange(5)[None, :] & 1), 77),
        # a window over the whole waveform and its margins beside narrow ones: as starts of one width they are a whole-waveform
        # list (width L + 64 from -32) ...
        "whole waveform, unsorted": (np.stack([np.full(W, -32), rng.integers(-L, L, W), np.full(W, -32)], axis=1), L + 64),
        # ... and narrow windows inside a wide one of the same width that overlaps them all
        "wide and dense": (np.stack([np.full(W, 100), np.full(W, 101), np.full(W, 3000), np.full(W, 100 + 2999)], axis=1), 3000),
    }
    for what, (starts, width) in lists.items():
        starts = np.ascontiguousarray(starts)
        # (260 waveforms of 7000 samples leave most of the chip's lanes idle: the batch takes the block form unless told otherwise)
        check(ctx, st, x, [(starts, None, 0, width, -7)], LANES, flags=D.DBG_WINDOWS_LANES, what=what)
        check(ctx, st, x, [(starts, None, 0, width, -7)], BLOCKS, what=what)
        ctx.set_option("debug_flags", D.DBG_WINDOWS_LANES)
        # the same rows as the sorted permutation gives, row for row
        order = np.argsort(starts, axis=1, kind="stable")
        sd, ss = dev(ctx, starts, np.int64), dev(ctx, np.take_along_axis(starts, order, axis=1), np.int64)
        got, srt = st.plan.decode_windows(st.enc, sd, width, pad=-7), st.plan.decode_windows(st.enc, ss, width, pad=-7)
        od = torch.from_numpy(order).to(ctx.device)
        ctx.set_option("debug_flags", 0)
        assert st.plan.last_windows_form() == LANES
        assert torch.equal(torch.gather(got, 1, od[:, :, None].expand(-1, -1, width)), srt), what


# --------------------------------------------------------------------------- 4. agreement with drx_decode_window
def test_windows_one_window_is_decode_window(ctx, edges, long_rows):
    # (the 260 waveforms of 7000 samples take the block form by default: both forms there)
    for (st, x), widths, cells in ((edges, (1, 16, 33, 201), ((0, LANES),)), (long_rows, (256, 7000), ((0, BLOCKS), (D.DBG_WINDOWS_LANES, LANES)))):
        rng = np.random.default_rng(4)
        starts = random_starts(rng, st, 1)
        sd = dev(ctx, starts, np.int64)
        for width in widths:
            one = st.plan.decode_window(st.enc, sd[:, 0], width, offset=-3, pad=9)
            for flags, form in cells:
                ctx.set_option("debug_flags", flags)
                try:
                    many = st.plan.decode_windows(st.enc, sd, width, offset=-3, pad=9)
                finally:
                    ctx.set_option("debug_flags", 0)
                assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.last_windows_form() == form, (width, flags)
                assert many.shape == (st.length.size, 1, width) and torch.equal(many[:, 0], one), (width, flags)


# --------------------------------------------------------------------------- 5. filters and RiceParameters
@pytest.mark.parametrize("fname", list(FILTERS))
def test_windows_filters(ctx, O, fname):
    taps = FILTERS[fname]
    Ns, Ls = [65 * 300] * 2, [300] * 2
    rng = np.random.default_rng(len(taps))
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        W = st.length.size
        check(ctx, st, samples_of(O, st, x, 8, taps), [(random_starts(rng, st, 3), random_counts(rng, W, 3), 0, 96, -1),
                                                       (random_starts(rng, st, 2), None, -3, 301, 9)], what=fname)
    finally:
        st.plan.close()


@pytest.mark.parametrize("m", [1, 8, 64, 32768])
def test_windows_rice_parameters(ctx, O, m):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    for sigma in (10, 400):
        rng = np.random.default_rng(m + sigma)
        x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, m)
        try:
            W = st.length.size
            check(ctx, st, x, [(np.sort(random_starts(rng, st, 3), axis=1), random_counts(rng, W, 3), 0, 96, -1),
                               (random_starts(rng, st, 3), None, 0, 300, 0)], what=(m, sigma))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 6. where the buffers lie
def test_windows_placements(ctx, O):
    Ns, Ls = [130 * 200 + 37] * 3, [200] * 3
    rng = np.random.default_rng(9)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    K, width, offset, pad = 3, 50, -9, -2
    try:
        starts = np.sort(random_starts(rng, st, K), axis=1)
        counts = random_counts(rng, W, K)
        want = torch.from_numpy(windows_multi(x, Ns, Ls, starts, counts, offset, width, pad)).to(ctx.device)
        # the starts as a column of wider records (the strides of drx_find_pulses' output), and at an address that is 8 mod 16
        records = torch.full((W, K, 5), 12345, dtype=torch.int64, device=ctx.device)
        records[:, :, 3] = dev(ctx, starts, np.int64)
        odd8 = window(W * K, torch.int64, 8, device=ctx.device)
        odd8.t.copy_(dev(ctx, starts, np.int64).reshape(-1))
        cw = window(W, torch.int32, 4, device=ctx.device)
        cw.t.copy_(dev(ctx, counts, np.int32))
        assert odd8.t.data_ptr() % 16 == 8 and cw.t.data_ptr() % 16 == 4
        givens = {"column": records[:, :, 3], "8 mod 16": odd8.t.view(W, K)}
        assert givens["column"].stride() == (5 * K, 5)
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            # (byte offset of d_out, samples between a waveform's rows, samples between waveforms beyond the least, pre-fill)
            for obyte, o_win, extra, fill, given in ((0, width, 0, 0x5A5A, "column"), (2, width + 1, 0, -1, "8 mod 16"), (6, width + 7, 3, 0x5A5A, "column"),
                                                     (14, width, 5, -1, "8 mod 16"), (10, width + 1, 1, 0x5A5A, "column")):
                o_wave = (K - 1) * o_win + width + extra
                yw = window((W - 1) * o_wave + (K - 1) * o_win + width, torch.int16, obyte, fill=fill, device=ctx.device)
                assert yw.t.data_ptr() % 16 == obyte
                for sideband in (False, True):
                    yw.t.fill_(fill)
                    rows = None

                    def launch():
                        nonlocal rows
                        rows = plan.decode_windows_async(ww.t, ow.t, givens[given], width, count=cw.t, offset=offset, pad=pad, out=yw.t,
                                                         out_strides=(o_wave, o_win), in_words=total, wave_words=st.table if sideband else None)
                    assert run(ctx, plan, launch) == 0
                    assert plan.last_decode_path() == D.PATH_WINDOWS and plan.last_windows_form() == LANES
                    same = torch.equal(rows, want)
                    # everything that is not a row kept the pre-fill: the rows put back, the whole buffer is the pre-fill
                    rows.fill_(fill)
                    intact = yw.intact() and ow.intact() and ww.intact() and odd8.intact() and cw.intact() and bool((yw.t == fill).all())
                    assert same and intact, (pname, obyte, o_win, extra, fill, given, sideband, "rows differ" * (not same),
                                             "guard or gap written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
        assert bool((records[:, :, [0, 1, 2, 4]] == 12345).all())
    finally:
        plan.close()


# --------------------------------------------------------------------------- 7. rows beyond 2^32 bytes
def test_windows_rows_beyond_4_gib(ctx, O):
    L, K, width = 300, 3, 40
    o_wave, o_win = (1 << 31) + 24, 1000  # a waveform's rows lie more than 2^31 samples behind the one before
    rng = np.random.default_rng(10)
    x = rng.normal(0, 10, 3 * L).astype(np.int16)
    st = Stream(ctx, O, x, [3 * L], [L], 8)
    try:
        try:
            out = torch.empty(2 * o_wave + (K - 1) * o_win + width, dtype=torch.int16, device=ctx.device)  # 8.6 GB, of which 9 rows are touched
        except (RuntimeError, MemoryError) as e:
            pytest.skip(f"no room for the output: {e}")
        assert out.numel() * 2 > 1 << 33
        starts = np.sort(random_starts(rng, st, K, -10, 10), axis=1)
        want = torch.from_numpy(windows_multi(x, st.Ns, st.Ls, starts, None, 0, width, -9)).to(ctx.device)
        for sideband in (False, True):
            rows = None

            def launch():
                nonlocal rows
                rows = st.plan.decode_windows_async(st.enc.words, st.enc.chunk_word_off, dev(ctx, starts, np.int64), width, pad=-9, out=out,
                                                    out_strides=(o_wave, o_win), in_words=st.enc.total_words,
                                                    wave_words=st.table if sideband else None)
            out.as_strided((3, K, width), (o_wave, o_win, 1)).fill_(0x5A5A)
            assert run(ctx, st.plan, launch) == 0 and st.plan.last_decode_path() == D.PATH_WINDOWS
            assert torch.equal(rows, want), sideband
        del out, rows
    finally:
        st.plan.close()
        torch.cuda.empty_cache()


# --------------------------------------------------------------------------- 8. argument errors
def test_windows_argument_errors(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [65 * 300] * 2, [300] * 2
    rng = np.random.default_rng(11)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good, W = st.plan, st.enc, st.plan.total_waves
    K, width = 2, 64
    starts = np.sort(random_starts(rng, st, K), axis=1)
    sd = dev(ctx, starts, np.int64)
    want = torch.from_numpy(windows_multi(x, Ns, Ls, starts, None, 0, width, -1)).to(ctx.device)

    def clean():
        got = plan.decode_windows(good, sd, width, pad=-1)
        assert torch.equal(got, want) and plan.last_decode_path() == D.PATH_WINDOWS and plan.finish() == 0

    try:
        clean()
        header = st.words.copy()
        header[int(st.offs[1]) + 1] += 1  # the first waveform header of chunk 1: a broken chain
        broken = dr.EncodedBatch(torch.from_numpy(header.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.decode_windows(broken, sd, width)
        assert e.value.status == 4
        clean()  # the plan stays usable, and its next call starts clean
        # DRX_ERR_ARG, nothing launched: the status word keeps the verdict of the call before
        out = torch.full((W, K, width), 0x5A5A, dtype=torch.int16, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.decode_windows_async(broken.words, good.chunk_word_off, sd, width, out=out, in_words=good.total_words)
        lib, w, off, h, nw, o, s = ctx.lib, good.words.data_ptr(), good.chunk_word_off.data_ptr(), plan._h, good.total_words, out.data_ptr(), sd.data_ptr()
        ow, oi = K * width, width
        call, side = lib.drx_decode_windows, lib.drx_decode_windows_with_wave_words
        assert call(h, None, nw, off, s, K, 1, None, K, 0, width, 0, o, ow, oi) == 1
        assert call(h, w, nw, None, s, K, 1, None, K, 0, width, 0, o, ow, oi) == 1
        assert call(h, w, nw, off, None, K, 1, None, K, 0, width, 0, o, ow, oi) == 1
        assert call(h, w, nw, off, s, K, 1, None, K, 0, width, 0, None, ow, oi) == 1
        assert call(h, w, nw, off, s, 0, 1, None, K, 0, width, 0, o, ow, oi) == 1  # start_wave_stride 0
        assert call(h, w, nw, off, s, K, 0, None, K, 0, width, 0, o, ow, oi) == 1  # start_win_stride 0
        assert call(h, w, nw, off, s, K, 1, None, K, 0, width, 0, o, ow, oi - 1) == 1  # a row does not hold its samples
        assert call(h, w, nw, off, s, K, 1, None, K, 0, width, 0, o, ow - 1, oi) == 1  # a waveform's rows overlap the next one's
        assert call(h, w, nw, off, s, K, 1, None, 4, 0, width, 0, o, (1 << 64) - 1, 1 << 63) == 1  # ... by a sum of more than 64 bits
        assert side(h, w, nw, off, None, s, K, 1, None, K, 0, width, 0, o, ow, oi) == 1
        assert side(h, w, nw, off, lib.drx_plan_wave_words(h), s, K, 1, None, K, 0, width, 0, o, ow, oi) == 1
        assert call(h, w, nw, off, s, K, 1, None, K, 0, 0, 0, o, ow, oi) == 0  # width 0: DRX_OK, nothing launched
        assert call(h, w, nw, off, s, K, 1, None, 0, 0, width, 0, o, ow, oi) == 0  # no window slot: DRX_OK, nothing launched
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.finish()
        assert e.value.status == 4
        torch.cuda.synchronize()
        clean()
        before = out.clone()
        assert call(h, w, nw, off, s, K, 1, None, K, 0, 0, 0, o, ow, oi) == 0 and plan.finish() == 0
        assert call(h, w, nw, off, s, K, 1, None, 0, 0, width, 0, o, ow, oi) == 0 and plan.finish() == 0
        torch.cuda.synchronize()
        assert torch.equal(out, before) and plan.last_decode_path() == D.PATH_WINDOWS
        # a decode behind a windows call reports its own path
        assert torch.equal(plan.decode(good), st.xd) and plan.last_decode_path() not in (0, D.PATH_WINDOWS)
        clean()
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. verdicts
@pytest.fixture(scope="module")
def verdict_streams(ctx, O):
    out = {}
    for name, (Ns, Ls, taps) in VERDICT_SHAPES.items():
        x = np.random.default_rng(len(name)).normal(0, 10, sum(Ns)).astype(np.int16)
        out[name] = (Stream(ctx, O, x, Ns, Ls, VERDICT_M, taps), x)
    yield out
    for st, _ in out.values():
        st.plan.close()


@pytest.mark.parametrize("by", [-1, 1], ids=["codes end after the last word", "codes end before the last word"])
@pytest.mark.parametrize("victim", VICTIMS, ids=lambda v: f"chunk{v[0]}-wave{v[1]}")
@pytest.mark.parametrize("shape", list(VERDICT_SHAPES))
def test_windows_payload_a_word_off_is_corrupt(ctx, verdict_streams, shape, victim, by):
    import deltarice_amd as dr
    st, x = verdict_streams[shape]
    W = st.length.size
    enc, table = damaged(ctx, st, *victim, by)
    # the second window of every waveform reaches its last sample: e_g = len_g
    starts = np.stack([np.zeros(W, np.int64), st.length - 10], axis=1)
    assert np.array_equal(extents(st.Ns, st.Ls, starts, None, 0, 24), st.length)
    sd = dev(ctx, starts, np.int64)
    for kw in ({}, dict(wave_words=table)):
        with pytest.raises(dr.DeltaRiceError) as e:
            st.plan.decode_windows(enc, sd, 24, **kw)
        assert e.value.status == 4, sorted(kw)


@pytest.mark.parametrize("by", [-1, 1], ids=["shorter", "longer"])
@pytest.mark.parametrize("victim", VICTIMS[:3], ids=lambda v: f"chunk{v[0]}-wave{v[1]}")  # (waveforms longer than the windows)
@pytest.mark.parametrize("shape", list(VERDICT_SHAPES))
def test_windows_do_not_report_damage_behind_them(ctx, verdict_streams, shape, victim, by):
    st, x = verdict_streams[shape]
    Ns, Ls, _ = VERDICT_SHAPES[shape]
    W = st.length.size
    enc, table = damaged(ctx, st, *victim, by)
    starts = np.stack([np.full(W, 2), np.zeros(W, np.int64)], axis=1)  # (unsorted; e_g = width + 2)
    g = int(np.flatnonzero(st.chunk == victim[0])[0]) + victim[1]  # the damaged waveform
    for width in (6, 22):  # a masked group alone; an unmasked one and a masked one
        assert extents(Ns, Ls, starts, None, 0, width)[g] == width + 2 < st.length[g]
        want = torch.from_numpy(windows_multi(x, Ns, Ls, starts, None, 0, width, -3, (st.start, st.length, st.chunk))).to(ctx.device)
        for kw in ({}, dict(wave_words=table)):
            got = st.plan.decode_windows(enc, dev(ctx, starts, np.int64), width, pad=-3, **kw)
            assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.finish() == 0, (width, sorted(kw))
            assert torch.equal(got, want), (width, sorted(kw))
