"""GPU: drx_decode_select and drx_gather_encoded over the data the full codec is held to -- every RiceParameter and signal
kind, payloads of exact sizes, code lengths that differ inside a chunk, general filters, lists longer than a launch's grid,
in_words given as a capacity.

Every comparison is exact.  The streams are the oracle's, the expected rows the oracle's input (its decode_chunk where a filter
is lossy), the expected bytes oracle.encode_chunk of the gathered samples or, for the largest list, a numpy range-gather of
the oracle's stream.  Every cell runs both entry points with and without the side-band table, the gather in both copy forms,
and asserts DRX_PATH_SELECT / DRX_PATH_GATHER.  tests/test_selection_shapes.py holds the shapes and shows, without a GPU,
which path each of them reaches."""
import numpy as np
import pytest
import torch

import test_selection_shapes as S
from deltarice_amd import _lib as D
from fuzz_parity import data as fuzz_data
from test_gpu_gather import Expected, check as gather_check, valid_part
from test_gpu_long_filters import TAPS
from test_gpu_parity import make_data
from test_gpu_placement import FF, run
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, expected_rows

pytestmark = pytest.mark.gpu


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


def both(ctx, O, st, x, m, taps, sel, gathers, what, trips=True):
    """decode_select of `sel`, gather_encoded of every (list, waveforms per chunk) of `gathers`: side-band off and on, the
    gather by both copy forms.  (gather_check: a list that breaks the one-length rule must be refused, and its valid part
    and a chunk that ends in the short waveform are gathered instead.)"""
    for sideband in (False, True):
        st.check(sel, sideband, what)
    try:
        for flags in (0, D.DBG_GATHER_OTHER_COPY):
            ctx.set_option("debug_flags", flags)
            for gsel, cw in gathers:
                gather_check(ctx, O, st, x, m, taps, gsel, cw, what + (cw, flags), trips=trips and flags == 0)
    finally:
        ctx.set_option("debug_flags", 0)


def reversed_and_duplicates(rng, W):
    d = rng.integers(0, W, 11)
    return np.arange(W)[::-1], np.concatenate([d, d[:5]])  # all of them; 16 with duplicates


# --------------------------------------------------------------------------- (a) RiceParameter x signal kind
KINDS = ("gauss10", "gauss300", "uniform", "zeros", "ramp", "steps", "pulses")
GEOMETRIES = ((3, 40, 1000), (2, 6, 20000))  # chunks, waveforms, WaveformLength; the last waveform a third shorter


def kind_data(rng, kind, n, k):
    if k == 0 and kind == "uniform":
        kind = "zeros"  # M = 1 is defined only while z < 32768 (the rule of tests/fuzz_parity.py): no full-range data ...
    x = fuzz_data(rng, kind, n, k) if kind == "pulses" else make_data(rng, kind, n)
    return (x // 4).astype(np.int16) if k == 0 else x  # ... and a quarter of the amplitude


# (the id says what the k = 0 rule makes of the uniform kind: that cell repeats 0-zeros with another draw of the lists)
@pytest.mark.parametrize("k,kind", [pytest.param(k, kind, id=f"{k}-{kind}" + "_as_zeros" * (k == 0 and kind == "uniform"))
                                    for k in range(16) for kind in KINDS])
def test_every_rice_parameter_and_signal_kind(ctx, O, k, kind):
    rng = np.random.default_rng((k, KINDS.index(kind)))
    for n_chunks, W, L in GEOMETRIES:
        N = W * L - L // 3
        x = np.concatenate([kind_data(rng, kind, N, k) for _ in range(n_chunks)])
        st = Stream(ctx, O, x, [N] * n_chunks, [L] * n_chunks, 1 << k)
        try:
            for sel in reversed_and_duplicates(rng, st.start.size):
                both(ctx, O, st, x, 1 << k, None, sel, [(sel, 1), (sel, 7)], (k, kind, L, sel.size))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- (b) exact payload sizes
def test_payloads_of_exact_sizes(ctx, O):
    """n_i of 1, 2, whole 16-word segments, whole 1024-word blocks and one word either side; entries of kGcPiece words and
    one either side, of two pieces, of fewer than four words -- in codes of random content (every one an escape) and in
    codes that never re-synchronise (zeros)."""
    x, Ns, Ls, n_want = S.exact_batch()
    n_i, _ = S.chain(O, x, Ns, Ls, S.EXACT_M)
    assert np.array_equal(n_i, n_want)  # on the host, before any GPU call
    st = Stream(ctx, O, x, Ns, Ls, S.EXACT_M)
    try:
        assert np.array_equal(st.table.cpu().numpy().view(np.uint32), n_want)
        W = st.start.size
        every = np.arange(W)
        shuffled = np.random.default_rng(30).permutation(W)
        per_length = [(every[c * S.EXACT_WAVES:(c + 1) * S.EXACT_WAVES], 3) for c in range(len(Ns))]
        both(ctx, O, st, x, S.EXACT_M, None, every, per_length + [(shuffled, 1)], ("exact",))
        st.check(shuffled, False, "exact, shuffled")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- (c) mixed code lengths in one chunk
def test_silent_and_full_range_waveforms_alternate(ctx, O):
    """The batch's mean code length gives slots = 2; a loud entry has more than 2 * kGcPiece words: its wavefronts take a
    second piece each."""
    x, Ns, Ls = S.levels_batch()
    m = S.LEVELS["m"]
    st = Stream(ctx, O, x, Ns, Ls, m)
    try:
        rng = np.random.default_rng(31)
        for sel in reversed_and_duplicates(rng, st.start.size):
            both(ctx, O, st, x, m, None, sel, [(sel, 1), (sel, 5)], ("levels", sel.size))
    finally:
        st.plan.close()


def edges_and_random(rng, W, loud_from):
    """Waveforms of chunks 0 and 2 of three: the first, the last silent one, the first loud one, the short last one; 20
    random ones of each chunk; duplicates."""
    edge = np.array([0, loud_from - 1, loud_from, W - 1, 2 * W, 2 * W + loud_from, 3 * W - 1])
    return np.concatenate([edge, rng.integers(0, W, 20), 2 * W + rng.integers(0, W, 20), edge[:3]])


def test_silent_and_loud_parts_of_a_chunk(ctx, O):
    """The "mixed" data of test_chunk_wide_walk_by_chains, k = 0: three quarters of each chunk one bit per sample, the rest
    escapes.  k_walk_sparse's chains hold from 2 to 56 headers there (it still walks the chunk itself)."""
    x, Ns, Ls = S.silent_loud_batch()
    g = S.SILENT_LOUD
    st = Stream(ctx, O, x, Ns, Ls, g["m"])
    try:
        sel = edges_and_random(np.random.default_rng(32), g["W"], (3 * g["W"]) // 4)
        assert set(st.chunk[sel].tolist()) == {0, 2}
        both(ctx, O, st, x, g["m"], None, sel, [(sel, 1), (sel, 7)], ("silent-loud",))
    finally:
        st.plan.close()


def test_selection_in_chunks_the_chain_walk_gives_up_on(ctx, O):
    """400 silent waveforms in front of 560 loud ones: k_walk_sparse's first chain meets more than kSwCap headers, the chunk
    is flagged in d_fail and k_walk_scalar_only walks it -- here behind a selection, through its chunk list: chunks 0 and 2
    of three."""
    x, Ns, Ls = S.chain_overflow_batch()
    g = S.CHAIN_OVERFLOW
    st = Stream(ctx, O, x, Ns, Ls, g["m"])
    try:
        sel = edges_and_random(np.random.default_rng(36), g["W"], g["quiet"])
        assert set(st.chunk[sel].tolist()) == {0, 2}
        both(ctx, O, st, x, g["m"], None, sel, [(sel, 1), (sel, 7)], ("chain-overflow",))
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- (d) general filters: a lane per waveform
def filters():
    rng = np.random.default_rng(24)
    long_a = (-1,) + tuple(int(v) for v in rng.integers(-2, 3, 63))  # DRX_MAX_TAPS: the whole history ring
    long_b = (3,) + tuple(int(v) for v in rng.integers(-2, 3, 63))   # ... and lossy
    return list(TAPS) + [(2, -1), (1, 70000, -5), (1, -1, 1, -1, 1), long_a, long_b]


FILTERS = filters()
# WaveformLength 1, 3 and 1000 (the short ones shorter than every filter but the one-tap ones), each with a shorter last waveform
# where there can be one; a ragged plan
FILTER_PLANS = (([47] * 3, [1] * 3), ([3 * 40 + 2] * 3, [3] * 3), ([1000 * 7 + 333] * 3, [1000] * 3),
                ([3 * 20 + 1, 1000 * 3 + 500, 64 * 5 + 10, 2500 * 7], [3, 1000, 64, 2500]))


@pytest.mark.parametrize("taps", FILTERS, ids=lambda t: "taps%d_%s" % (len(t), "_".join(str(v) for v in t[:3])))
def test_general_filters(ctx, O, taps):
    """k_select_serial.  Lists of 1, 63, 64, 65 and 130: a last workgroup that is full, one short of it, one lane, two lanes."""
    rng = np.random.default_rng(len(taps) * 1000 + taps[0])
    m = 8
    lossless = abs(taps[0]) == 1
    opts = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps)
    for kind in ("gauss300", "uniform", "steps"):
        for Ns, Ls in FILTER_PLANS:
            x = make_data(rng, kind, sum(Ns))
            st = Stream(ctx, O, x, Ns, Ls, m, taps)
            try:
                # the rows wanted: the oracle's decode of the oracle's stream (the input itself only while taps[0] is +-1)
                dec = np.concatenate([O.decode_chunk(st.words[st.offs[c]:st.offs[c + 1]], (m, L) + opts) for c, L in enumerate(Ls)])
                assert not lossless or np.array_equal(dec, x)
                st.xd = torch.from_numpy(dec).to(ctx.device)
                for n_sel in (1, 63, 64, 65, 130):
                    sel = rng.integers(0, st.start.size, n_sel)
                    both(ctx, O, st, x, m, taps, sel, [(sel, 7)], (taps[:3], kind, Ls[0], len(Ns), n_sel), trips=lossless)
            finally:
                st.plan.close()


# --------------------------------------------------------------------------- (e) lists beyond the launch caps
def test_lists_beyond_the_launch_caps(ctx, O):
    """More entries than k_decode_select has wavefronts (2^20), than k_gather_scan has lanes for blocks of entries (2^20), than
    k_gather_waves has wavefronts (2^22): each strides over its list."""
    g = S.CAPS
    L, cw, m = g["L"], g["cw"], g["m"]
    x, Ns, Ls = S.caps_batch()
    st = Stream(ctx, O, x, Ns, Ls, m)
    plan = st.plan
    try:
        W = st.start.size
        rng = np.random.default_rng(33)
        rows = st.xd.view(W, L)
        sel = rng.integers(0, W, g["n_select"])
        want = rows.index_select(0, torch.from_numpy(sel).to(ctx.device))
        for tab in (None, st.table):
            y = plan.decode_select(st.enc, sel, wave_words=tab)
            assert plan.last_decode_path() == D.PATH_SELECT
            assert torch.equal(y, want), ("select", tab is not None)
            del y
        del want

        # the bytes wanted: a range-gather of the oracle's stream by the oracle's header chain
        sel = rng.integers(0, W, g["n_gather"])
        n_src = st.table.cpu().numpy().view(np.uint32).astype(np.int64)
        src = np.empty(W, np.int64)  # every waveform's header word
        for c in range(len(Ns)):
            w0, w1 = c * g["W"], (c + 1) * g["W"]
            src[w0:w1] = st.offs[c] + 1 + np.cumsum(n_src[w0:w1] + 1) - (n_src[w0:w1] + 1)
        cnt = n_src[sel] + 1
        n_out = -(-sel.size // cw)
        dst = np.cumsum(cnt) - cnt + np.arange(sel.size) // cw + 1
        total = int(cnt.sum()) + n_out
        assert total < 1 << 31
        offs = np.concatenate([dst[::cw] - 1, [total]])
        pos = np.repeat((np.arange(sel.size) // cw + 1).astype(np.int32), cnt) + np.arange(total - n_out, dtype=np.int32)
        bytes_want = np.empty(total, np.uint32)
        bytes_want[pos] = st.words[np.repeat((src[sel] - dst).astype(np.int32), cnt) + pos]
        N_c = np.full(n_out, cw * L, np.int64)
        N_c[-1] = (sel.size - (n_out - 1) * cw) * L
        bytes_want[offs[:-1]] = N_c
        del pos
        want_d = torch.from_numpy(bytes_want.view(np.int32)).to(ctx.device)
        offs_d = torch.from_numpy(offs).to(ctx.device)
        n_d = torch.from_numpy(n_src[sel].astype(np.uint32).view(np.int32)).to(ctx.device)
        # chunk 0, a middle one, the last (short) one and those that hold entries 2^20 j: the oracle's own encoding of their samples
        spots = sorted({0, n_out // 2, n_out - 1} | {(j << 20) // cw for j in range(1, (sel.size >> 20) + 1)})
        assert len(spots) >= 5
        spot_words = {c: O.encode_chunk(x.reshape(W, L)[sel[c * cw:(c + 1) * cw]].reshape(-1), (m, L)) for c in spots}
        for c, w in spot_words.items():
            assert bytes_want[offs[c]:offs[c + 1]].tobytes() == w.tobytes(), ("the range-gather itself", c)

        first = None
        for flags in (0, D.DBG_GATHER_OTHER_COPY):
            ctx.set_option("debug_flags", flags)
            for tab in (None, st.table):
                cell = (flags, tab is not None)
                got = plan.gather_encoded(st.enc, sel, cw, wave_words=tab)
                assert plan.last_decode_path() == D.PATH_GATHER, cell
                assert got.enc.total_words == total and got.enc.words.numel() == total, cell
                assert torch.equal(got.enc.chunk_word_off, offs_d), cell
                assert torch.equal(got.wave_words, n_d), cell
                assert torch.equal(got.enc.words, want_d), (cell, int((got.enc.words != want_d).nonzero()[0]))
                assert np.array_equal(got.chunk_samples, N_c) and (got.wave_lens == L).all(), cell
                first = first or got
                del got
        ctx.set_option("debug_flags", 0)
        for c, w in spot_words.items():
            assert first.enc.words[offs[c]:offs[c + 1]].cpu().numpy().view(np.uint32).tobytes() == w.tobytes(), c
        gp = first.plan(ctx)  # the result is a batch: its own plan decodes it to the gathered rows
        try:
            y = gp.decode(first.enc)
            assert torch.equal(y.view(-1, L), rows.index_select(0, torch.from_numpy(sel).to(ctx.device)))
        finally:
            gp.close()
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


# --------------------------------------------------------------------------- (f) in_words as a capacity
@pytest.mark.parametrize("name", ["levels", "short"])
def test_in_words_as_a_capacity(ctx, O, name):
    """The stream in a buffer 64 times its size, the rest 0xFFFFFFFF, in_words the buffer's size: the gather then sizes its
    copy by another mean code length (other slots; a wavefront per entry where the stream's own size chooses tiles).  The
    same rows, the same bytes, the slack untouched."""
    if name == "levels":
        (x, Ns, Ls), m = S.levels_batch(), S.LEVELS["m"]
    else:
        Ns, Ls, m, _, sigma = BATCHES[name]
        x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m)
    plan = st.plan
    try:
        total = int(st.offs[-1])
        cap = total * S.CAPACITY_FACTOR
        buf = torch.full((cap,), FF, dtype=torch.int32, device=ctx.device)
        buf[:total].copy_(st.enc.words[:total])
        offs = st.enc.chunk_word_off
        rng = np.random.default_rng(34)
        full = valid_part(st.length, np.arange(st.start.size))
        sel = np.concatenate([full[:1], full[-1:], rng.choice(full, 200)])
        cw, stride = 7, plan.longest_wave()
        rows = expected_rows(st.xd, st.start, st.length, sel, stride, fill=0x5A5A)
        want = Expected(O, x, st.start, st.length, sel, cw, m, None)
        for flags in (0, D.DBG_GATHER_OTHER_COPY):
            ctx.set_option("debug_flags", flags)
            for tab in (None, st.table):
                for in_words in (total, cap):
                    cell = (name, flags, tab is not None, in_words)
                    y = torch.full((sel.size, stride), 0x5A5A, dtype=torch.int16, device=ctx.device)
                    run(ctx, plan, lambda: plan.decode_select_async(buf, offs, sel, out=y, in_words=in_words, wave_words=tab))
                    assert plan.last_decode_path() == D.PATH_SELECT, cell
                    assert torch.equal(y, rows), cell
                    out = torch.full((want.total + 64,), FF, dtype=torch.int32, device=ctx.device)
                    res = []
                    n = run(ctx, plan, lambda: res.append(plan.gather_encoded_async(buf, offs, sel, cw, out, in_words, tab)))
                    assert plan.last_decode_path() == D.PATH_GATHER, cell
                    assert n == want.total, cell
                    assert out[:n].cpu().numpy().view(np.uint32).tobytes() == want.words.tobytes(), cell
                    assert bool((out[n:] == FF).all()), cell
                    assert res[0][1].cpu().tolist() == want.offs, cell
                    assert np.array_equal(res[0][2].cpu().numpy().view(np.uint32), want.n_i), cell
                    assert bool((buf[total:] == FF).all()) and torch.equal(buf[:total], st.enc.words[:total]), cell
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


# --------------------------------------------------------------------------- a walk that failed
@pytest.mark.parametrize("taps", [None, (1, -1, 1, -1)], ids=["delta", "fir4"])
def test_select_follows_no_table_of_a_chunk_that_failed_validation(ctx, O, taps):
    """Regression: k_decode_select and k_select_serial once ran whatever the walk in front of them had reported, indexing the
    stream through tables a rejecting walker may have left partly written.  Like the gather they now return at once: a
    touched chunk with a broken header chain is DRX_ERR_CORRUPT and not one sample is written.  One chunk shape per walker
    of the selection (the chain walk, the LDS block walker, the hop-by-hop one), and the side-band's check."""
    import deltarice_amd as dr
    rng = np.random.default_rng(35)
    for W, L in ((20, 7000), (300, 100), (3, 50000)):
        Ns, Ls = [W * L] * 3, [L] * 3
        x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, 8, taps)
        try:
            at = int(st.offs[1]) + 1  # chunk 1: its second waveform's n_i one too many
            at += int(st.words[at]) + 1
            w = st.words.copy()
            w[at] += 1
            broken = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), st.enc.chunk_word_off, st.enc.total_words)
            sel = np.array([W + 2, 0, W, 2 * W - 1, 3 * W - 1])
            for tab in (None, st.table):
                out = torch.full((sel.size, L), 0x5A5A, dtype=torch.int16, device=ctx.device)
                with pytest.raises(dr.DeltaRiceError) as e:
                    st.plan.decode_select(broken, sel, out=out, wave_words=tab)
                assert e.value.status == 4, (W, L, tab is not None)
                assert bool((out == 0x5A5A).all()), (W, L, tab is not None)
                keep = sel[st.chunk[sel] != 1]  # chunk 1 is not looked at
                y = st.plan.decode_select(broken, keep, wave_words=tab)
                assert torch.equal(y, expected_rows(st.xd, st.start, st.length, keep, L)), (W, L, tab is not None)
        finally:
            st.plan.close()
