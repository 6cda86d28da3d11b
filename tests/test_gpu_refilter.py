"""GPU: drx_transcode_filter / drx_estimate_words_encoded_filter -- an encoded batch re-coded under another prediction filter
and another RiceParameter without decoding it to memory.

The streams are the oracle's (oracle.encode_chunk), the expectation of a cell is Want(O, y, Ns, Ls, m2, taps2) with y the
oracle's decode of the source (for a source lead of +-1: the samples themselves), the comparisons tobytes() / torch.equal:
no tolerance anywhere.  Every cell asserts DRX_PATH_TRANSCODE alone and the form word: LANES | REFILTER, REFILTER_SERIAL
exactly where the pair of filters is not the fast kernels', never BLOCKS."""
import ctypes as C
import math

import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_offsets64 import SMALL
from test_gpu_placement import FF, run, window
from test_gpu_select import Stream, header_table
from test_gpu_transcode import Want, opts_of, same_stream
from test_gpu_wave_stats import crafted_rows
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGE = ([130 * 200 + 37] * 3, [200] * 3)  # 131 waveforms per chunk: two wavefronts and two lanes, the last one of 37 samples
FIR4 = (1, -1, 1, -1)
FIR4B = (-1, 2, -1, 1)
FIR5 = (1, -1, 1, -1, 1)
TAPS64 = tuple([1] + [int(v) for v in np.random.default_rng(64).integers(-2, 3, 62)] + [-1])  # 64 taps, lead 1, no zero at the end
TARGETS = {"delta": (1, -1), "fir3": (1, -2, 1), "fir4": FIR4, "fir4b": FIR4B, "lead2": (2, -1), "fir5": FIR5, "taps64": TAPS64}
# a lane per waveform of 50 000 and 261 001 samples through 64 taps is seconds: those batches keep the 5-tap serial target
CELLS = [(name, t) for name in SMALL for t in TARGETS if not (t == "taps64" and name in ("long", "whole-chunk"))]
LANES_REFILTER = D.TRANSCODE_FORM_LANES | D.TRANSCODE_FORM_REFILTER


def fast_pair(src, dst):
    return (src is None or (len(src) <= 4 and src[0] in (1, -1))) and len(dst) <= 4


def form_of(src, dst, forced_serial=False):
    return LANES_REFILTER | (0 if fast_pair(src, dst) and not forced_serial else D.TRANSCODE_FORM_REFILTER_SERIAL)


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def small(ctx, O):
    """name -> (Stream, its samples): every SMALL batch encoded by the oracle once, shared by the cells"""
    made = {}

    def get(name):
        if name not in made:
            Ns, Ls, m, taps, sigma = SMALL[name]
            x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
            made[name] = (Stream(ctx, O, x, Ns, Ls, m, taps), x)
        return made[name]

    yield get
    for st, _ in made.values():
        st.plan.close()


def check(ctx, st, src, taps2, want, m2, sidebands=(False, True), decodes_to=None, what=""):
    t = None
    for sideband in sidebands:
        t = st.plan.refilter(st.enc, taps2, rice_m=m2, wave_words=st.table if sideband else None)
        cell = (what, taps2[:5], m2, sideband)
        assert st.plan.last_decode_path() == D.PATH_TRANSCODE, cell
        assert st.plan.last_transcode_form() == form_of(src, taps2), (cell, st.plan.last_transcode_form())
        assert t.rice_m == m2 and t.taps == (None if tuple(taps2) == (1, -1) else tuple(taps2)), cell
        same_stream(t, want, cell)
    if decodes_to is not None:
        p2 = t.plan(ctx)
        try:
            assert torch.equal(p2.decode(t.enc), decodes_to), (what, taps2[:5], m2, "decode of the result")
        finally:
            p2.close()


# --------------------------------------------------------------------------- 1. every small batch, seven targets
@pytest.mark.parametrize("name,target", CELLS)
def test_refilter_every_batch(ctx, O, small, name, target):
    Ns, Ls, m, taps, sigma = SMALL[name]
    assert not taps or taps[0] in (1, -1)  # (the source decodes to the samples: y = x)
    st, x = small(name)
    taps2 = TARGETS[target]
    whole = [L if L > 0 else 0xFFFFFFFF for L in Ls]  # (the whole chunk, spelt so that taps can follow it in the options)
    for m2 in (1, 8, 32768):
        check(ctx, st, taps, taps2, Want(O, x, Ns, whole, m2, taps2), m2, decodes_to=st.xd if m2 == 8 else None, what=name)
    assert not st.plan.last_transcode_form() & D.TRANSCODE_FORM_BLOCKS


# --------------------------------------------------------------------------- 2. both pairs of kernels on the same inputs
def test_refilter_serial_kernels_on_a_fast_pair(ctx, O):
    Ns, Ls = EDGE
    x = np.random.default_rng(2).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, FIR4)
    plan = st.plan
    try:
        for m2 in (1, 16):
            want = Want(O, x, Ns, Ls, m2, FIR4B)
            fast = plan.refilter(st.enc, FIR4B, rice_m=m2)
            assert plan.last_transcode_form() == LANES_REFILTER
            est_fast = plan.estimate_words_refiltered(st.enc, FIR4B)
            assert plan.last_transcode_form() == LANES_REFILTER
            ctx.set_option("debug_flags", D.DBG_REFILTER_SERIAL)
            serial = plan.refilter(st.enc, FIR4B, rice_m=m2)
            assert plan.last_transcode_form() == LANES_REFILTER | D.TRANSCODE_FORM_REFILTER_SERIAL
            est_serial = plan.estimate_words_refiltered(st.enc, FIR4B)
            assert plan.last_transcode_form() == LANES_REFILTER | D.TRANSCODE_FORM_REFILTER_SERIAL
            ctx.set_option("debug_flags", 0)
            same_stream(fast, want, ("fast", m2))
            same_stream(serial, want, ("serial", m2))
            assert serial.enc.total_words == fast.enc.total_words and torch.equal(serial.enc.words, fast.enc.words)
            assert torch.equal(serial.enc.chunk_word_off, fast.enc.chunk_word_off) and torch.equal(serial.wave_words, fast.wave_words)
            assert est_fast.tolist() == est_serial.tolist() and int(est_fast[int(math.log2(m2))]) == want.total
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


# --------------------------------------------------------------------------- 3. edges of the lane kernels
def test_refilter_wavefront_edges(ctx, O):
    Ns, Ls = EDGE
    x = np.random.default_rng(3).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, FIR4)
    try:
        for m2 in (1, 8, 32768):
            check(ctx, st, FIR4, FIR4B, Want(O, x, Ns, Ls, m2, FIR4B), m2, decodes_to=st.xd, what="edges")
    finally:
        st.plan.close()


def test_refilter_short_waveforms(ctx, O):
    Ls = [1, 2, 3, 4, 15, 16, 17, 63, 64, 65]  # shorter than the history; the group boundaries of the reader
    Ns = [70 * L + L // 2 for L in Ls]  # 70 waveforms each, and a shorter last one where there is room for it
    x = np.random.default_rng(33).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, FIR4)
    try:
        for m2 in (1, 8, 32768):
            check(ctx, st, FIR4, FIR4B, Want(O, x, Ns, Ls, m2, FIR4B), m2, decodes_to=st.xd, what="short waveforms")
        check(ctx, st, FIR4, FIR5, Want(O, x, Ns, Ls, 8, FIR5), 8, decodes_to=st.xd, what="short waveforms, serial")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. arithmetic mod 2^16
SRC_A, DST_A = (-1, 3, -3, 1), (-1, 2147483647, -2147483648, 65537)  # (the target's taps only matter mod 2^16)


@pytest.mark.parametrize("data", ["uniform", "crafted"])
@pytest.mark.parametrize("m", [1, 32768])  # escapes all over; the wide canonical form from k = 13 on
def test_refilter_arithmetic(ctx, O, data, m):
    if data == "uniform":
        Ns, Ls = [67 * 1000 + 333], [1000]
        x = np.random.default_rng(4).integers(-32768, 32768, sum(Ns)).astype(np.int16)  # all of int16
    else:
        rows = crafted_rows(W=70, L=70000)
        Ns, Ls = [rows.size], [rows.shape[1]]
        x = rows.reshape(-1)
    st = Stream(ctx, O, x, Ns, Ls, m, SRC_A)
    try:
        y = O.decode_chunk(st.words, opts_of(m, Ls[0], SRC_A))
        assert y.tobytes() == x.tobytes()  # (a lead of -1 decodes exactly)
        for m2 in (1, 4096):
            check(ctx, st, SRC_A, DST_A, Want(O, y, Ns, Ls, m2, DST_A), m2, sidebands=(False,), decodes_to=st.xd if m2 == 1 else None,
                  what=(data, m))
    finally:
        st.plan.close()


def test_refilter_source_lead_not_one(ctx, O):
    """a source whose lead is not +-1 decodes with the reference's division towards zero: the serial kernels, and the result
    is the encode of THOSE samples"""
    Ns, Ls = [65 * 300 + 11], [300]
    x = np.random.default_rng(41).integers(-32768, 32768, sum(Ns)).astype(np.int16)  # (residuals that wrap: the division is not exact)
    for src in ((2, -1), (-3, 1, 1)):
        st = Stream(ctx, O, x, Ns, Ls, 8, src)
        try:
            y = O.decode_chunk(st.words, opts_of(8, 300, src))
            assert y.tobytes() != x.tobytes()  # (lossy: the division)
            yd = torch.from_numpy(y).to(ctx.device)
            assert torch.equal(st.plan.decode(st.enc), yd)
            for taps2 in ((1, -1), FIR4):
                check(ctx, st, src, taps2, Want(O, y, Ns, Ls, 16, taps2), 16, decodes_to=yd, what=("lead", src))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 5. identities
@pytest.mark.parametrize("src", [None, FIR4, FIR5], ids=["delta", "fir4", "fir5"])
def test_refilter_to_the_same_filter_is_transcode(ctx, O, src):
    Ns, Ls = EDGE
    x = np.random.default_rng(5).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, src)
    try:
        for m2 in (2, 8, 64):
            a = st.plan.transcode(st.enc, rice_m=m2)
            b = st.plan.refilter(st.enc, src or (1, -1), rice_m=m2)
            assert a.enc.total_words == b.enc.total_words and torch.equal(a.enc.words, b.enc.words), (src, m2)
            assert torch.equal(a.enc.chunk_word_off, b.enc.chunk_word_off) and torch.equal(a.wave_words, b.wave_words), (src, m2)
            assert a.taps == b.taps and a.rice_m == b.rice_m
    finally:
        st.plan.close()


@pytest.mark.parametrize("A,B", [(None, FIR4), (FIR4, FIR4B), (FIR4B, None), (FIR5, (1, -2, 1))], ids=["delta-fir4", "fir4-fir4b", "fir4b-delta", "fir5-fir3"])
def test_refilter_there_and_back(ctx, O, A, B):
    Ns, Ls = EDGE
    x = np.random.default_rng(55).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, A)
    p2 = None
    try:
        there = st.plan.refilter(st.enc, B or (1, -1), rice_m=32)
        same_stream(there, Want(O, x, Ns, Ls, 32, B), ("there", A, B))
        p2 = there.plan(ctx)
        back = p2.refilter(there.enc, A or (1, -1), rice_m=8, wave_words=there.wave_words)
        assert p2.last_transcode_form() == form_of(B, A or (1, -1))
        assert back.enc.total_words == st.enc.total_words and back.enc.to_numpy()[0].tobytes() == st.words.tobytes(), (A, B)
        assert torch.equal(back.wave_words, st.table) and back.taps == (tuple(A) if A else None)
    finally:
        st.plan.close()
        if p2 is not None:
            p2.close()


# --------------------------------------------------------------------------- 6. the estimate
@pytest.mark.parametrize("taps2", [FIR4, FIR5], ids=["fast", "serial"])
def test_estimate_words_refiltered(ctx, O, taps2):
    Ns, Ls = EDGE
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    fresh = ctx.plan(Ns, Ls, 8, taps2)
    try:
        want = [Want(O, x, Ns, Ls, 1 << k, taps2).total for k in range(16)]
        for sideband in (False, True):
            got = st.plan.estimate_words_refiltered(st.enc, taps2, wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_TRANSCODE and st.plan.last_transcode_form() == form_of(None, taps2)
            assert got.dtype == np.uint64 and got.tolist() == want, sideband
        assert fresh.estimate_words(st.xd).tolist() == want
        best = int(np.argmin(want))
        t = st.plan.refilter(st.enc, taps2)  # rice_m None: the smallest, on a tie the smaller
        assert t.rice_m == 1 << best and t.enc.total_words == want[best]
        same_stream(t, Want(O, x, Ns, Ls, 1 << best, taps2), "best")
    finally:
        st.plan.close()
        fresh.close()


# --------------------------------------------------------------------------- 7. verdicts and buffers
@pytest.mark.parametrize("taps2", [FIR4B, FIR5], ids=["fast", "serial"])
def test_refilter_placements_and_capacity(ctx, O, taps2):
    Ns, Ls = EDGE
    x = np.random.default_rng(7).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, FIR4)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    want = Want(O, x, Ns, Ls, 32, taps2)
    slack = 67
    try:
        for ib in (0, 4, 12):
            ww = window(total + slack, torch.int32, ib, fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            for ob in (0, 4, 8, 12):
                for fill in (FF, 0):
                    cell = (ib, ob, fill)
                    yw = window(want.total, torch.int32, ob, fill=fill, device=ctx.device)  # out_cap_words = the total
                    ow = window(len(Ns) + 1, torch.int64, 8 if ob & 4 else 0, fill=fill, device=ctx.device)
                    nw = window(W, torch.int32, ob, fill=fill, device=ctx.device)
                    assert ww.t.data_ptr() % 16 == ib and yw.t.data_ptr() % 16 == ob
                    got = run(ctx, plan, lambda: plan.refilter_async(ww.t, st.enc.chunk_word_off, taps2, 32, yw.t, total, None, ow.t, nw.t))
                    assert got == want.total and plan.last_decode_path() == D.PATH_TRANSCODE, cell
                    assert plan.last_transcode_form() == form_of(FIR4, taps2), cell
                    assert yw.t.cpu().numpy().view(np.uint32).tobytes() == want.words.tobytes(), cell
                    assert ow.t.cpu().numpy().view(np.uint64).tobytes() == want.offs.tobytes(), cell
                    assert nw.t.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes(), cell
                    assert yw.intact() and ow.intact() and nw.intact() and ww.intact(), cell
            assert bool((ww.t[total:] == FF).all()), ib
        # one word short: DRX_ERR_CAPACITY at finish, the total NEEDED reported, the whole window still holding its fill
        for fill in (FF, 0):
            yw = window(want.total - 1, torch.int32, 4, fill=fill, device=ctx.device)
            ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
            plan.refilter_async(st.enc.words, st.enc.chunk_word_off, taps2, 32, yw.t, total)
            n = C.c_uint64()
            assert ctx.lib.drx_plan_finish(plan._h, C.byref(n)) == 3 and n.value == want.total
            assert bool((yw.t == fill).all()) and yw.intact(), fill
        # the sizing call: both tables and nothing else
        ow = window(len(Ns) + 1, torch.int64, 8, fill=-1, device=ctx.device)
        nw = window(W, torch.int32, 4, fill=-1, device=ctx.device)
        got = run(ctx, plan, lambda: plan.refilter_async(st.enc.words, st.enc.chunk_word_off, taps2, 32, None, total, None, ow.t, nw.t))
        assert got == want.total
        assert ow.t.cpu().numpy().view(np.uint64).tobytes() == want.offs.tobytes() and ow.intact()
        assert nw.t.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes() and nw.intact()
        # arguments: DRX_ERR_ARG, nothing launched
        lib, w, off, o = ctx.lib, st.enc.words.data_ptr(), st.enc.chunk_word_off.data_ptr(), ow.t.data_ptr()
        n2, good = len(taps2), (C.c_int32 * 64)(*taps2)
        zero = (C.c_int32 * 4)(0, 1, -1, 1)
        est = (C.c_uint64 * 16)()
        assert lib.drx_transcode_filter(plan._h, w, total, off, 5, 0, good, None, 0, o, None) == 1    # no taps
        assert lib.drx_transcode_filter(plan._h, w, total, off, 5, 65, good, None, 0, o, None) == 1   # more than DRX_MAX_TAPS
        assert lib.drx_transcode_filter(plan._h, w, total, off, 5, n2, None, None, 0, o, None) == 1   # NULL taps
        assert lib.drx_transcode_filter(plan._h, w, total, off, 5, 4, zero, None, 0, o, None) == 1    # a lead of 0
        assert lib.drx_transcode_filter(plan._h, w, total, off, 16, n2, good, None, 0, o, None) == 1  # new_rice_k > 15
        assert lib.drx_transcode_filter(plan._h, None, total, off, 5, n2, good, None, 0, o, None) == 1
        assert lib.drx_transcode_filter(plan._h, w, total, None, 5, n2, good, None, 0, o, None) == 1
        assert lib.drx_transcode_filter(plan._h, w, total, off, 5, n2, good, None, 0, None, None) == 1
        assert lib.drx_transcode_filter(plan._h, w, total, off, 5, n2, good, None, 10, o, None) == 1  # a capacity and no buffer
        assert lib.drx_transcode_filter_with_wave_words(plan._h, w, total, off, None, 5, n2, good, None, 0, o, None) == 1
        assert lib.drx_estimate_words_encoded_filter(plan._h, w, total, off, None, 0, good, est) == 1
        assert lib.drx_estimate_words_encoded_filter(plan._h, w, total, off, None, 65, good, est) == 1
        assert lib.drx_estimate_words_encoded_filter(plan._h, w, total, off, None, n2, None, est) == 1
        assert lib.drx_estimate_words_encoded_filter(plan._h, w, total, off, None, 4, zero, est) == 1
        assert lib.drx_estimate_words_encoded_filter(plan._h, w, total, off, None, n2, good, None) == 1
        assert plan.finish() == want.total  # (the status word as the sizing call left it)
    finally:
        plan.close()


@pytest.mark.parametrize("taps2", [FIR4B, FIR5], ids=["fast", "serial"])
def test_refilter_corrupt_input(ctx, O, taps2):
    import deltarice_amd as dr
    Ns, Ls = EDGE
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, FIR4)
    plan, good = st.plan, st.enc
    want = Want(O, x, Ns, Ls, 32, taps2)
    words, offs = st.words, st.offs

    def header_at(c, i):  # word index of waveform i's header in chunk c
        at = int(offs[c]) + 1
        for _ in range(i):
            at += int(words[at]) + 1
        return at

    def batch_of(w, o=None, total=None):
        o = offs if o is None else o
        return dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), torch.from_numpy(np.asarray(o, np.int64)).to(ctx.device),
                               int(o[-1]) if total is None else total)

    cases = {}
    # a payload cut short by a word, the chain repaired: its codes no longer end in its last word
    h = header_at(1, 70)
    n = int(words[h])
    w = np.delete(words, h + n)
    w[h] = n - 1
    o = offs.copy()
    o[2:] -= 1
    cases["n_i shortened, chain repaired"] = batch_of(w, o)
    # a payload word zeroed: sixteen escapes' worth of zeros, the codes run past the payload's end
    h = header_at(0, 5)
    w = words.copy()
    w[h + 3] = 0
    cases["payload word zeroed"] = batch_of(w)
    cases["stream a word short"] = dr.EncodedBatch(good.words, good.chunk_word_off, good.total_words - 1)
    cap = plan.max_encoded_words
    try:
        for cname, enc in cases.items():
            for fill in (FF, 0):
                yw = window(cap, torch.int32, 4, fill=fill, device=ctx.device)
                with pytest.raises(dr.DeltaRiceError) as e:
                    run(ctx, plan, lambda: plan.refilter_async(enc.words, enc.chunk_word_off, taps2, 32, yw.t, enc.total_words))
                assert e.value.status == 4, cname
                assert bool((yw.t == fill).all()) and yw.intact(), (cname, fill)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.estimate_words_refiltered(enc, taps2)
            assert e.value.status == 4, cname
            same_stream(plan.refilter(good, taps2, rice_m=32), want, (cname, "the call after"))  # the plan stays usable
    finally:
        plan.close()


# --------------------------------------------------------------------------- 8. among the plan's other calls
def test_refilter_in_sequence_on_one_plan(ctx, O):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(10).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, FIR4)
    plan = st.plan
    try:
        ctx.set_option("profile", 1)
        out = torch.empty(plan.max_encoded_words, dtype=torch.int32, device=ctx.device)
        t = plan.refilter(st.enc, FIR4B, rice_m=64, out_words=out)
        assert plan.last_decode_path() == D.PATH_TRANSCODE and plan.last_transcode_form() == LANES_REFILTER
        ms = plan.last_timings()
        assert len(ms) == 4 and all(math.isfinite(v) and v >= 0 for v in ms) and ms[3] > 0, ms
        same_stream(t, Want(O, x, Ns, Ls, 64, FIR4B), "refilter")
        assert plan.wave_words().tobytes() == header_table(st.words, st.offs, Ns, Ls).tobytes()  # the SOURCE's n_i
        # the plan's own filter and RiceParameter are as they were: a re-code under ITS filter, statistics, the decode, an encode
        t2 = plan.transcode(st.enc, rice_m=64)
        assert plan.last_transcode_form() == D.TRANSCODE_FORM_LANES
        same_stream(t2, Want(O, x, Ns, Ls, 64, FIR4), "transcode")
        stats = plan.wave_stats(st.enc, head=100)
        assert plan.last_decode_path() == D.PATH_STATS
        assert stats.cpu().numpy().tobytes() == wave_stats_heads(x, Ns, Ls, [100])[0].tobytes()
        assert torch.equal(plan.decode(st.enc), st.xd) and plan.last_decode_path() != D.PATH_TRANSCODE
        enc = plan.encode(st.xd)
        assert enc.total_words == st.enc.total_words and torch.equal(enc.words[:enc.total_words], st.enc.words)
    finally:
        ctx.set_option("profile", 0)
        plan.close()


# --------------------------------------------------------------------------- 9. the optimiser over the stream
def test_optimise_encoded_is_optimise(ctx, O):
    from deltarice_amd.optimise import optimise, optimise_encoded
    W, L, rho = 20, 7000, 0.95
    rng = np.random.default_rng(9)
    e = rng.normal(0, 12, (W, L))
    a = np.empty((W, L))
    a[:, 0] = e[:, 0]
    for i in range(1, L):
        a[:, i] = rho * a[:, i - 1] + e[:, i]
    x = np.round(a).astype(np.int16).reshape(-1)
    st = Stream(ctx, O, x, [W * L], [L], 8)  # the delta filter's stream
    try:
        want = optimise(ctx, st.xd, W * L, L, taps=(1, -1, 1), search=1, max_steps=3)
        got = optimise_encoded(ctx, st.plan, st.enc, taps=(1, -1, 1), search=1, max_steps=3)
        assert (got["taps"], got["k"], got["m"], got["words"], got["steps"]) == (want["taps"], want["k"], want["m"], want["words"], want["steps"])
        assert got["bits_per_sample"] == want["bits_per_sample"]
        assert list(got["evaluated"]) == list(want["evaluated"])
        assert all(got["evaluated"][f].tolist() == want["evaluated"][f].tolist() for f in want["evaluated"])
        side = optimise_encoded(ctx, st.plan, st.enc, taps=(1, -1, 1), search=1, max_steps=3, wave_words=st.table)
        assert side["taps"] == want["taps"] and side["words"] == want["words"]
        assert optimise_encoded(ctx, st.plan, st.enc, max_steps=0)["taps"] == (1, -1)  # taps None: the plan's own filter
        t = st.plan.refilter(st.enc, got["taps"], got["m"])
        assert t.enc.total_words == got["words"]
        same_stream(t, Want(O, x, [W * L], [L], got["m"], got["taps"]), "the optimum")
    finally:
        st.plan.close()
