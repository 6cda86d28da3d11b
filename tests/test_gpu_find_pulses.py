"""GPU: drx_find_pulses -- every run of samples over a per-waveform threshold, parsed from the encoded stream.

The streams are the oracle's (oracle.encode_chunk), the expected counts and records numpy's over the oracle's input
(tests/find_pulses_reference.py; for a filter whose lead is not +-1, over the oracle's decode of that stream), the comparison
torch.equal on the counts and on the whole record tensor, zero slots included.  Every cell runs through the walk and through
the side-band and asserts DRX_PATH_PULSES alone and plan.finish() == 0."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from find_pulses_reference import find_pulses, runs_of
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, geometry, header_table  # noqa: F401  (Stream builds its side-band with header_table)
from test_gpu_wave_stats import FILTERS, samples_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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


def expected(st, y, thr, pol, mw, mp, tab=None):
    return find_pulses(y, st.Ns, st.Ls, thr, pol, mw, mp, tab, (st.start, st.length, st.chunk))


def check(ctx, st, y, cases, sidebands=(False, True), what="", wants=None):
    """Every (thr, polarity, min_width, max_pulses, table or None) x {walk, side-band} on st against numpy over the samples y."""
    for i, (thr, pol, mw, mp, tab) in enumerate(cases):
        n, p = wants[i] if wants is not None else expected(st, y, thr, pol, mw, mp, tab)
        n, p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
        assert n.shape == (st.plan.total_waves,) and p.shape == (st.plan.total_waves, mp, D.PULSE_COLS)
        td = None if tab is None else torch.from_numpy(np.asarray(tab, np.int64)).to(ctx.device)
        for sideband in sidebands:
            cell = (what, thr, pol, mw, mp, "per-lane" if tab is not None else "", sideband)
            gn, gp = st.plan.find_pulses(st.enc, thr if td is None else td, pol, mw, mp, offset=0 if td is None else thr,
                                         wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_PULSES and st.plan.finish() == 0, cell
            assert gn.dtype == torch.int32 and gn.shape == n.shape and gp.dtype == torch.int64 and gp.shape == p.shape, cell
            if not torch.equal(gn, n):
                g = int(torch.nonzero(gn != n).flatten()[0])
                raise AssertionError((cell, f"{int((gn != n).sum())} counts differ; waveform {g}", int(gn[g]), int(n[g])))
            if not torch.equal(gp, p):
                bad = torch.nonzero((gp != p).flatten(1).any(dim=1)).flatten()
                g = int(bad[0])
                raise AssertionError((cell, f"{bad.numel()} rows differ; waveform {g}, count {int(n[g])}", gp[g].tolist(), p[g].tolist()))


# --------------------------------------------------------------------------- 1. every batch of the route table
@pytest.mark.parametrize("name", list(BATCHES))
def test_pulses_every_batch(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        check(ctx, st, samples_of(O, st, x, m, taps), [(2 * sigma, 1, 1, 3, None), (-2 * sigma, -1, 1, 3, None)], what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. group and round edges
EDGE_NS, EDGE_LS = [130 * 200 + 37] * 3, [200] * 3  # 131 waveforms per chunk: lanes in two chunks, the last waveform of 37 samples


def test_pulses_noise_on_the_edge_geometry(ctx, O):
    x = np.random.default_rng(2).normal(0, 10, sum(EDGE_NS)).astype(np.int16)
    st = Stream(ctx, O, x, EDGE_NS, EDGE_LS, 8)
    try:
        cases = [(20, 1, 1, 3, None), (-20, -1, 1, 3, None)]
        wants = [expected(st, x, *c) for c in cases]
        for (thr, pol, _, mp, _), (n, p) in zip(cases, wants):
            g, s, e, _ = runs_of(x, st.Ns, st.Ls, thr, pol)
            print(f"threshold {thr}: {int((n == 0).sum())} empty rows, {int((n > mp).sum())} overflowing, largest count {int(n.max())}")
            assert (n == 0).any() and (n > mp).any() and ((s == 0) | (e == st.length[g])).any()
        check(ctx, st, x, cases, what="edge noise", wants=wants)
    finally:
        st.plan.close()


def planted():
    """Runs on a floor of zeros, one waveform each: -> (samples, {what: waveform}).  Chunk 2 is chunk 0 negated."""
    first, length, _ = geometry(EDGE_NS, EDGE_LS)
    x = np.zeros(sum(EDGE_NS), np.int16)
    rng = np.random.default_rng(21)
    g, where = 0, {}

    def plant(what, s, w, values=None):
        nonlocal g
        v = rng.integers(30, 3000, w) if values is None else values
        x[first[g] + s:first[g] + s + w] = v
        where.setdefault(what, g)

    for s in (0, 1, 15, 16, 17, 63, 64, 65):
        for w in (1, 2, 15, 16, 17, 33):
            plant((s, w), s, w)
            g += 1
    plant("to the last sample", 190, 10)
    g += 1
    plant("end to end", 0, 200, np.full(200, 50))
    g += 1
    plant("one sample apart", 10, 3)
    plant("one sample apart", 14, 2)
    g += 1
    plant("plateau", 40, 4, [30, 80, 80, 30])
    g += 1
    plant("three wide runs", 5, 20)
    plant("three wide runs", 60, 1)
    plant("three wide runs", 100, 18)
    plant("three wide runs", 150, 2)
    plant("three wide runs", 170, 30)
    g = 130  # the 37-sample waveform
    assert length[g] == 37
    plant("to the last sample of the short waveform", 30, 7)
    assert g < 131
    n0 = EDGE_NS[0]
    x[2 * n0:3 * n0] = -x[:n0]
    return x, where


def test_pulses_planted_runs(ctx, O):
    x, where = planted()
    st = Stream(ctx, O, x, EDGE_NS, EDGE_LS, 8)
    try:
        n, p = expected(st, x, 20, 1, 1, 3)
        assert n[where[(16, 17)]] == 1 and p[where[(16, 17)], 0, :2].tolist() == [16, 17]
        assert p[where["to the last sample"], 0, :2].tolist() == [190, 10] and p[130, 0, :2].tolist() == [30, 7]
        assert p[where["end to end"], 0].tolist() == [0, 200, 50, 0, 10000] and n[where["one sample apart"]] == 2
        assert p[where["plateau"], 0].tolist() == [40, 4, 80, 41, 220] and n[where["three wide runs"]] == 5
        n, p = expected(st, x, -20, -1, 1, 3)
        assert n[:262].sum() == 0 and p[262 + where["plateau"], 0].tolist() == [40, 4, -80, 41, -220]
        cases = [(thr, pol, mw, mp, None) for thr, pol in ((20, 1), (-20, -1)) for mw in (1, 2, 3, 17) for mp in (0, 1, 3)]
        check(ctx, st, x, cases, what="planted")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 3. wide runs
def ar1(rng, rows, n, phi=0.95, sigma=5.0):
    """x[i] = phi x[i - 1] + N(0, sigma), every row started anew"""
    e = rng.normal(0, sigma, (rows, n))
    x = np.empty((rows, n))
    acc = np.zeros(rows)
    for i in range(n):
        acc = phi * acc + e[:, i]
        x[:, i] = acc
    return x


def test_pulses_wide_runs(ctx, O):
    rng = np.random.default_rng(31)
    rows = ar1(rng, 393, 200).astype(np.int16)
    x = np.concatenate([np.concatenate([rows[c * 131:c * 131 + 130].reshape(-1), rows[c * 131 + 130, :37]]) for c in range(3)])
    assert x.size == sum(EDGE_NS)
    st = Stream(ctx, O, x, EDGE_NS, EDGE_LS, 8)
    try:
        thr = int(round(5.0 / np.sqrt(1 - 0.95 ** 2)))  # 1 sigma of the series: 16
        g, s, e, _ = runs_of(x, st.Ns, st.Ls, thr, 1)
        widths = (1, 4, 16, 40)
        for mw in widths:
            assert mw == 1 or (e - s < mw).any(), mw
            assert (e - s > mw).any(), mw
        assert (s // 64 != (e - 1) // 64).any()  # a run that crosses a 64-sample round
        print(f"AR(1) at threshold {thr}: {g.size} runs, the longest {int((e - s).max())}, {int((s // 64 != (e - 1) // 64).sum())} cross a round")
        check(ctx, st, x, [(thr, 1, mw, 3, None) for mw in widths] + [(-thr, -1, 16, 2, None)], what="AR(1)")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. refills
def test_pulses_refills(ctx, O):
    Ns, Ls = [130 * 7000] * 2, [7000] * 2
    x = np.random.default_rng(3).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        cases = [(20, 1, 1, 4, None), (35, 1, 1, 4, None), (45, 1, 1, 4, None), (20, 1, 1, 0, None), (35, 1, 1, 0, None)]
        wants = [expected(st, x, *c) for c in cases]
        n20, n35, n45 = wants[0][0], wants[1][0], wants[2][0]
        assert n20.min() == 97 and n20.max() == 150  # every row overflows
        assert int((n35 == 0).sum()) == 80 and n35.max() <= 4 and int((n45 == 0).sum()) == 258
        check(ctx, st, x, cases, what="7000", wants=wants)
        ctx.set_option("profile", 1)
        try:
            st.plan.find_pulses(st.enc, 35)
            print(f"find_pulses of 260 x 7000 at threshold 35: walk / kernel / - / call ms = {st.plan.last_timings()}")
        finally:
            ctx.set_option("profile", 0)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 5. escapes and other parameters
@pytest.mark.parametrize("m,sigma", [(8, 3000), (1, 10), (64, 10), (32768, 10)])
def test_pulses_rice_parameters_and_escapes(ctx, O, m, sigma):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(m + sigma).normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m)
    try:
        check(ctx, st, x, [(2 * sigma, 1, 1, 3, None), (-sigma, -1, 2, 3, None)], what=(m, sigma))
    finally:
        st.plan.close()


def test_pulses_thresholds_at_the_ends(ctx, O):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    rng = np.random.default_rng(5)
    x = rng.normal(0, 3000, sum(Ns)).astype(np.int16)
    x[rng.integers(0, x.size, 40)] = -32768
    x[rng.integers(0, x.size, 40)] = 32767
    x[300:600] = 32767
    x[900:1200] = -32768  # (waveforms 1 and 3)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    W = st.plan.total_waves
    try:
        ends = (-32768, -32769, 32767, 32766, 32768)
        n = expected(st, x, -32768, -1, 1, 2)[0]
        assert n.sum() == 0  # nothing lies below -32768 ...
        n = expected(st, x, 32767, -1, 1, 2)[0]
        assert n[1] == 0 and n[3] == 1 and n.max() > 1  # ... and 32767 does not lie below 32767
        check(ctx, st, x, [(t, pol, 1, 2, None) for pol in (-1, 1) for t in ends], what="ends")
        # the int64 extremes for thr, with a column of the opposite extreme (t = -1) or of the same (saturated) in every other row
        for thr in (I64_MAX, I64_MIN):
            tab = np.where(np.arange(W) & 1, thr, -1 - thr).astype(np.int64)  # (-1 - max == min)
            for pol in (1, -1):
                n = expected(st, x, thr, pol, 1, 2, tab)[0]
                assert (n[0::2] > 0).all() and ((n[1::2] == 0).all() or (n[1::2] == 1).all())
            check(ctx, st, x, [(thr, 1, 1, 2, tab), (thr, -1, 1, 2, tab)], what=("int64 ends", thr))
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 6. per-lane thresholds
def test_pulses_per_lane_thresholds(ctx, O):
    x = np.random.default_rng(6).normal(0, 10, sum(EDGE_NS)).astype(np.int16)
    first, length, _ = geometry(EDGE_NS, EDGE_LS)
    x = (x + np.repeat(np.random.default_rng(66).integers(-500, 500, first.size), length)).astype(np.int16)  # a baseline per waveform
    st = Stream(ctx, O, x, EDGE_NS, EDGE_LS, 8)
    plan, W, head = st.plan, st.plan.total_waves, 30
    try:
        stats = plan.wave_stats(st.enc, head=head)
        tab8 = torch.full((W, D.STAT_COLS), 0x5A5A, dtype=torch.int64, device=ctx.device)
        tab8[:, D.STAT_HEAD_SUM] = stats[:, D.STAT_HEAD_SUM] // head + 25  # on the device: no host round trip
        col = tab8[:, D.STAT_HEAD_SUM]
        assert col.stride(0) == D.STAT_COLS and not col.is_contiguous()
        tab = col.cpu().numpy()
        assert np.unique(tab).size > 100
        n, p = expected(st, x, 0, 1, 1, 3, tab)
        assert (n == 0).any() and (n > 0).any()
        want_n, want_p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
        n5, p5 = expected(st, x, -5, 1, 1, 3, tab)
        for given in (col, col.contiguous()):
            for sideband in (False, True):
                gn, gp = plan.find_pulses(st.enc, given, 1, 1, 3, wave_words=st.table if sideband else None)
                assert plan.last_decode_path() == D.PATH_PULSES and plan.finish() == 0
                assert torch.equal(gn, want_n) and torch.equal(gp, want_p), (given.stride(0), sideband)
                gn, gp = plan.find_pulses(st.enc, given, 1, 1, 3, offset=-5, wave_words=st.table if sideband else None)
                assert torch.equal(gn.cpu(), torch.from_numpy(n5)) and torch.equal(gp.cpu(), torch.from_numpy(p5)), (given.stride(0), sideband)
        assert bool((tab8[:, :D.STAT_HEAD_SUM] == 0x5A5A).all())  # (the tensor the column lies in was not written)
    finally:
        plan.close()
    # W == 1
    x = np.array([0, 9, 9, 0, 0, 7, 0], np.int16)
    st = Stream(ctx, O, x, [7], [0], 8)
    try:
        check(ctx, st, x, [(1, 1, 1, 2, np.array([3])), (0, -1, 1, 2, np.array([1])), (3, 1, 1, 1, None)], what="one waveform")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. general filters
@pytest.mark.parametrize("fname", list(FILTERS))
def test_pulses_filters(ctx, O, fname):
    taps = FILTERS[fname]
    Ns, Ls = EDGE_NS[:1], EDGE_LS[:1]
    x = np.random.default_rng(len(taps)).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        y = samples_of(O, st, x, 8, taps)
        sd = int(round(float(np.std(y.astype(np.float64)))))  # (a lead that divides changes the scale of what the stream decodes to)
        check(ctx, st, y, [(2 * sd, 1, 1, 3, None), (-2 * sd, -1, 1, 3, None), (sd, 1, 2, 3, None), (sd, 1, 1, 0, None)], what=fname)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 8. a long waveform
def test_pulses_long_waveform(ctx, O):
    L = 200000
    rng = np.random.default_rng(8)
    phi = 0.95 ** np.arange(400)  # (0.95^400 < 2e-9: the AR(1) series as a convolution)
    x = np.concatenate([np.convolve(rng.normal(0, 5, L + 399), phi, mode="valid") for _ in range(2)]).astype(np.int16)
    assert x.size == 2 * L
    st = Stream(ctx, O, x, [L, L], [0, 0], 8)
    try:
        cases = [(30, 1, 4, 1024, None), (-30, -1, 4, 1024, None), (30, 1, 1, 1024, None)]  # (1.9 sigma of the series)
        wants = [expected(st, x, *c) for c in cases]
        for (_, _, mw, _, _), (n, _) in zip(cases, wants):
            print(f"two waveforms of {L} samples: {n.tolist()} pulses of at least {mw} samples")
            assert n.min() > 256
        assert wants[0][0].max() < 1024 < wants[2][0].min()  # every record of a row, and a row that overflows 1024 slots
        check(ctx, st, x, cases, what="long", wants=wants)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 9. where the buffers lie
def test_pulses_placements(ctx, O):
    rng = np.random.default_rng(9)
    x = rng.normal(0, 10, sum(EDGE_NS)).astype(np.int16)
    st = Stream(ctx, O, x, EDGE_NS, EDGE_LS, 8)
    plan, total, W, mp = st.plan, st.enc.total_words, st.plan.total_waves, 3
    try:
        tab = rng.integers(15, 26, W)
        n, p = expected(st, x, 0, 1, 1, mp, tab)
        assert (n == 0).any() and (n > mp).any()
        want_n, want_p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
        tw = window(W, torch.int64, 8, device=ctx.device)  # d_thr at an odd 8-byte position
        tw.t.copy_(torch.from_numpy(tab).to(ctx.device))
        assert tw.t.data_ptr() % 16 == 8
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)  # junk behind the stream
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(EDGE_NS) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            for cbyte, obyte in ((4, 8), (12, 8), (0, 0), (4, 0)):
                for fill in (0, -1):
                    cw = window(W, torch.int32, cbyte, fill=fill, device=ctx.device)
                    yw = window(W * mp * D.PULSE_COLS, torch.int64, obyte, fill=fill, device=ctx.device)
                    assert cw.t.data_ptr() % 16 == cbyte and yw.t.data_ptr() % 16 == obyte
                    for sideband in (False, True):
                        cw.t.fill_(fill)
                        yw.t.fill_(fill)
                        got = []
                        run(ctx, plan, lambda: got.append(plan.find_pulses_async(ww.t, ow.t, tw.t, 1, 1, mp, count=cw.t, out=yw.t, in_words=total,
                                                                                 wave_words=st.table if sideband else None)))
                        assert plan.last_decode_path() == D.PATH_PULSES
                        gn, gp = got[0]
                        assert gn.data_ptr() == cw.t.data_ptr() and gp.data_ptr() == yw.t.data_ptr()
                        same = torch.equal(gn, want_n) and torch.equal(gp, want_p)
                        intact = cw.intact() and yw.intact() and ow.intact() and ww.intact() and tw.intact()
                        assert same and intact, (pname, cbyte, obyte, fill, sideband, "results differ" * (not same), "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
        assert torch.equal(tw.t.cpu(), torch.from_numpy(tab))
    finally:
        plan.close()


# --------------------------------------------------------------------------- 10. verdicts
def test_pulses_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [65 * 300] * 2, [300] * 2
    rng = np.random.default_rng(10)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    other = Stream(ctx, O, np.roll(x, 4321), Ns, Ls, 8)
    plan, good = st.plan, st.enc
    n, p = expected(st, x, 20, 1, 1, 3)
    want_n, want_p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)

    def clean(**kw):
        gn, gp = plan.find_pulses(good, 20, 1, 1, 3, **kw)
        assert torch.equal(gn, want_n) and torch.equal(gp, want_p) and plan.last_decode_path() == D.PATH_PULSES and plan.finish() == 0

    try:
        clean()
        # a payload whose last word is cut off, its header word reduced by one and the chunk's words closed up
        g, at = 7, 1
        for _ in range(g):
            at += int(st.words[at]) + 1
        nw = int(st.words[at])
        cut = np.concatenate([st.words[:at], [np.uint32(nw - 1)], st.words[at + 1:at + nw], st.words[at + 1 + nw:]]).astype(np.uint32)
        offs = st.offs.copy()
        offs[1:] -= 1
        short = dr.EncodedBatch(torch.from_numpy(cut.view(np.int32)).to(ctx.device), torch.from_numpy(offs).to(ctx.device), int(offs[-1]))
        table = st.table.clone()
        table[g] = nw - 1
        assert not torch.equal(other.table, st.table)
        for cname, enc, kw in (("payload", short, {}), ("payload, side-band", short, dict(wave_words=table)),
                               ("another stream's side-band", good, dict(wave_words=other.table))):
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.find_pulses(enc, 20, 1, 1, 3, **kw)
            assert e.value.status == 4, cname
            clean()  # the plan stays usable, and its next call starts clean
            clean(wave_words=st.table)
        # DRX_ERR_ARG, nothing launched: the status word keeps the verdict of the call before
        W = plan.total_waves
        cnt = torch.zeros(W, dtype=torch.int32, device=ctx.device)
        out = torch.zeros(W * 3 * D.PULSE_COLS, dtype=torch.int64, device=ctx.device)
        thr = torch.zeros(W, dtype=torch.int64, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.find_pulses_async(short.words, short.chunk_word_off, 20, count=cnt, out=out, max_pulses=3, in_words=short.total_words)
        lib, w, off, h, tw = ctx.lib, good.words.data_ptr(), good.chunk_word_off.data_ptr(), plan._h, good.total_words
        c, o, t = cnt.data_ptr(), out.data_ptr(), thr.data_ptr()
        assert lib.drx_find_pulses(h, None, tw, off, t, 1, 0, 1, 1, 3, c, o) == 1
        assert lib.drx_find_pulses(h, w, tw, None, t, 1, 0, 1, 1, 3, c, o) == 1
        assert lib.drx_find_pulses(h, w, tw, off, t, 1, 0, 1, 1, 3, None, o) == 1
        assert lib.drx_find_pulses(h, w, tw, off, t, 1, 0, 1, 1, 3, c, None) == 1
        assert lib.drx_find_pulses(h, w, tw, off, t, 1, 0, 0, 1, 3, c, o) == 1  # polarity 0
        assert lib.drx_find_pulses(h, w, tw, off, t, 1, 0, 1, 0, 3, c, o) == 1  # min_width 0
        assert lib.drx_find_pulses(h, w, tw, off, t, 0, 0, 1, 1, 3, c, o) == 1  # thr_stride 0 with a table
        assert lib.drx_find_pulses_with_wave_words(h, w, tw, off, None, t, 1, 0, 1, 1, 3, c, o) == 1
        assert lib.drx_find_pulses_with_wave_words(h, w, tw, off, lib.drx_plan_wave_words(h), t, 1, 0, 1, 1, 3, c, o) == 1
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.finish()
        assert e.value.status == 4
        clean()
        # the counting form takes no output; thr_stride 0 is fine without a table
        assert lib.drx_find_pulses(h, w, tw, off, None, 0, 20, 1, 1, 0, c, None) == 0 and plan.finish() == 0
        torch.cuda.synchronize()
        assert torch.equal(cnt, want_n)
        # a decode behind a pulse call reports its own path
        assert torch.equal(plan.decode(good), st.xd) and plan.last_decode_path() not in (0, D.PATH_PULSES)
        clean()
    finally:
        plan.close()
        other.plan.close()


def test_pulses_among_other_calls(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [30 * 7000] * 4, [7000] * 4
    rng = np.random.default_rng(12)
    xa = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    xb = rng.normal(0, 60, sum(Ns)).astype(np.int16)  # louder: other code lengths, other header positions
    a, b = Stream(ctx, O, xa, Ns, Ls, 8), Stream(ctx, O, xb, Ns, Ls, 8)
    plan = a.plan
    try:
        # between a gather's sizing call and its copy call: the copy must not resume from tables this call rewrote
        sel, cw = rng.permutation(120)[:70], 10
        ref = plan.gather_encoded(a.enc, sel, cw)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        _, off, tab = plan.gather_encoded_async(a.enc.words, a.enc.chunk_word_off, sel, cw, None, a.enc.total_words)
        total = plan.finish()
        assert total == ref.enc.total_words
        nb, pb = expected(b, xb, 120, 1, 1, 3)
        gn, gp = plan.find_pulses(b.enc, 120, 1, 1, 3)  # b's header positions are in the plan's tables now
        assert torch.equal(gn.cpu(), torch.from_numpy(nb)) and torch.equal(gp.cpu(), torch.from_numpy(pb)) and plan.last_decode_path() == D.PATH_PULSES
        out = torch.full((total + 16,), FF, dtype=torch.int32, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        _, off, tab = plan.gather_encoded_async(a.enc.words, a.enc.chunk_word_off, sel, cw, out, a.enc.total_words, None, off, tab)
        assert plan.finish() == total and torch.equal(out[:total], ref.enc.words[:total]) and bool((out[total:] == FF).all())
        assert torch.equal(off, ref.enc.chunk_word_off) and torch.equal(tab, ref.wave_words)
        # another plan of the same context keeps its pending verdict
        broken = b.words.copy()
        broken[int(b.offs[1]) + 1] += 1  # the first waveform header of chunk 1: a broken chain
        bad = torch.from_numpy(broken.view(np.int32)).to(ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        b.plan.find_pulses_async(bad, b.enc.chunk_word_off, 120, in_words=b.enc.total_words)
        na, pa = expected(a, xa, 20, 1, 1, 3)
        gn, gp = plan.find_pulses(a.enc, 20, 1, 1, 3)
        assert plan.finish() == 0 and torch.equal(gn.cpu(), torch.from_numpy(na)) and torch.equal(gp.cpu(), torch.from_numpy(pa))
        with pytest.raises(dr.DeltaRiceError) as e:
            b.plan.finish()
        assert e.value.status == 4
        gn, gp = b.plan.find_pulses(b.enc, 120, 1, 1, 3)
        assert b.plan.finish() == 0 and torch.equal(gn.cpu(), torch.from_numpy(nb)) and torch.equal(gp.cpu(), torch.from_numpy(pb))
    finally:
        a.plan.close()
        b.plan.close()
