"""GPU: drx_find_pulses for few long waveforms -- a workgroup per block of a waveform's stream, the runs stitched across the
blocks' borders behind it (csrc/drx_pulses_blocks.hip, csrc/drx_pulse_runs.h).

The batches that drx_wave_stats gives to its block form take that form under the delta filter; drx_plan_last_pulses_form says
which form ran, drx_plan_last_decode_path keeps saying DRX_PATH_PULSES alone.  The streams are the oracle's, the expected counts
and records numpy's over the oracle's input (tests/find_pulses_reference.py), the comparison torch.equal on the counts and on
the whole record tensor, zero slots included, by the walk and by the side-band."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from find_pulses_reference import ARGPEAK, START, WIDTH, find_pulses, runs_of
from test_gpu_noise_levels import LEVELS, noise
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, header_table

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS, ALL = D.PULSES_FORM_LANES, D.PULSES_FORM_BLOCKS, D.PULSES_FORM_FALLBACK_ALL
CAP = D.PULSES_STAGE_CAP  # the records a block stages (DRX_PULSES_STAGE_CAP)


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


def expected(st, y, thr, pol, mw, mp, tab=None):
    return find_pulses(y, st.Ns, st.Ls, thr, pol, mw, mp, tab, (st.start, st.length, st.chunk))


def check(ctx, st, y, cases, form, what="", flags=0, sidebands=(False, True), wants=None, column=False):
    """Every (thr, polarity, min_width, max_pulses, table or None) x {walk, side-band} on st against numpy over the samples y, and
    the form of every call.  column: a table goes in as a column of an [W, 8] tensor (element stride 8), as a column of
    wave_stats' output would."""
    ctx.set_option("debug_flags", flags)
    try:
        for i, (thr, pol, mw, mp, tab) in enumerate(cases):
            n, p = wants[i] if wants is not None else expected(st, y, thr, pol, mw, mp, tab)
            n, p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
            td = None
            if tab is not None:
                td = torch.from_numpy(np.asarray(tab, np.int64)).to(ctx.device)
                if column:
                    wide = torch.full((td.numel(), 8), 12345, dtype=torch.int64, device=ctx.device)
                    wide[:, 3] = td
                    td = wide[:, 3]
                    assert td.stride(0) == 8
            for sideband in sidebands:
                cell = (what, flags, thr, pol, mw, mp, "per-lane" if tab is not None else "", sideband)
                gn, gp = st.plan.find_pulses(st.enc, thr if td is None else td, pol, mw, mp, offset=0 if td is None else thr,
                                             wave_words=st.table if sideband else None)
                assert st.plan.last_decode_path() == D.PATH_PULSES and st.plan.finish() == 0, cell
                assert st.plan.last_pulses_form() == form, (cell, st.plan.last_pulses_form())
                if not torch.equal(gn, n):
                    g = int(torch.nonzero(gn != n).flatten()[0])
                    raise AssertionError((cell, f"{int((gn != n).sum())} counts differ; waveform {g}", int(gn[g]), int(n[g])))
                if not torch.equal(gp, p):
                    bad = torch.nonzero((gp != p).flatten(1).any(dim=1)).flatten()
                    g = int(bad[0])
                    slot = int(torch.nonzero((gp[g] != p[g]).any(dim=1)).flatten()[0])
                    raise AssertionError((cell, f"{bad.numel()} rows differ; waveform {g}, count {int(n[g])}, slot {slot}", gp[g, slot].tolist(),
                                          p[g, slot].tolist()))
    finally:
        ctx.set_option("debug_flags", 0)


def stream_of(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    return Stream(ctx, O, x, Ns, Ls, m, taps), x, sigma


# --------------------------------------------------------------------------- 1. which batches take which form
@pytest.mark.parametrize("name,form", [("long-2", BLOCKS), ("long-40", BLOCKS), ("whole-chunk", BLOCKS),
                                       ("stream-quiet", LANES), ("short", LANES), ("fir4", LANES)])
def test_forms(ctx, O, name, form):
    st, x, sigma = stream_of(ctx, O, name)
    try:
        assert st.plan.last_pulses_form() == 0  # no pulse call yet
        y = x
        if BATCHES[name][3] is not None:  # (a filter whose lead is +-1: the samples come back as they went in)
            assert torch.equal(st.plan.decode(st.enc), st.xd)
        cases = [(3 * sigma, 1, 1, 4, None)] if name == "long-40" else [(3 * sigma, 1, 1, 4, None), (-2 * sigma, -1, 2, 0, None)]
        check(ctx, st, y, cases, form, what=name)
        if name == "long-2":
            one = cases[:1]
            check(ctx, st, y, one, LANES, what=name, flags=D.DBG_PULSES_LANES)
            check(ctx, st, y, one, LANES, what=name, flags=D.DBG_NO_LONG_PATHS)
            check(ctx, st, y, one, LANES, what=name, flags=D.DBG_LONG_NOT_BLOCKS)
            check(ctx, st, y, cases, BLOCKS | ALL, what=name, flags=D.DBG_PULSES_ALL_FALLBACK)
            check(ctx, st, y, one, BLOCKS, what=name, flags=D.DBG_STATS_LANES)  # (the statistics call's flag, not this call's)
            check(ctx, st, y, one, BLOCKS, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. stitching, crafted
L2 = 50000
RUN_D, PEAK_D = 10000, 10100  # row (d): where its run begins and where its peak first stands


def crafted():
    """Four rows of L2 samples on a floor of clipped noise (|y| <= 40), every run well above 100:
      0  (a) a run of width 1 at sample 0 and a run that ends at the last sample; (e) runs of width 30 every 37 samples over
         samples 20 000 .. 25 000, so that lane borders (a lane holds some tens of samples) cut many of them
      1  (b) every sample near 1000: one run of width L2 under any threshold below the row's minimum
      2  (c) a square wave of period 100, 50 over and 50 under, over the whole row
      3  (d) a run of 25 000 samples across several blocks (a block holds some 10 000), its peak value first 100 samples in and
         again 1, 50, 9 000 and 20 000 samples later"""
    rng = np.random.default_rng(52)
    x = np.clip(rng.normal(0, 10, (4, L2)), -40, 40).astype(np.int16)
    x[0, 0] += 500
    x[0, L2 - 7:] += 500
    for j in range(20000, 25000 - 30, 37):
        x[0, j:j + 30] += 400
    x[1] += 1000
    x[2] += np.where(np.arange(L2) % 100 < 50, 200, 0).astype(np.int16)
    x[3, RUN_D:RUN_D + 25000] += 300
    for d in (0, 1, 50, 9000, 20000):
        x[3, PEAK_D + d] = 1000
    return x


@pytest.mark.parametrize("pol", [1, -1])
def test_stitching_crafted(ctx, O, pol):
    x = crafted() * pol  # (mirrored: every value stays far inside the int16 range)
    flat = np.ascontiguousarray(x).reshape(-1)
    st = Stream(ctx, O, flat, [2 * L2] * 2, [L2] * 2, 8)
    thr = 100 * pol
    below_b = int(x[1].min()) - 1 if pol > 0 else int(x[1].max()) + 1
    tab = np.array([thr, below_b, thr, thr], np.int64)
    try:
        # what the rows were built for, from numpy
        n, p = expected(st, flat, thr, pol, 1, 600)
        n_e = len(range(20000, 25000 - 30, 37))
        assert n[0] == 2 + n_e and p[0, 0, :2].tolist() == [0, 1] and p[0, n[0] - 1, :2].tolist() == [L2 - 7, 7]
        assert n[1] == 1 and p[1, 0, :2].tolist() == [0, L2]
        assert n[2] == L2 // 100 and (p[2, :n[2], WIDTH] == 50).all()
        assert n[3] == 1 and p[3, 0, [START, WIDTH, ARGPEAK]].tolist() == [RUN_D, 25000, PEAK_D] and p[3, 0, 2] == 1000 * pol
        assert expected(st, flat, thr, pol, 50, 0)[0][2] == L2 // 100 and expected(st, flat, thr, pol, 51, 0)[0][2] == 0
        assert expected(st, flat, thr, pol, 30, 0)[0][0] == n_e and expected(st, flat, thr, pol, 31, 0)[0][0] == 0
        assert n[2] > CAP and n[0] > CAP and n[0] > 4 and n[1] <= 1  # counts on both sides of the staging cap and of max_pulses
        for mw in (1, 30, 31, 50, 51):
            cases = [(thr, pol, mw, mp, None) for mp in (0, 1, 4, 600)]
            check(ctx, st, flat, cases, BLOCKS, what=("crafted", mw))
            check(ctx, st, flat, [(0, pol, mw, mp, tab) for mp in (0, 4, 600)], BLOCKS, what=("crafted column", mw), column=True)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 3. the staging cap
def test_staging_cap(ctx, O):
    """max_pulses above the cap.  Waveform 0: a block holds more pulses than it stages and few lie in front of it -- exact,
    through the second launch of the blocks.  Waveform 1: as many pulses spread thinly over all blocks -- exact, from the
    staged records.  plan.last_pulses_redone() counts the waveforms that the second launch of the blocks finished: exactly
    waveform 0 where a block of it needs more than CAP records, none otherwise; none goes to the lane kernel."""
    rng = np.random.default_rng(53)
    L, mp = 120000, 3 * CAP
    x = np.clip(rng.normal(0, 10, (4, L)), -40, 40).astype(np.int16)
    x[0, 100:110] += 300                      # one pulse in front
    for j in range(40000, 40000 + 20 * 60, 60):  # twenty within 1200 samples: one or two blocks
        x[0, j:j + 5] += 300
    for j in range(2500, L, 5000):            # twenty-four, 5000 samples apart: at most three in a block of some 10 000
        x[1, j:j + 5] += 300
    x[2, 7::9000] += 300
    flat = x.reshape(-1)
    st = Stream(ctx, O, flat, [2 * L] * 2, [L] * 2, 8)
    try:
        n, _ = expected(st, flat, 100, 1, 1, mp)
        assert n[0] == 21 and n[1] == 24 and n[3] == 0, n
        check(ctx, st, flat, [(100, 1, 1, mp, None), (100, 1, 1, 0, None), (100, 1, 1, CAP, None), (100, 1, 1, CAP + 1, None), (100, 1, 5, mp, None),
                              (100, 1, 6, mp, None)], BLOCKS, what="staging cap")
        # which waveforms the second launch of the blocks finished, and that none went to the lane kernel: mp, min_width -> how many
        for mp_, mw, redone in [(mp, 1, 1), (0, 1, 0), (CAP, 1, 0), (CAP + 1, 1, 0), (mp, 5, 1), (mp, 6, 0)]:
            for sideband in (False, True):
                st.plan.find_pulses(st.enc, 100, 1, mw, mp_, wave_words=st.table if sideband else None)
                got = (st.plan.last_pulses_form(), st.plan.last_pulses_redone(), st.plan.last_pulses_listed())
                assert got == (BLOCKS, redone, 0), (mp_, mw, sideband, got)
        ctx.set_option("debug_flags", D.DBG_PULSES_ALL_FALLBACK)
        st.plan.find_pulses(st.enc, 100, 1, 1, 4)
        assert st.plan.last_pulses_listed() == st.plan.total_waves
        ctx.set_option("debug_flags", D.DBG_PULSES_LANES)
        st.plan.find_pulses(st.enc, 100, 1, 1, mp)
        assert st.plan.last_pulses_form() == LANES and st.plan.last_pulses_listed() == 0
        ctx.set_option("debug_flags", 0)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. the block geometries
def test_geometry_classes(ctx, O):
    """9 / 11 / 15 / 19 stream words per lane by the stream's bits per sample, and waveforms of one or two blocks (64 / 128
    lanes per block) in the outer classes; a threshold at 2 sigma of each level, so that every lane meets runs."""
    rng = np.random.default_rng(41)
    seen = set()
    for sigma, m in LEVELS:
        x = noise(rng, sigma, 2 * 3 * 90000)
        st = Stream(ctx, O, x, [3 * 90000] * 2, [90000] * 2, m)
        try:
            bits = st.words.size * 32.0 / x.size
            seen.add(9 if bits < 5.4 else 11 if bits < 8.2 else 15 if bits < 11.7 else 19)
            check(ctx, st, x, [(2 * sigma, 1, 1, 4, None), (-2 * sigma, -1, 2, 0, None)], BLOCKS, what=(sigma, m))
        finally:
            st.plan.close()
    assert seen == {9, 11, 15, 19}, seen
    for sigma, m, L in [(1, 8, 5000), (2000, 2048, 4000), (1, 8, 12000), (2000, 2048, 9000)]:
        N = 7 * L - L // 3
        x = noise(rng, sigma, 3 * N)
        st = Stream(ctx, O, x, [N] * 3, [L] * 3, m)
        try:
            check(ctx, st, x, [(2 * sigma, 1, 1, 4, None), (-2 * sigma, -1, 2, 3, None)], BLOCKS, what=(sigma, m, L))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 5. more codes on a lane than its share
def test_quiet_stretches_take_the_second_parse(ctx, O):
    rng = np.random.default_rng(42)
    x = noise(rng, 200, 2 * 2 * 120000).reshape(4, 120000)
    x[:, 30000:70000] = 0
    x[0, 40000:40020] = 3000  # inside the quiet stretch
    x[0, 50000] = 3000
    x[1, 29990:30015] = 3000  # astride its beginning
    x[1, 69990:70010] = 3000  # ... and its end
    x[2, 30000:70000] = 2500  # all of it
    x[3, 90000:90040] = 3000  # behind it
    x[3, 119990:] = 3000
    x = np.ascontiguousarray(x).reshape(-1)
    st = Stream(ctx, O, x, [2 * 120000] * 2, [120000] * 2, 256)
    try:
        n, p = expected(st, x, 2000, 1, 1, 4)
        assert n.tolist() == [2, 2, 1, 2] and p[2, 0, :2].tolist() == [30000, 40000] and p[1, :2, :2].tolist() == [[29990, 25], [69990, 20]]
        check(ctx, st, x, [(2000, 1, 1, 4, None), (2000, 1, 2, 4, None), (2000, 1, 21, 0, None), (-400, -1, 1, 4, None), (0, 1, 1, 2, None)], BLOCKS,
              what="quiet stretches")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 6. streams that do not fall into step
@pytest.mark.parametrize("case,thr", [("slope 1 sawtooth", 0), ("square wave", 0), ("alternating +-1", 7), ("ramp with noise stretches", 0)])
def test_equal_length_codes(ctx, O, case, thr):
    n = 3 * 300000
    i = np.arange(n)
    v = {
        "slope 1 sawtooth": (i % 60000 - 30000),
        "square wave": np.where((i // 50) % 2 == 0, 100, -100),
        "alternating +-1": np.where(i % 2 == 0, 7, 8),
        "ramp with noise stretches": np.where((i // 40000) % 3 == 0, np.random.default_rng(46).normal(0, 10, n), i % 60000 - 30000),
    }[case]
    x = np.ascontiguousarray(v).astype(np.int16)
    st = Stream(ctx, O, x, [300000] * 3, [100000] * 3, 8)
    try:
        _, s, e, _ = runs_of(x, st.Ns, st.Ls, thr, 1)
        if case == "slope 1 sawtooth":
            assert (e - s).max() == 29999 and (e - s >= 9999).all()  # runs of 30 000 samples, cut by the waveforms' ends
        if case == "alternating +-1":
            assert (e - s == 1).all() and s.size == n // 2  # a pulse every second sample
        check(ctx, st, x, [(thr, 1, 1, 4, None), (thr, 1, 1, 0, None), (thr, -1, 1, 4, None)], BLOCKS, what=case)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. a ragged plan of long waveforms
def test_ragged_long_batch(ctx, O):
    Ns, Ls = [2048 * 5 + 9, 30000 * 3, 150001, 9001 * 4 - 3000], [2048, 30000, 0, 9001]
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        assert torch.equal(st.plan.decode(st.enc), st.xd)
        assert st.plan.last_decode_path() & D.PATH_BLOCKS, st.plan.last_decode_path()  # (this shape: the block decoder's)
        cases = [(25, 1, 1, 4, None), (-20, -1, 2, 4, None), (30, 1, 1, 0, None), (15, 1, 1, 12, None)]
        check(ctx, st, x, cases, BLOCKS, what="ragged")
        check(ctx, st, x, cases[:2], BLOCKS | ALL, what="ragged", flags=D.DBG_PULSES_ALL_FALLBACK)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 8. where the buffers lie
def test_placements(ctx, O):
    st, x, sigma = stream_of(ctx, O, "long-2")
    plan, total, W, mp = st.plan, st.enc.total_words, st.plan.total_waves, 3
    tab = np.random.default_rng(58).integers(25, 55, W)  # 2.5 to 5.5 sigma: rows that overflow and rows without a pulse
    n, p = expected(st, x, 0, 1, 1, mp, tab)
    assert (n == 0).any() and (n > mp).any()
    want_n, want_p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
    tw = window(W, torch.int64, 8, device=ctx.device)  # d_thr at an odd 8-byte position
    tw.t.copy_(torch.from_numpy(tab).to(ctx.device))
    try:
        for pname, P in PLACEMENTS.items():  # the words at byte offsets 0, 4, 8 and 12
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(st.Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            for cbyte, obyte in ((4, 8), (12, 0)):  # d_count at 4 mod 8; d_out at 8 mod 16 and at 0
                for fill in (0x5A5A5A5A, -1):
                    cw = window(W, torch.int32, cbyte, fill=fill, device=ctx.device)
                    yw = window(W * mp * D.PULSE_COLS, torch.int64, obyte, fill=fill, device=ctx.device)
                    assert cw.t.data_ptr() % 8 == 4 and yw.t.data_ptr() % 16 == obyte
                    for sideband in (False, True):
                        cw.t.fill_(fill)
                        yw.t.fill_(fill)
                        got = []
                        run(ctx, plan, lambda: got.append(plan.find_pulses_async(ww.t, ow.t, tw.t, 1, 1, mp, count=cw.t, out=yw.t, in_words=total,
                                                                                 wave_words=st.table if sideband else None)))
                        assert plan.last_decode_path() == D.PATH_PULSES and plan.last_pulses_form() == BLOCKS
                        gn, gp = got[0]
                        same = torch.equal(gn, want_n) and torch.equal(gp, want_p)
                        intact = cw.intact() and yw.intact() and ow.intact() and ww.intact() and tw.intact()
                        assert same and intact, (pname, cbyte, obyte, fill, sideband, "results differ" * (not same), "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. verdicts
def test_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [3 * 40000], [40000]
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    n, p = expected(st, x, 30, 1, 1, 4)
    want_n, want_p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
    w = st.words
    h1 = 1 + 1 + int(w[1])  # the header of waveform 1: behind the chunk's word, waveform 0's header and its payload
    n1 = int(w[h1])

    def batch_of(words):
        off = torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device)
        return dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), off, int(words.size)), words

    def clean():
        gn, gp = plan.find_pulses(good, 30, 1, 1, 4)
        assert torch.equal(gn, want_n) and torch.equal(gp, want_p)
        assert plan.last_decode_path() == D.PATH_PULSES and plan.last_pulses_form() == BLOCKS

    # a header one smaller, the payload's last word taken out (the chain stays consistent: the codes run past the payload)
    short = np.delete(w, h1 + n1)
    short[h1] = n1 - 1
    # a payload whose codes end one word early: a word of padding more, counted in the header
    early = np.insert(w, h1 + 1 + n1, np.uint32(0))
    early[h1] = n1 + 1
    # a broken chain
    chain = w.copy()
    chain[h1] += 1
    try:
        clean()
        for cname, (enc, words) in {"header": batch_of(short), "payload": batch_of(early), "chain": batch_of(chain)}.items():
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.find_pulses(enc, 30, 1, 1, 4)
            assert e.value.status == 4, cname
            assert plan.last_pulses_form() == BLOCKS, cname
            clean()  # the plan stays usable, and its next call starts clean
            if cname != "chain":  # ... and by the side-band (the table that belongs to that stream)
                table = torch.from_numpy(header_table(words, np.array([0, words.size]), Ns, Ls).view(np.int32)).to(ctx.device)
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.find_pulses(enc, 30, 1, 1, 4, wave_words=table)
                assert e.value.status == 4, cname
                clean()
    finally:
        plan.close()


# --------------------------------------------------------------------------- 10. among the plan's other calls
def test_sequences_on_one_plan(ctx, O):
    from wave_stats_reference import wave_stats_heads
    st, x, sigma = stream_of(ctx, O, "long-2")
    plan = st.plan
    taps = (1, -1, 1, -1)
    fst = Stream(ctx, O, x, st.Ns, st.Ls, 8, taps)  # the same samples under another filter (its plan is not used)
    n, p = expected(st, x, 30, 1, 1, 4)
    want_n, want_p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
    want_s = torch.from_numpy(wave_stats_heads(x, st.Ns, st.Ls, [100])[0]).to(ctx.device)

    def pulses(enc, form, **kw):
        gn, gp = plan.find_pulses(enc, 30, 1, 1, 4, **kw)
        assert plan.last_decode_path() == D.PATH_PULSES and plan.last_pulses_form() == form and plan.finish() == 0
        assert torch.equal(gn, want_n) and torch.equal(gp, want_p)

    def stats(enc, form):
        assert torch.equal(plan.wave_stats(enc, head=100), want_s)
        assert plan.last_stats_form() == form

    try:
        pulses(st.enc, BLOCKS)
        assert torch.equal(plan.decode(st.enc), st.xd) and plan.last_decode_path() & D.PATH_BLOCKS  # (shares the block scratch)
        pulses(st.enc, BLOCKS)
        stats(st.enc, D.STATS_FORM_BLOCKS)
        pulses(st.enc, BLOCKS, wave_words=st.table)
        assert plan.last_stats_form() == D.STATS_FORM_BLOCKS  # (the last STATISTICS call's)
        st.check(np.array([0, 63, 17, 40]))
        pulses(st.enc, BLOCKS)
        gn, gp = plan.find_pulses(st.enc, 30, 1, 1, 3 * CAP)  # more staging than the plan has had so far
        en, ep = expected(st, x, 30, 1, 1, 3 * CAP)
        assert torch.equal(gn, torch.from_numpy(en).to(ctx.device)) and torch.equal(gp, torch.from_numpy(ep).to(ctx.device))
        stats(st.enc, D.STATS_FORM_BLOCKS)
        assert plan.last_pulses_form() == BLOCKS  # (the last PULSE call's)
        plan.set_filter(taps)
        pulses(fst.enc, LANES)
        stats(fst.enc, D.STATS_FORM_LANES)
        assert torch.equal(plan.decode(fst.enc), st.xd)
        assert plan.last_pulses_form() == LANES
        plan.set_filter(None)
        pulses(st.enc, BLOCKS)
        stats(st.enc, D.STATS_FORM_BLOCKS)
    finally:
        plan.close()
        fst.plan.close()
