"""GPU: the block forms of drx_wave_stats, drx_find_pulses, drx_decode_windows and drx_transcode / drx_estimate_words_encoded
at every RiceParameter, on every (lanes per block, stream words per lane) class, on data that the parameter does not suit, and
with a payload that ends on or next to a block's border.

The cells are tests/block_cells.py's (tests/test_block_cells_model.py proves on the CPU which class each one runs and which of
them need several staging passes).  The streams are the oracle's, the expected values numpy's over the oracle's input
(tests/wave_stats_reference.py, find_pulses_reference.py, decode_windows_reference.py) and, for the re-code, the oracle's encode
of the same samples at the target parameter; every comparison is exact, by the walk and by the side-band.  Every call asserts
its path and its form.  A block form leaves the waveforms it flags to the lane kernel behind it: on the matched cells with
k >= 1 the calls that report that list must report it empty -- the blocks did the work; on the other cells the count goes into
the failure message."""
import numpy as np
import pytest

import block_cells as bc
from decode_windows_reference import windows_multi
from deltarice_amd import _lib as D
from find_pulses_reference import START, find_pulses
from test_gpu_decode_windows import check as windows_check, dev, prefilled
from test_gpu_decode_windows_blocks import check_tiling, sorted_cases
from test_gpu_select import Stream
from test_gpu_transcode import Want, same_stream
from test_gpu_wave_stats_blocks import check as stats_check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BLOCKS, ALL, LANES = D.STATS_FORM_BLOCKS, D.STATS_FORM_FALLBACK_ALL, D.STATS_FORM_LANES
assert (D.PULSES_FORM_BLOCKS, D.PULSES_FORM_FALLBACK_ALL, D.PULSES_FORM_LANES) == (BLOCKS, ALL, LANES)
assert (D.WINDOWS_FORM_BLOCKS, D.WINDOWS_FORM_FALLBACK_ALL, D.WINDOWS_FORM_LANES) == (BLOCKS, ALL, LANES)
assert (D.TRANSCODE_FORM_BLOCKS, D.TRANSCODE_FORM_FALLBACK_ALL, D.TRANSCODE_FORM_LANES) == (BLOCKS, ALL, LANES)
TAPS = (1, -1, 1, -1)


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


class CellStream:
    """A cell's samples and their oracle stream on the device; what its listed counts must be."""

    def __init__(self, ctx, O, cell, taps=None):
        self.cell, self.x = cell, cell.x()
        self.st = Stream(ctx, O, self.x, cell.Ns, cell.Ls, cell.m, taps)
        self.taps = taps
        self.W = self.st.plan.total_waves
        self.blocks_alone = cell.kind == "matched" and cell.k >= 1
        self.seen = []  # listed counts of the calls so far, for the messages

    def listed(self, rule="blocks"):
        """The predicate over a call's listed count: every waveform under *_ALL_FALLBACK ("all"); none on the lane form
        ("lanes"); on the block form none on a matched cell with k >= 1, recorded otherwise."""
        def holds(n):
            self.seen.append(n)
            if rule == "all":
                return n == self.W
            if rule == "lanes" or self.blocks_alone:
                return n == 0
            return 0 <= n <= self.W
        return holds

    def close(self):
        self.st.plan.close()


@pytest.fixture(scope="module", params=bc.CELLS, ids=lambda c: c.id)
def cs(request, ctx, O):
    s = CellStream(ctx, O, request.param)
    yield s
    s.close()


def heads_of(n):
    return (0, 1, 100, n - 1, n, n + 1)


# --------------------------------------------------------------------------- the four calls
def two_sigma(c):
    """2 sigma of the cell's samples as a threshold: at least 1, and 30 000 where 2 sigma leaves the int16 range (k = 15)"""
    return min(max(1, int(round(2 * c.sigma))), 30000)


def pulse_cases(s):
    """(thr, polarity, min_width, max_pulses, per-waveform thresholds or None): +-2 sigma and a column of thresholds from half a
    sigma to three; both polarities, min_width 1 and 2, max_pulses 0, 3 and 64.  zeros: thresholds 0 and -1 (nothing over, and
    one run over the whole waveform)."""
    c = s.cell
    rng = np.random.default_rng(c.k + c.L)
    if c.kind == "zeros":
        tab = -(np.arange(s.W) % 2)
        return [(0, 1, 1, 3, None), (-1, 1, 2, 0, None), (-1, 1, 1, 64, None), (0, -1, 1, 64, None), (-1, -1, 2, 3, None),
                (0, 1, 1, 3, tab), (0, -1, 2, 64, tab)]
    T = two_sigma(c)
    tab = rng.integers(max(1, T // 4), 3 * T // 2 + 2, s.W)
    return [(T, 1, 1, 3, None), (-T, -1, 2, 0, None), (T, 1, 2, 64, None), (-T, -1, 1, 64, None), (0, 1, 1, 3, tab), (0, -1, 2, 64, -tab)]


def pulses_check(ctx, s, cases, form, flags=0, listed=None, what=""):
    st = s.st
    listed = listed or s.listed()
    ctx.set_option("debug_flags", flags)
    try:
        for thr, pol, mw, mp, tab in cases:
            n, p = find_pulses(s.x, st.Ns, st.Ls, thr, pol, mw, mp, tab, (st.start, st.length, st.chunk))
            n, p = torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)
            td = dev(ctx, tab, np.int64)
            for sideband in (False, True):
                gn, gp = st.plan.find_pulses(st.enc, thr if td is None else td, pol, mw, mp, offset=0 if td is None else thr,
                                             wave_words=st.table if sideband else None)
                k = st.plan.last_pulses_listed()
                call = (s.cell.id, what, flags, thr, pol, mw, mp, "column" if tab is not None else "", sideband, "listed", k)
                assert st.plan.last_decode_path() == D.PATH_PULSES and st.plan.finish() == 0, call
                assert st.plan.last_pulses_form() == form, (call, st.plan.last_pulses_form())
                assert listed(k), call
                if not torch.equal(gn, n):
                    g = int(torch.nonzero(gn != n).flatten()[0])
                    raise AssertionError((call, f"{int((gn != n).sum())} counts differ; waveform {g}", int(gn[g]), int(n[g])))
                if not torch.equal(gp, p):
                    g = int(torch.nonzero((gp != p).flatten(1).any(dim=1)).flatten()[0])
                    slot = int(torch.nonzero((gp[g] != p[g]).any(dim=1)).flatten()[0])
                    raise AssertionError((call, f"records differ; waveform {g}, count {int(n[g])}, slot {slot}", gp[g, slot].tolist(), p[g, slot].tolist()))
    finally:
        ctx.set_option("debug_flags", 0)


def windows(ctx, s, cases, form, flags=0, listed=None, what=""):
    """check() of test_gpu_decode_windows with the listed counts in its message"""
    try:
        return windows_check(ctx, s.st, s.x, cases, form, flags=flags, what=(s.cell.id, what), listed=listed or s.listed())
    except AssertionError as e:
        raise AssertionError((e.args, "listed", s.seen[-4:])) from e


def pulse_windows(ctx, s, form, flags=0, listed=None):
    """The samples around the cell's own pulses: the records and counts of find_pulses as they lie on the device"""
    st, c = s.st, s.cell
    thr = -1 if c.kind == "zeros" else two_sigma(c)
    n, p = find_pulses(s.x, st.Ns, st.Ls, thr, 1, 1, 8, None, (st.start, st.length, st.chunk))
    assert n.max() > 0, c
    gn, gp = st.plan.find_pulses(st.enc, thr, 1, 1, 8)
    assert torch.equal(gn.cpu(), torch.from_numpy(n)) and torch.equal(gp.cpu(), torch.from_numpy(p)), c
    want = torch.from_numpy(windows_multi(s.x, st.Ns, st.Ls, p[:, :, START], n, -64, 256, 0)).to(ctx.device)
    listed = listed or s.listed()
    ctx.set_option("debug_flags", flags)
    try:
        for sideband in (False, True):
            got = st.plan.decode_windows(st.enc, gp[:, :, START], 256, count=gn, offset=-64, out=prefilled(ctx, want.shape, 0),
                                         wave_words=st.table if sideband else None)
            k = st.plan.last_windows_listed()
            call = (c.id, "windows of the pulses", flags, sideband, "listed", k)
            assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.finish() == 0, call
            assert st.plan.last_windows_form() == form, (call, st.plan.last_windows_form())
            assert listed(k), call
            assert torch.equal(got, want), call
    finally:
        ctx.set_option("debug_flags", 0)


def transcode_check(ctx, O, s, targets, form, flags=0, listed=None, what=""):
    """The re-code at every target against the oracle's encode of the samples -- words, chunk offsets, side-band -- and a decode
    of the result; at the plan's own parameter the input word for word."""
    st, c = s.st, s.cell
    listed = listed or s.listed()
    ctx.set_option("debug_flags", flags)
    try:
        for m2 in targets:
            want = Want(O, s.x, st.Ns, st.Ls, m2, s.taps)
            for sideband in (False, True):
                t = st.plan.transcode(st.enc, rice_m=m2, wave_words=st.table if sideband else None)
                k = st.plan.last_transcode_listed()
                call = (c.id, what, flags, m2, sideband, "listed", k)
                assert st.plan.last_decode_path() == D.PATH_TRANSCODE, call
                assert st.plan.last_transcode_form() == form, (call, st.plan.last_transcode_form())
                assert listed(k), call
                assert t.rice_m == m2
                same_stream(t, want, call)
                if m2 == c.m:
                    assert t.enc.to_numpy()[0].tobytes() == st.words.tobytes(), call
            p2 = t.plan(ctx)
            try:
                assert torch.equal(p2.decode(t.enc), st.xd), (c.id, what, flags, m2, "decode of the result")
            finally:
                p2.close()
    finally:
        ctx.set_option("debug_flags", 0)


def estimate_check(ctx, O, s, form, flags=0, listed=None, what=""):
    st = s.st
    listed = listed or s.listed()
    want = [Want(O, s.x, st.Ns, st.Ls, 1 << k, s.taps).total for k in range(16)]
    ctx.set_option("debug_flags", flags)
    try:
        for sideband in (False, True):
            got = st.plan.estimate_words_encoded(st.enc, wave_words=st.table if sideband else None)
            k = st.plan.last_transcode_listed()
            call = (s.cell.id, what, flags, "estimate", sideband, "listed", k)
            assert st.plan.last_decode_path() == D.PATH_TRANSCODE and st.plan.last_transcode_form() == form, call
            assert listed(k), call
            assert got.dtype == np.uint64 and got.tolist() == want, (call, got.tolist(), want)
        assert int(got[s.cell.k]) == st.enc.total_words  # (the stream's own parameter: its own total)
    finally:
        ctx.set_option("debug_flags", 0)


# --------------------------------------------------------------------------- 1. every cell, the block forms
def test_wave_stats(ctx, cs):
    stats_check(ctx, cs.st, cs.x, heads_of(cs.cell.L), BLOCKS, what=cs.cell.id)


def test_find_pulses(ctx, cs):
    pulses_check(ctx, cs, pulse_cases(cs), BLOCKS)


def test_decode_windows(ctx, cs):
    try:
        check_tiling(ctx, cs.st, cs.x, 333, BLOCKS, what=(cs.cell.id, "tiling"), listed=cs.listed())  # the rows are the decode
    except AssertionError as e:
        raise AssertionError((e.args, "listed", cs.seen[-4:])) from e
    windows(ctx, cs, sorted_cases(np.random.default_rng(cs.cell.k), cs.st), BLOCKS, what="random windows")
    pulse_windows(ctx, cs, BLOCKS)


def test_transcode_and_estimate(ctx, O, cs):
    transcode_check(ctx, O, cs, sorted({1, 8, 32768, cs.cell.m}), BLOCKS)
    estimate_check(ctx, O, cs, BLOCKS)


# --------------------------------------------------------------------------- 2. every cell once more: all listed, and the lane form
def test_all_fallback_and_lanes(ctx, O, cs):
    c = cs.cell
    T = pulse_cases(cs)[2:3]
    one_window = sorted_cases(np.random.default_rng(c.k), cs.st)[:1]
    for form, rule, flag in ((BLOCKS | ALL, "all", "ALL_FALLBACK"), (LANES, "lanes", "LANES")):
        f = lambda call: getattr(D, f"DBG_{call}_{flag}")  # noqa: E731
        stats_check(ctx, cs.st, cs.x, (100,), form, what=(c.id, flag), flags=f("STATS"))
        pulses_check(ctx, cs, T, form, flags=f("PULSES"), listed=cs.listed(rule), what=flag)
        windows(ctx, cs, one_window, form, flags=f("WINDOWS"), listed=cs.listed(rule), what=flag)
        transcode_check(ctx, O, cs, (1,), form, flags=f("TRANSCODE"), listed=cs.listed(rule), what=flag)
        estimate_check(ctx, O, cs, form, flags=f("TRANSCODE"), listed=cs.listed(rule), what=flag)


# --------------------------------------------------------------------------- 3. the re-code under another filter
@pytest.mark.parametrize("cell", [c for c in bc.CELLS if c.L == 3000 and c.k in (0, 15)], ids=lambda c: c.id)
def test_transcode_under_four_taps(ctx, O, cell):
    """The transcode form admits every filter: the L = 3000 cells at k = 0 and 15 under taps (1, -1, 1, -1)"""
    s = CellStream(ctx, O, cell, TAPS)
    try:
        assert torch.equal(s.st.plan.decode(s.st.enc), s.st.xd)
        transcode_check(ctx, O, s, sorted({1, 8, 32768, cell.m}), BLOCKS, what="fir4")
        estimate_check(ctx, O, s, BLOCKS, what="fir4")
        transcode_check(ctx, O, s, (1,), BLOCKS | ALL, flags=D.DBG_TRANSCODE_ALL_FALLBACK, listed=s.listed("all"), what="fir4")
        transcode_check(ctx, O, s, (1,), LANES, flags=D.DBG_TRANSCODE_LANES, listed=s.listed("lanes"), what="fir4")
    finally:
        s.close()


# --------------------------------------------------------------------------- 4. where a payload ends in its last block
@pytest.mark.parametrize("k,L,kind", bc.RESIDUE_CELLS)
def test_payload_ends_around_a_block_border(ctx, O, k, L, kind):
    """The chunks' last waveform at the lengths at which the payload of chunk 0's ends n words in with n mod (words per block)
    in {0, 1, 3, 4, 5, 8, 9, B - 1} (tests/block_cells.py searches them; the model test names the residues no length reaches):
    all four calls, with heads and windows that end one sample before, at and one behind the waveform's last sample, and a
    threshold column that makes every waveform's last sample part of a run."""
    found = {name: cell for name, cell in bc.residue_cells(O, k, L, kind).items() if cell is not None}
    assert found
    for name, cell in found.items():
        s = CellStream(ctx, O, cell)
        st, n = s.st, cell.last
        try:
            what = (f"residue {name}", n)
            assert st.length[2] == n and st.length[5] == n
            stats_check(ctx, st, s.x, (n - 1, n, n + 1, L), BLOCKS, what=(cell.id, what))
            last = s.x[st.start + st.length - 1].astype(np.int64)
            pulses_check(ctx, s, [(-1, 1, 1, 64, last), (1, -1, 1, 0, last), (-1, 1, 2, 3, last)], BLOCKS, what=what)
            ends = (st.length[:, None] - 64 + np.array([-1, 0, 1])[None, :]).astype(np.int64)  # windows that end at len - 1, len, len + 1
            windows(ctx, s, [(ends, None, 0, 64, -3)], BLOCKS, what=what)
            check_tiling(ctx, st, s.x, 333, BLOCKS, what=(cell.id, what, "tiling"), listed=s.listed())
            transcode_check(ctx, O, s, sorted({1, 32768, cell.m}), BLOCKS, what=what)
            estimate_check(ctx, O, s, BLOCKS, what=what)
        finally:
            s.close()
