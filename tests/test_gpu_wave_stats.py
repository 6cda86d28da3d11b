"""GPU: drx_wave_stats -- eight exact statistics per waveform, parsed from the encoded stream.

The streams are the oracle's (oracle.encode_chunk), the expected rows numpy's over the oracle's input
(tests/wave_stats_reference.py; for a filter whose lead is not +-1, over the oracle's decode of that stream), the comparison
torch.equal on all eight columns of every row.  Every cell asserts DRX_PATH_STATS alone."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES, make_plan
from test_gpu_select import Stream, geometry, header_table  # noqa: F401  (Stream builds its side-band with header_table)
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U32 = (1 << 32) - 1


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


def opts_of(m, L, taps):
    return ((m, L) if L else (m,)) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())


def samples_of(O, st, x, m, taps):
    """What the stream decodes to: the oracle's input, or -- a lead that is not +-1 divides -- the oracle's decode of it."""
    if not taps or taps[0] in (1, -1):
        return x
    return np.concatenate([O.decode_chunk(st.words[st.offs[c]:st.offs[c + 1]], opts_of(m, L, taps)) for c, L in enumerate(st.Ls)])


def check(ctx, st, y, heads, sidebands=(False, True), what=""):
    """Every head x {walk, side-band} on st against numpy over the samples y."""
    wants = wave_stats_heads(y, st.Ns, st.Ls, heads)
    assert wants[0].shape == (st.plan.total_waves, D.STAT_COLS)
    for head, want in zip(heads, wants):
        want = torch.from_numpy(want).to(ctx.device)
        for sideband in sidebands:
            got = st.plan.wave_stats(st.enc, head=head, wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_STATS, (what, head, sideband)
            assert got.dtype == torch.int64 and got.shape == want.shape, (what, head, sideband)
            if not torch.equal(got, want):
                bad = torch.nonzero((got != want).any(dim=1)).flatten()
                g = int(bad[0])
                raise AssertionError((what, head, sideband, f"{bad.numel()} rows differ; row {g}", got[g].tolist(), want[g].tolist()))


# --------------------------------------------------------------------------- 1. every batch of the route table
@pytest.mark.parametrize("name", list(BATCHES))
def test_stats_every_batch(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        check(ctx, st, samples_of(O, st, x, m, taps), (0, 100), what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. where the head window ends
def test_stats_window_boundaries(ctx, O):
    Ns, Ls = [130 * 200 + 37] * 3, [200] * 3  # 131 waveforms per chunk: two wavefronts and two lanes, the last one of 37 samples
    x = np.random.default_rng(2).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        check(ctx, st, x, (0, 1, 15, 16, 17, 63, 64, 65, 199, 200, 201, U32), sidebands=(False,), what="window")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 3. crafted rows
def crafted_rows(W=70, L=70000):
    rng = np.random.default_rng(3)
    x = np.empty((W, L), np.int16)
    for i in range(W):
        x[i] = rng.normal(0, (1, 400, 5000)[i % 3], L).astype(np.int16)
    x[0] = -32768  # sum below -2^31, sum of squares above 2^46
    x[1] = 32767
    x[2] = np.where(np.arange(L) & 1, 16000, 0)  # an escape every sample: the hungriest stream
    x[3] = (np.arange(L) + 30000).astype(np.uint16).view(np.int16)  # a slope-1 ramp through the int16 wrap
    n = rng.normal(0, 10, L).astype(np.int16)
    n[5:10] = 200
    n[69990] = 200  # (the plateau's first sample wins)
    n[0] = n[L - 1] = -200
    x[4] = n
    for j, p in enumerate((15, 16, 63, 64, L - 1)):
        for row, v in ((5 + j, 3000), (10 + j, -3000)):
            n = rng.normal(0, 10, L).astype(np.int16)
            n[p] = v
            x[row] = n
    return x


def test_stats_crafted_rows(ctx, O):
    x = crafted_rows()
    W, L = x.shape
    st = Stream(ctx, O, x.reshape(-1), [W * L], [L], 8)
    try:
        want = wave_stats_heads(x.reshape(-1), st.Ns, st.Ls, [100])[0]
        assert want[0, D.STAT_SUM] < -(1 << 31) and want[0, D.STAT_SUMSQ] > 1 << 46
        assert want[4].tolist()[:4] == [-200, 0, 200, 5]
        assert [int(want[5 + j, D.STAT_ARGMAX]) for j in range(5)] == [15, 16, 63, 64, L - 1]
        assert [int(want[10 + j, D.STAT_ARGMIN]) for j in range(5)] == [15, 16, 63, 64, L - 1]
        check(ctx, st, x.reshape(-1), (100,), what="crafted")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. RiceParameter
@pytest.mark.parametrize("m", [1, 8, 64, 32768])
def test_stats_rice_parameters(ctx, O, m):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    for sigma in (10, 400):
        x = np.random.default_rng(m + sigma).normal(0, sigma, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, m)
        try:
            check(ctx, st, x, (0, 100), what=(m, sigma))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 5. filters through the serial kernel
FILTERS = {
    "minus-delta": (-1, 1),
    "second-difference": (1, -2, 1),
    "lead-3": (3, -1),
    "five-taps": (1, -1, 1, -1, 1),
    "64-taps": (1,) + tuple(int(v) for v in np.random.default_rng(64).integers(-1, 2, 63)),
}


@pytest.mark.parametrize("fname", list(FILTERS))
def test_stats_filters(ctx, O, fname):
    taps = FILTERS[fname]
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(len(taps)).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        check(ctx, st, samples_of(O, st, x, 8, taps), (0, 100), what=fname)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 6. ragged plans, the smallest batch
def test_stats_ragged_lengths_and_one_sample(ctx, O):
    Ns, Ls = [64 * 70 + 5, 512 * 3, 7000 * 2 + 100, 999], [64, 512, 7000, 0]
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        check(ctx, st, x, (0, 100), what="ragged lengths")
    finally:
        st.plan.close()
    x = np.array([-123], np.int16)
    st = Stream(ctx, O, x, [1], [0], 8)
    try:
        check(ctx, st, x, (0, 1, 100), what="one sample")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. where the buffers lie
def test_stats_placements(ctx, O):
    Ns, Ls = [130 * 200 + 37] * 3, [200] * 3
    x = np.random.default_rng(7).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    want = torch.from_numpy(wave_stats_heads(x, Ns, Ls, [100])[0]).to(ctx.device)
    try:
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            for obyte in (8, 0):  # an 8-byte offset that is not 16-byte aligned, and the aligned control
                for fill in (0x5A5A5A5A5A5A5A5A, -1):
                    yw = window(W * D.STAT_COLS, torch.int64, obyte, fill=fill, device=ctx.device)
                    assert yw.t.data_ptr() % 16 == obyte
                    out = yw.t.view(W, D.STAT_COLS)
                    run(ctx, plan, lambda: plan.wave_stats_async(ww.t, ow.t, head=100, out=out, in_words=total))
                    assert plan.last_decode_path() == D.PATH_STATS
                    same, intact = torch.equal(out, want), yw.intact() and ow.intact() and ww.intact()
                    assert same and intact, (pname, obyte, fill, "rows differ" * (not same), "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
    finally:
        plan.close()


# --------------------------------------------------------------------------- 8. verdicts
def flipped_payload(O, words, offs, Ns, Ls, k):
    """The stream with ONE payload bit flipped, chosen with the oracle's own parser so that every code is still a valid one but
    the waveform's codes no longer end in its last payload word.  (A flip changes a code's length, the parse re-synchronises
    within a few codes and the waveform's end moves by about one code: unnoticed by any decoder unless that crosses a word
    boundary.  So: a waveform whose last word holds at most four bits of code, and a flip that makes two codes of one.)"""
    start, length, chunk = geometry(Ns, Ls)
    at, c = 1, 0
    for g in range(start.size - 1):
        if chunk[g] != c:
            c, at = c + 1, int(offs[c + 1]) + 1
        n = int(words[at])
        clean = O.rice_unpack(words[at + 1:at + 1 + n], int(length[g]), k)[1]
        if 1 <= clean - 32 * (n - 1) <= 4:
            for bit in range(clean - 1, -1, -1):
                p = words[at + 1:at + 1 + n].copy()
                p[bit >> 5] ^= np.uint32(1 << (31 - (bit & 31)))
                used = O.rice_unpack(p, int(length[g]), k)[1]
                if used >= 0 and (used + 31) // 32 != n:
                    w = words.copy()
                    w[at + 1:at + 1 + n] = p
                    return w
        at += n + 1
    raise AssertionError("no single flip moves a payload's end out of its last word")


def test_stats_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    want = torch.from_numpy(wave_stats_heads(x, Ns, Ls, [100])[0]).to(ctx.device)

    def batch_of(w):
        return dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)

    def clean():
        assert torch.equal(plan.wave_stats(good, head=100), want) and plan.last_decode_path() == D.PATH_STATS

    try:
        clean()
        header = st.words.copy()
        header[int(st.offs[1]) + 1] += 1  # the first waveform header of chunk 1
        cases = {"header": batch_of(header), "payload": batch_of(flipped_payload(O, st.words, st.offs, Ns, Ls, 3)),
                 "short": dr.EncodedBatch(good.words, good.chunk_word_off, good.total_words - 1)}
        for cname, enc in cases.items():
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.wave_stats(enc, head=100)
            assert e.value.status == 4, cname
            clean()  # the plan stays usable, and its next call starts clean
        other = Stream(ctx, O, np.roll(x, 4321), Ns, Ls, 8)
        try:
            assert not torch.equal(other.table, st.table)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.wave_stats(good, head=100, wave_words=other.table)
            assert e.value.status == 4
        finally:
            other.plan.close()
        clean()
        # NULL pointers: DRX_ERR_ARG, nothing launched -- the status word keeps the verdict of the call before
        out = torch.full((plan.total_waves, D.STAT_COLS), 0x5A5A, dtype=torch.int64, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.wave_stats_async(cases["header"].words, good.chunk_word_off, head=100, out=out, in_words=good.total_words)
        lib, w, off = ctx.lib, good.words.data_ptr(), good.chunk_word_off.data_ptr()
        assert lib.drx_wave_stats(plan._h, w, good.total_words, off, 100, None) == 1
        assert lib.drx_wave_stats(plan._h, None, good.total_words, off, 100, out.data_ptr()) == 1
        assert lib.drx_wave_stats(plan._h, w, good.total_words, None, 100, out.data_ptr()) == 1
        assert lib.drx_wave_stats_with_wave_words(plan._h, w, good.total_words, off, None, 100, out.data_ptr()) == 1
        assert lib.drx_wave_stats_with_wave_words(plan._h, w, good.total_words, off, lib.drx_plan_wave_words(plan._h), 100, out.data_ptr()) == 1
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.finish()
        assert e.value.status == 4
        clean()
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. among the plan's other calls
def test_stats_in_sequence_on_one_plan(ctx, O):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(9).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan = st.plan
    want = torch.from_numpy(wave_stats_heads(x, Ns, Ls, [100])[0]).to(ctx.device)
    taps = (1, -2, 1)
    fst = Stream(ctx, O, x, Ns, Ls, 8, taps)  # the same samples under another filter (its plan is not used)
    try:
        enc = plan.encode(st.xd)
        assert enc.total_words == st.enc.total_words and torch.equal(enc.words[:enc.total_words], st.enc.words)
        got = plan.wave_stats(enc, head=100)  # the plan's own encode, then its statistics
        assert plan.last_decode_path() == D.PATH_STATS and plan.finish() == 0 and torch.equal(got, want)
        assert torch.equal(plan.decode(enc), st.xd) and plan.last_decode_path() != D.PATH_STATS
        got = plan.wave_stats(enc, head=100, wave_words=plan.wave_words_device())
        assert plan.last_decode_path() == D.PATH_STATS and torch.equal(got, want)
        plan.set_filter(taps)
        got = plan.wave_stats(fst.enc, head=100)  # the serial kernel
        assert plan.last_decode_path() == D.PATH_STATS and plan.finish() == 0 and torch.equal(got, want)
        assert torch.equal(plan.decode(fst.enc), st.xd) and plan.last_decode_path() != D.PATH_STATS
        plan.set_filter(None)
        got = plan.wave_stats(st.enc, head=100)
        assert plan.last_decode_path() == D.PATH_STATS and plan.finish() == 0 and torch.equal(got, want)
        assert plan.encode(st.xd).total_words == st.enc.total_words  # (finish() reports an encode's words again)
    finally:
        plan.close()
        fst.plan.close()
