"""GPU: drx_wave_stats for few long waveforms -- a workgroup per block of a waveform's stream (csrc/drx_stats_blocks.hip).

The batches that drx_decode gives to its block decoder take that form under the delta filter; drx_plan_last_stats_form says
which form ran, drx_plan_last_decode_path keeps saying DRX_PATH_STATS alone.  The streams are the oracle's, the expected rows
numpy's over the oracle's input (tests/wave_stats_reference.py), the comparison torch.equal on all eight columns, by the walk
and by the side-band, for head windows of 0, 1, 100, len - 1, len and len + 1 samples unless a test says otherwise."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_noise_levels import LEVELS, noise
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, header_table
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS, ALL = D.STATS_FORM_LANES, D.STATS_FORM_BLOCKS, D.STATS_FORM_FALLBACK_ALL


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


def heads_of(L):
    return (0, 1, 100, L - 1, L, L + 1)


def check(ctx, st, x, heads, form, what="", flags=0, sidebands=(False, True)):
    """Every head x {walk, side-band} on st against numpy over the samples x; the form of every call."""
    wants = wave_stats_heads(x, st.Ns, st.Ls, heads)
    ctx.set_option("debug_flags", flags)
    try:
        for head, want in zip(heads, wants):
            want = torch.from_numpy(want).to(ctx.device)
            for sideband in sidebands:
                got = st.plan.wave_stats(st.enc, head=head, wave_words=st.table if sideband else None)
                assert st.plan.last_decode_path() == D.PATH_STATS, (what, head, sideband)
                assert st.plan.last_stats_form() == form, (what, head, sideband, st.plan.last_stats_form())
                if not torch.equal(got, want):
                    bad = torch.nonzero((got != want).any(dim=1)).flatten()
                    g = int(bad[0])
                    raise AssertionError((what, flags, head, sideband, f"{bad.numel()} rows differ; row {g}", got[g].tolist(), want[g].tolist()))
    finally:
        ctx.set_option("debug_flags", 0)


def stream_of(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    return Stream(ctx, O, x, Ns, Ls, m, taps), x


# --------------------------------------------------------------------------- 1. which batches take which form
@pytest.mark.parametrize("name,form", [("long-2", BLOCKS), ("long-40", BLOCKS), ("whole-chunk", BLOCKS),
                                       ("stream-quiet", LANES), ("short", LANES), ("fir4", LANES)])
def test_forms(ctx, O, name, form):
    st, x = stream_of(ctx, O, name)
    try:
        assert st.plan.last_stats_form() == 0  # no statistics call yet
        L = BATCHES[name][1][0] or BATCHES[name][0][0]
        check(ctx, st, x, heads_of(L), form, what=name)
        if name == "long-2":
            check(ctx, st, x, (100,), LANES, what=name, flags=D.DBG_STATS_LANES)
            check(ctx, st, x, (100,), LANES, what=name, flags=D.DBG_NO_LONG_PATHS)
            check(ctx, st, x, heads_of(L), BLOCKS | ALL, what=name, flags=D.DBG_STATS_ALL_FALLBACK)
            check(ctx, st, x, (100,), BLOCKS, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. the block geometries
def test_geometry_classes(ctx, O):
    """9 / 11 / 15 / 19 stream words per lane by the stream's bits per sample, and waveforms of one or two blocks (64 / 128
    lanes per block) in the outer classes."""
    rng = np.random.default_rng(41)
    seen = set()
    for sigma, m in LEVELS:
        x = noise(rng, sigma, 2 * 3 * 90000)
        st = Stream(ctx, O, x, [3 * 90000] * 2, [90000] * 2, m)
        try:
            bits = st.words.size * 32.0 / x.size
            seen.add(9 if bits < 5.4 else 11 if bits < 8.2 else 15 if bits < 11.7 else 19)
            check(ctx, st, x, heads_of(90000), BLOCKS, what=(sigma, m))
        finally:
            st.plan.close()
    assert seen == {9, 11, 15, 19}, seen
    for sigma, m, L in [(1, 8, 5000), (2000, 2048, 4000), (1, 8, 12000), (2000, 2048, 9000)]:
        N = 7 * L - L // 3
        x = noise(rng, sigma, 3 * N)
        st = Stream(ctx, O, x, [N] * 3, [L] * 3, m)
        try:
            check(ctx, st, x, heads_of(L), BLOCKS, what=(sigma, m, L))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 3. more codes on a lane than its share
def test_quiet_stretches_take_the_second_parse(ctx, O):
    rng = np.random.default_rng(42)
    x = noise(rng, 200, 2 * 2 * 120000).reshape(4, 120000)
    x[:, 30000:70000] = 0
    x[1, 90000:] = 7
    x = np.ascontiguousarray(x).reshape(-1)
    st = Stream(ctx, O, x, [2 * 120000] * 2, [120000] * 2, 256)
    try:
        check(ctx, st, x, heads_of(120000) + (30000, 50001, 70000), BLOCKS, what="quiet stretches")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. streams that do not fall into step
@pytest.mark.parametrize("case", ["slope 1 sawtooth", "square wave", "alternating +-1", "ramp with noise stretches"])
def test_equal_length_codes(ctx, O, case):
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
        check(ctx, st, x, heads_of(100000), BLOCKS, what=case)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 5. crafted rows
def crafted(L=50000):
    rng = np.random.default_rng(5)
    x = np.empty((4, L), np.int16)
    # ties: the maximum at sample 0 and again in the last block; the minimum first in the middle of the waveform and again 1
    # to 20 000 samples behind it (blocks hold some 10 000 samples here: repeats in the same lane, the next lane, the next
    # block and two blocks on)
    t = rng.normal(0, 10, L).astype(np.int16)
    t[0] = t[L - 10] = 300
    first = 20011
    for d in (0, 1, 2, 50, 997, 5000, 9000, 11000, 14000, 20000):
        t[first + d] = -300
    x[0] = t
    x[1] = np.cumsum(rng.normal(0, 300, L)).astype(np.int64).astype(np.int16)  # a running sum that wraps
    x[2] = -32768
    x[3] = np.where((np.arange(L) // 1000) % 2 == 0, 32767, -32768)
    return x, first


def test_crafted_rows(ctx, O):
    x, first = crafted()
    L = x.shape[1]
    flat = x.reshape(-1)
    st = Stream(ctx, O, flat, [2 * L] * 2, [L] * 2, 8)
    try:
        want = wave_stats_heads(flat, st.Ns, st.Ls, [L])[0]
        assert want[0].tolist()[:4] == [-300, first, 300, 0]
        assert int(want[1, D.STAT_MAX]) - int(want[1, D.STAT_MIN]) > 40000  # the running sum went round the int16 range
        assert want[2, D.STAT_SUMSQ] == L << 30 and want[2, D.STAT_SUM] == -32768 * L
        assert want[3].tolist()[:4] == [-32768, 1000, 32767, 0]
        check(ctx, st, flat, tuple(range(0, L + 1, 3331)) + (L - 1, L, L + 1), BLOCKS, what="crafted")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 6. a ragged plan of long waveforms
def test_ragged_long_batch(ctx, O):
    Ns, Ls = [2048 * 5 + 9, 30000 * 3, 150001, 9001 * 4 - 3000], [2048, 30000, 0, 9001]
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        assert torch.equal(st.plan.decode(st.enc), st.xd)
        assert st.plan.last_decode_path() & D.PATH_BLOCKS, st.plan.last_decode_path()  # (this shape: the block decoder's)
        check(ctx, st, x, (0, 1, 9, 100, 2047, 2048, 9001, 150000, 150001, 150002), BLOCKS, what="ragged")
        check(ctx, st, x, (100,), BLOCKS | ALL, what="ragged", flags=D.DBG_STATS_ALL_FALLBACK)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. where the buffers lie
def test_placements(ctx, O):
    st, x = stream_of(ctx, O, "long-2")
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    want = torch.from_numpy(wave_stats_heads(x, st.Ns, st.Ls, [100])[0]).to(ctx.device)
    try:
        for pname, P in PLACEMENTS.items():  # the words at byte offsets 0, 4, 8 and 12
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(st.Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            for obyte in (8, 0):  # an 8-byte address that is not 16-byte aligned, and the aligned control
                for fill in (0x5A5A5A5A5A5A5A5A, -1):
                    yw = window(W * D.STAT_COLS, torch.int64, obyte, fill=fill, device=ctx.device)
                    assert yw.t.data_ptr() % 16 == obyte
                    out = yw.t.view(W, D.STAT_COLS)
                    run(ctx, plan, lambda: plan.wave_stats_async(ww.t, ow.t, head=100, out=out, in_words=total))
                    assert plan.last_decode_path() == D.PATH_STATS and plan.last_stats_form() == BLOCKS
                    same, intact = torch.equal(out, want), yw.intact() and ow.intact() and ww.intact()
                    assert same and intact, (pname, obyte, fill, "rows differ" * (not same), "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
    finally:
        plan.close()


# --------------------------------------------------------------------------- 8. verdicts
def test_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [3 * 40000], [40000]
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    want = torch.from_numpy(wave_stats_heads(x, Ns, Ls, [100])[0]).to(ctx.device)
    w = st.words
    h1 = 1 + 1 + int(w[1])  # the header of waveform 1: behind the chunk's word, waveform 0's header and its payload
    n1 = int(w[h1])

    def batch_of(words):
        off = torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device)
        return dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), off, int(words.size)), words

    def clean():
        assert torch.equal(plan.wave_stats(good, head=100), want)
        assert plan.last_decode_path() == D.PATH_STATS and plan.last_stats_form() == BLOCKS

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
                plan.wave_stats(enc, head=100)
            assert e.value.status == 4, cname
            assert plan.last_stats_form() == BLOCKS, cname
            clean()  # the plan stays usable, and its next call starts clean
            if cname != "chain":  # ... and by the side-band (the table that belongs to that stream)
                table = torch.from_numpy(header_table(words, np.array([0, words.size]), Ns, Ls).view(np.int32)).to(ctx.device)
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.wave_stats(enc, head=100, wave_words=table)
                assert e.value.status == 4, cname
                clean()
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. among the plan's other calls
def test_sequences_on_one_plan(ctx, O):
    st, x = stream_of(ctx, O, "long-2")
    plan = st.plan
    taps = (1, -1, 1, -1)
    fst = Stream(ctx, O, x, st.Ns, st.Ls, 8, taps)  # the same samples under another filter (its plan is not used)
    want = torch.from_numpy(wave_stats_heads(x, st.Ns, st.Ls, [100])[0]).to(ctx.device)

    def stats(enc, form, **kw):
        got = plan.wave_stats(enc, head=100, **kw)
        assert plan.last_decode_path() == D.PATH_STATS and plan.last_stats_form() == form and plan.finish() == 0
        assert torch.equal(got, want)

    try:
        stats(st.enc, BLOCKS)
        assert torch.equal(plan.decode(st.enc), st.xd) and plan.last_decode_path() & D.PATH_BLOCKS  # (shares the block scratch)
        stats(st.enc, BLOCKS)
        st.check(np.array([0, 63, 17, 40]))
        stats(st.enc, BLOCKS, wave_words=st.table)
        assert torch.equal(plan.decode(st.enc), st.xd)
        assert plan.last_stats_form() == BLOCKS  # (the last STATISTICS call's)
        plan.set_filter(taps)
        stats(fst.enc, LANES)
        assert torch.equal(plan.decode(fst.enc), st.xd)
        plan.set_filter(None)
        stats(st.enc, BLOCKS)
    finally:
        plan.close()
        fst.plan.close()
