"""GPU: drx_transcode / drx_estimate_words_encoded for few long waveforms -- a workgroup per block of a waveform's stream, for
the sizes and again for the pack (csrc/drx_transcode_blocks.hip).

The batches that drx_decode gives to its block decoder take that form under every prediction filter;
drx_plan_last_transcode_form says which form ran, drx_plan_last_decode_path keeps saying DRX_PATH_TRANSCODE alone.  The streams
and the expectations are the oracle's (oracle.encode_chunk at the target parameter; for a lead other than +-1 the oracle's decode
of both streams), the comparison tobytes() on words, offsets and side-band plus a decode of the result.  Every cell asserts the
path and the expected form."""
import ctypes as C

import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_noise_levels import LEVELS, noise
from test_gpu_placement import FF, PLACEMENTS, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, header_table
from test_gpu_transcode import Want, check, opts_of, same_stream
from test_gpu_wave_stats_blocks import crafted
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS, ALL = D.TRANSCODE_FORM_LANES, D.TRANSCODE_FORM_BLOCKS, D.TRANSCODE_FORM_FALLBACK_ALL


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


def stream_of(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    return Stream(ctx, O, x, Ns, Ls, m, taps), x


def cells(ctx, O, st, x, targets, form, what="", flags=0, taps=None, sidebands=(False, True), listed=None):
    """check() of test_gpu_transcode for every target -- bytes by the walk and by the side-band, a decode of the result -- under
    the debug flags, with the form of the call (transcode() sizes first, then packs: both calls' form is the last one's)."""
    ctx.set_option("debug_flags", flags)
    try:
        for m2 in targets:
            check(ctx, st, Want(O, x, st.Ns, st.Ls, m2, taps), m2, sidebands=sidebands, decodes_to=st.xd, what=(what, flags))
            assert st.plan.last_transcode_form() == form, (what, m2, flags, st.plan.last_transcode_form())
            if listed is not None:
                assert st.plan.last_transcode_listed() == listed, (what, m2, flags, st.plan.last_transcode_listed())
    finally:
        ctx.set_option("debug_flags", 0)


# --------------------------------------------------------------------------- 1. which batches take which form
@pytest.mark.parametrize("name,form", [("long-2", BLOCKS), ("long-40", BLOCKS), ("whole-chunk", BLOCKS),
                                       ("stream-quiet", LANES), ("short", LANES)])
def test_forms(ctx, O, name, form):
    st, x = stream_of(ctx, O, name)
    m = BATCHES[name][2]
    targets = (16,) if name == "long-40" else sorted({1, 8, 32, 32768, m})  # (long-40: the CPU oracle is the cost)
    try:
        assert st.plan.last_transcode_form() == 0  # no such call yet
        cells(ctx, O, st, x, targets, form, what=name)
        if form == LANES:
            assert st.plan.last_transcode_listed() == 0
        if name == "long-2":
            cells(ctx, O, st, x, (16,), LANES, what=name, flags=D.DBG_TRANSCODE_LANES, listed=0)
            cells(ctx, O, st, x, (16,), LANES, what=name, flags=D.DBG_NO_LONG_PATHS, listed=0)
            cells(ctx, O, st, x, targets, BLOCKS | ALL, what=name, flags=D.DBG_TRANSCODE_ALL_FALLBACK, listed=st.plan.total_waves)
            cells(ctx, O, st, x, (16,), BLOCKS, what=name)
    finally:
        st.plan.close()


def test_forms_general_filters(ctx, O):
    Ns, Ls, m, _, sigma = BATCHES["long-2"]
    x = np.random.default_rng(12).normal(0, sigma, sum(Ns)).astype(np.int16)
    # four taps with lead 1: byte-exact against the oracle's encode of the samples
    taps = (1, -1, 1, -1)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        cells(ctx, O, st, x, (1, 32, 32768), BLOCKS, what="fir4", taps=taps)
    finally:
        st.plan.close()
    # five taps with lead 3: compared by the oracle's decode of both streams
    taps = (3, -1, 1, -1, 1)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        ys = [O.decode_chunk(st.words[int(a):int(b)], opts_of(m, L, taps)) for a, b, L in zip(st.offs[:-1], st.offs[1:], Ls)]
        for m2 in (1, 32768):
            for sideband in (False, True):
                t = st.plan.transcode(st.enc, rice_m=m2, wave_words=st.table if sideband else None)
                assert st.plan.last_decode_path() == D.PATH_TRANSCODE and st.plan.last_transcode_form() == BLOCKS, (m2, sideband)
                w, offs = t.enc.to_numpy()
                for c, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
                    assert O.decode_chunk(w[int(a):int(b)], opts_of(m2, Ls[c], taps)).tobytes() == ys[c].tobytes(), (m2, sideband, c)
                assert t.wave_words.cpu().numpy().view(np.uint32).tobytes() == header_table(w, offs, Ns, Ls).tobytes()
        t = st.plan.transcode(st.enc, rice_m=m)  # the plan's own parameter: the input, word for word
        assert t.enc.total_words == st.enc.total_words and t.enc.to_numpy()[0].tobytes() == st.words.tobytes()
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. the block geometries
def test_geometry_classes(ctx, O):
    """9 / 11 / 15 / 19 stream words per lane by the stream's bits per sample, re-coded at the targets of the largest expansion
    and contraction; and waveforms of one or two blocks (64 / 128 lanes per block) in the outer classes."""
    rng = np.random.default_rng(41)
    seen = set()
    for sigma, m in LEVELS:
        x = noise(rng, sigma, 2 * 3 * 90000)
        st = Stream(ctx, O, x, [3 * 90000] * 2, [90000] * 2, m)
        try:
            bits = st.words.size * 32.0 / x.size
            seen.add(9 if bits < 5.4 else 11 if bits < 8.2 else 15 if bits < 11.7 else 19)
            cells(ctx, O, st, x, (1, 32768), BLOCKS, what=(sigma, m), sidebands=(False,))
        finally:
            st.plan.close()
    assert seen == {9, 11, 15, 19}, seen
    for sigma, m, L in [(1, 8, 5000), (2000, 2048, 4000), (1, 8, 12000), (2000, 2048, 9000)]:
        N = 7 * L - L // 3
        x = noise(rng, sigma, 3 * N)
        st = Stream(ctx, O, x, [N] * 3, [L] * 3, m)
        try:
            cells(ctx, O, st, x, (1, 32768), BLOCKS, what=(sigma, m, L))
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
        cells(ctx, O, st, x, (1, 8, 32768), BLOCKS, what="quiet stretches")  # (m' = 1: a drain of many passes)
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
        cells(ctx, O, st, x, (1, 64), BLOCKS, what=case)  # bytes, whatever last_transcode_listed() says
        if case == "ramp with noise stretches":
            # the result does not depend on which waveforms a launch happened to flag: three further calls, byte for byte
            want = Want(O, x, st.Ns, st.Ls, 64)
            for again in range(3):
                t = st.plan.transcode(st.enc, rice_m=64)
                assert st.plan.last_transcode_form() == BLOCKS
                same_stream(t, want, (case, "again", again, st.plan.last_transcode_listed()))
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 5. crafted rows
def test_crafted_rows(ctx, O):
    """The four rows of the statistics block test (test_gpu_wave_stats.crafted_rows has fifteen and takes no fewer): ties, a
    running sum that wraps, constant -32768, alternating extremes (escapes with z up to 65535), as 2 chunks of 2 x 70 000."""
    x, _ = crafted(L=70000)
    W, L = x.shape
    assert W == 4 and bool((x[2] == -32768).all()) and int(x[3].max()) - int(x[3].min()) == 65535
    x = np.ascontiguousarray(x).reshape(-1)
    st = Stream(ctx, O, x, [2 * L] * 2, [L] * 2, 8)
    try:
        cells(ctx, O, st, x, (1, 4096), BLOCKS, what="crafted")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 6. a ragged plan of long waveforms
RAGGED = ([2048 * 5 + 9, 30000 * 3, 150001, 9001 * 4 - 3000], [2048, 30000, 0, 9001])


def test_ragged_long_batch(ctx, O):
    Ns, Ls = RAGGED
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        cells(ctx, O, st, x, (1, 32), BLOCKS, what="ragged")
        cells(ctx, O, st, x, (1, 32), BLOCKS | ALL, what="ragged", flags=D.DBG_TRANSCODE_ALL_FALLBACK, listed=st.plan.total_waves)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. where the buffers lie, and how large
def test_placements_capacity_sizing(ctx, O):
    st, x = stream_of(ctx, O, "long-2")
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    Ns = st.Ns
    want = Want(O, x, st.Ns, st.Ls, 16)
    slack = 67
    try:
        for ib in sorted({P["w"] for P in PLACEMENTS.values()}):  # the words at byte offsets 0, 4, 8 and 12
            ww = window(total + slack, torch.int32, ib, fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            for ob in (0, 4, 8, 12):
                for fill in (FF, 0x5A5A5A5A):  # (what OR-ing into a word that was not cleared would show)
                    cell = (ib, ob, fill)
                    yw = window(want.total, torch.int32, ob, fill=fill, device=ctx.device)  # out_cap_words = the total
                    ow = window(len(Ns) + 1, torch.int64, 8 if ob & 4 else 0, fill=fill, device=ctx.device)
                    nw = window(W, torch.int32, ob, fill=fill, device=ctx.device)
                    assert ww.t.data_ptr() % 16 == ib and yw.t.data_ptr() % 16 == ob
                    got = run(ctx, plan, lambda: plan.transcode_async(ww.t, st.enc.chunk_word_off, 16, yw.t, total, None, ow.t, nw.t))
                    assert got == want.total and plan.last_decode_path() == D.PATH_TRANSCODE and plan.last_transcode_form() == BLOCKS, cell
                    assert yw.t.cpu().numpy().view(np.uint32).tobytes() == want.words.tobytes(), cell
                    assert ow.t.cpu().numpy().view(np.uint64).tobytes() == want.offs.tobytes(), cell
                    assert nw.t.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes(), cell
                    assert yw.intact() and ow.intact() and nw.intact() and ww.intact(), cell
            assert bool((ww.t[total:] == FF).all()), ib
        # one word short: DRX_ERR_CAPACITY at finish, the total NEEDED reported, the whole window still holding its fill
        for fill in (FF, 0x5A5A5A5A):
            yw = window(want.total - 1, torch.int32, 4, fill=fill, device=ctx.device)
            ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
            plan.transcode_async(st.enc.words, st.enc.chunk_word_off, 16, yw.t, total)
            n = C.c_uint64()
            assert ctx.lib.drx_plan_finish(plan._h, C.byref(n)) == 3 and n.value == want.total
            assert plan.last_transcode_form() == BLOCKS
            assert bool((yw.t == fill).all()) and yw.intact(), fill
        # the sizing call: both tables and the total, nothing else
        ow = window(len(Ns) + 1, torch.int64, 8, fill=-1, device=ctx.device)
        nw = window(W, torch.int32, 4, fill=-1, device=ctx.device)
        got = run(ctx, plan, lambda: plan.transcode_async(st.enc.words, st.enc.chunk_word_off, 16, None, total, None, ow.t, nw.t))
        assert got == want.total and plan.last_transcode_form() == BLOCKS
        assert ow.t.cpu().numpy().view(np.uint64).tobytes() == want.offs.tobytes() and ow.intact()
        assert nw.t.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes() and nw.intact()
    finally:
        plan.close()


# --------------------------------------------------------------------------- 8. verdicts
def test_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [3 * 40000], [40000]
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    want = Want(O, x, Ns, Ls, 32)
    w = st.words
    h1 = 1 + 1 + int(w[1])  # the header of waveform 1: behind the chunk's word, waveform 0's header and its payload
    n1 = int(w[h1])
    cap = plan.max_encoded_words

    def batch_of(words):
        off = torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device)
        return dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), off, int(words.size)), words

    def clean():
        same_stream(plan.transcode(good, rice_m=32), want, "the call after")
        assert plan.last_decode_path() == D.PATH_TRANSCODE and plan.last_transcode_form() == BLOCKS

    def refused(enc, cname, table=None):
        for fill in (FF, 0x5A5A5A5A):
            yw = window(cap, torch.int32, 4, fill=fill, device=ctx.device)
            with pytest.raises(dr.DeltaRiceError) as e:
                run(ctx, plan, lambda: plan.transcode_async(enc.words, enc.chunk_word_off, 32, yw.t, enc.total_words, table))
            assert e.value.status == 4, cname
            assert plan.last_transcode_form() == BLOCKS, cname
            assert bool((yw.t == fill).all()) and yw.intact(), (cname, fill)

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
            refused(enc, cname)
            clean()  # the plan stays usable, and its next call starts clean
            with pytest.raises(dr.DeltaRiceError) as e:  # the estimate returns the verdict itself
                plan.estimate_words_encoded(enc)
            assert e.value.status == 4 and plan.last_transcode_form() == BLOCKS, cname
            clean()
            if cname != "chain":  # ... and by the side-band (the table that belongs to that stream)
                table = torch.from_numpy(header_table(words, np.array([0, words.size]), Ns, Ls).view(np.int32)).to(ctx.device)
                refused(enc, cname, table)
                clean()
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. the estimate
@pytest.mark.parametrize("name", ["long-2", "whole-chunk", "ragged"])
def test_estimate(ctx, O, name):
    if name == "ragged":
        Ns, Ls = RAGGED
        x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, 8)
    else:
        st, x = stream_of(ctx, O, name)
    try:
        want = [Want(O, x, st.Ns, st.Ls, 1 << k).total for k in range(16)]
        for flags, form, listed in ((0, BLOCKS, None), (D.DBG_TRANSCODE_ALL_FALLBACK, BLOCKS | ALL, st.plan.total_waves)):
            ctx.set_option("debug_flags", flags)
            for sideband in (False, True):
                got = st.plan.estimate_words_encoded(st.enc, wave_words=st.table if sideband else None)
                assert st.plan.last_decode_path() == D.PATH_TRANSCODE and st.plan.last_transcode_form() == form, (name, flags, sideband)
                assert got.dtype == np.uint64 and got.tolist() == want, (name, flags, sideband)
                if listed is not None:
                    assert st.plan.last_transcode_listed() == listed
        assert int(got[3]) == st.enc.total_words  # (m = 8: a canonical stream's own total)
    finally:
        ctx.set_option("debug_flags", 0)
        st.plan.close()


# --------------------------------------------------------------------------- 10. among the plan's other calls
def test_sequences_on_one_plan(ctx, O):
    st, x = stream_of(ctx, O, "long-2")
    plan = st.plan
    taps = (1, -1, 1, -1)
    fst = Stream(ctx, O, x, st.Ns, st.Ls, 8, taps)  # the same samples under another filter (its plan is not used)
    want, fwant = Want(O, x, st.Ns, st.Ls, 64), Want(O, x, st.Ns, st.Ls, 64, taps)
    stats = torch.from_numpy(wave_stats_heads(x, st.Ns, st.Ls, [100])[0]).to(ctx.device)

    def trc(enc, w, **kw):
        t = plan.transcode(enc, rice_m=64, **kw)
        assert plan.last_decode_path() == D.PATH_TRANSCODE and plan.last_transcode_form() == BLOCKS and plan.finish() == w.total
        same_stream(t, w, "in sequence")

    try:
        trc(st.enc, want)
        assert torch.equal(plan.decode(st.enc), st.xd) and plan.last_decode_path() & D.PATH_BLOCKS  # (shares the block scratch)
        trc(st.enc, want)
        assert torch.equal(plan.wave_stats(st.enc, head=100), stats) and plan.last_stats_form() == D.STATS_FORM_BLOCKS
        trc(st.enc, want, wave_words=st.table)
        assert plan.last_transcode_form() == BLOCKS
        plan.set_filter(taps)
        trc(fst.enc, fwant)
        assert torch.equal(plan.decode(fst.enc), st.xd)
        plan.set_filter(None)
        trc(st.enc, want)
    finally:
        plan.close()
        fst.plan.close()
