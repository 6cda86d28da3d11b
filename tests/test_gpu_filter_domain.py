"""GPU: every route a prediction filter can take, over the whole domain drx_plan_set_filter accepts -- 1 to 64 taps, any int32
coefficients, any lead but 0 (the table of tests/filter_reference.py, which tests/test_filter_reference.py holds the oracle
to).  Bytes and samples are the oracle's; drx_estimate_words, for which the oracle has no entry point, is held to the helper
module's sizes.  Every comparison is exact; every case is a few thousand samples unless its route needs more."""
import functools

import numpy as np
import pytest

import filter_reference as F
from deltarice_amd import _lib as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x5A5A
LANES_ANY = D.PATH_LANES | D.PATH_LANES_FUSED
RICE_M = (8, 2, 64, 32768)  # by the index of the WaveformLength in a filter's list


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


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def fast_decode(taps):
    """The filters the fast decoders take (include/deltarice_hip.h at drx_plan_set_filter): up to four taps, lead +-1."""
    return len(taps) <= 4 and abs(taps[0]) == 1


def wave_lens(n_taps):
    return sorted({L for L in (1, 2, n_taps - 1, n_taps, n_taps + 1, 63, 64, 65, 1000) if L >= 1})


@functools.lru_cache(maxsize=None)
def batch(name, L, li):
    """Three chunks of waveforms of L samples with a shorter last one (where L allows one), each chunk another kind of data.
    -> (N, m, x, opts)"""
    N = 4 * L + max(1, L // 3) if L > 1 else 5
    kinds = list(F.DATA)
    x = np.concatenate([F.make_data(kinds[(3 * li + c) % len(kinds)], N, seed=c) for c in range(3)])
    m = RICE_M[li % len(RICE_M)]
    return N, m, x, F.opts_of(m, L, F.FILTERS[name])


@functools.lru_cache(maxsize=None)
def expected(name, L, li):
    """-> (oracle words, chunk offsets, what the oracle decodes them to), computed once per case."""
    from oracle import oracle as O
    N, m, x, opts = batch(name, L, li)
    w, off = O.encode_batch(x, N, opts)
    y = O.decode_batch(w, off, N, opts)
    if F.lossless(F.FILTERS[name]):
        assert np.array_equal(y, x)
    return w, off, y


def as_encoded(ctx, w, off):
    import deltarice_amd as dr
    return dr.EncodedBatch(dev(ctx, w.view(np.int32)), dev(ctx, off.astype(np.int64)), w.size)


def test_every_data_kind_meets_every_filter():
    for name, taps in F.FILTERS.items():
        Ls = wave_lens(len(taps))
        assert len(Ls) >= 2  # (three chunks a length, another kind each: two lengths see all six)
        assert 1000 in Ls and (len(taps) == 1 or len(taps) - 1 in Ls)


@pytest.mark.parametrize("name", list(F.FILTERS))
def test_encoders(ctx, name):
    taps = F.FILTERS[name]
    single = len(taps) <= 4  # the single-pass encoders' filters
    try:
        for li, L in enumerate(wave_lens(len(taps))):
            N, m, x, opts = batch(name, L, li)
            ref_w, ref_off, _ = expected(name, L, li)
            plan = ctx.plan_uniform(3, N, opts)
            xd = dev(ctx, x)
            routes = [(0, 0), (1, 0), (2, 0), (2, D.DBG_FORCE_STREAM), (2, D.DBG_FORCE_PIECES)]
            if L >= 64:
                routes.append((2, D.DBG_FORCE_STREAM_SEGS))
            for eimpl, flags in routes:
                ctx.set_option("encode_impl", eimpl)
                ctx.set_option("debug_flags", flags)
                w, off = plan.encode(xd).to_numpy()
                what = (name, L, eimpl, flags)
                assert np.array_equal(off, ref_off), what
                assert np.array_equal(w, ref_w), what
                path = plan.last_encode_path()
                if eimpl == 0 or not single:
                    assert path == D.ENC_TWO_PASS, (what, path)
                else:
                    assert path != D.ENC_TWO_PASS, (what, path)
                    if flags == D.DBG_FORCE_STREAM:
                        assert path == D.ENC_STREAM, (what, path)
                    if flags == D.DBG_FORCE_STREAM_SEGS:
                        assert path == D.ENC_STREAM_SEGS, (what, path)
                    if flags == D.DBG_FORCE_PIECES and L >= 64:
                        assert path == D.ENC_PIECES, (what, path)
            plan.close()
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("encode_impl", 2)


@pytest.mark.parametrize("name", list(F.FILTERS))
def test_decoders(ctx, name):
    """decode_impl 0 / 7 / 8 and DBG_NO_LONG_PATHS, the oracle's stream and the GPU's own.  L = 1000 under 63 and 64 taps is
    where the 64-entry history of k_decode_simple wraps with every entry in use."""
    taps = F.FILTERS[name]
    try:
        for li, L in enumerate(wave_lens(len(taps))):
            N, m, x, opts = batch(name, L, li)
            ref_w, ref_off, want = expected(name, L, li)
            plan = ctx.plan_uniform(3, N, opts)
            own = plan.encode(dev(ctx, x))
            for which, enc in (("oracle's", as_encoded(ctx, ref_w, ref_off)), ("own", own)):
                for impl, flags in ((8, 0), (7, 0), (0, 0), (8, D.DBG_NO_LONG_PATHS)):
                    ctx.set_option("decode_impl", impl)
                    ctx.set_option("debug_flags", flags)
                    y = plan.decode(enc).cpu().numpy()
                    what = (name, L, which, impl, flags)
                    assert np.array_equal(y, want), what        # the oracle's decode: lossy leads too
                    if F.lossless(taps):
                        assert np.array_equal(y, x), what
                    path = plan.last_decode_path()
                    if impl != 0 and fast_decode(taps):         # (decode_impl 0 is the simple kernel for any filter)
                        assert not path & D.PATH_SIMPLE and path & LANES_ANY, (what, path)
                    else:
                        assert path == D.PATH_SIMPLE, (what, path)
            plan.close()
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("decode_impl", 8)


def wave_table(N, L, n_chunks):
    """(first sample, length) of every waveform of a uniform batch."""
    return [(c * N + s, n) for c in range(n_chunks) for s, n in F.waveforms(N, L)]


@pytest.mark.parametrize("name", list(F.FILTERS))
def test_select_gather_and_side_band(ctx, O, name):
    """decode_select (the lane-per-waveform kernel of drx_select.hip for every filter but the delta one), with and without the
    side-band; gather_encoded in both copy forms; decode_with_wave_words.  Waveforms shorter than the filter, and longer than
    its 64-entry history."""
    taps = F.FILTERS[name]
    nt = len(taps)
    try:
        for li, L in ((wave_lens(nt).index(max(nt - 1, 1)), max(nt - 1, 1)), (wave_lens(nt).index(1000), 1000)):
            N, m, x, opts = batch(name, L, li)
            ref_w, ref_off, want = expected(name, L, li)
            plan = ctx.plan_uniform(3, N, opts)
            enc = as_encoded(ctx, ref_w, ref_off)
            plan.encode(dev(ctx, x))
            table = plan.wave_words_device()

            # the encoder's n_i table as a side-band of the whole decode
            y = plan.decode_with_wave_words(enc.words, enc.chunk_word_off, table, in_words=enc.total_words)
            plan.finish()
            assert np.array_equal(y.cpu().numpy(), want), (name, L)

            # 40 waveforms, duplicates among them; the batch's first and last and a chunk's short last one are in
            waves = wave_table(N, L, 3)
            W = len(waves) // 3
            rng = np.random.default_rng((nt, L))
            sel = np.concatenate([[0, len(waves) - 1, W - 1, 0, W - 1], rng.integers(0, len(waves), 35)])
            stride = min(L, N) + 3
            for tab in (None, table):
                out = torch.full((sel.size, stride), SENTINEL, dtype=torch.int16, device=ctx.device)
                y = plan.decode_select(enc, sel, out=out, wave_words=tab).cpu().numpy()
                assert plan.last_decode_path() == D.PATH_SELECT
                for i, g in enumerate(sel):
                    s, n = waves[g]
                    assert np.array_equal(y[i, :n], want[s:s + n]), (name, L, tab is not None, i, int(g))
                    assert (y[i, n:] == SENTINEL).all(), (name, L, tab is not None, i, int(g))  # between the rows: untouched

            # entries of one length (the full waveforms), at two chunkings, both copy forms
            full = np.array([g for g, (s, n) in enumerate(waves) if n == min(L, N)])
            gsel = full[rng.integers(0, full.size, 12)]
            for cw, flags in ((5, 0), (12, D.DBG_GATHER_OTHER_COPY), (5, D.DBG_GATHER_OTHER_COPY), (12, 0)):
                ctx.set_option("debug_flags", flags)
                got = plan.gather_encoded(enc, gsel, cw, wave_words=table if cw == 5 else None)
                assert plan.last_decode_path() == D.PATH_GATHER
                bytes_want = [O.encode_chunk(np.concatenate([x[waves[g][0]:waves[g][0] + waves[g][1]] for g in gsel[c0:c0 + cw]]), opts)
                              for c0 in range(0, gsel.size, cw)]
                what = (name, L, cw, flags)
                assert np.array_equal(got.enc.chunk_word_off.cpu().numpy(), np.cumsum([0] + [w.size for w in bytes_want])), what
                assert np.array_equal(got.enc.words.cpu().numpy().view(np.uint32), np.concatenate(bytes_want)), what
                ctx.set_option("debug_flags", 0)
                if not F.lossless(taps):  # what those bytes decode to: the oracle's decode of the source rows
                    gp = got.plan(ctx)
                    rows = np.concatenate([want[waves[g][0]:waves[g][0] + waves[g][1]] for g in gsel])
                    assert np.array_equal(gp.decode(got.enc).cpu().numpy(), rows), what
                    gp.close()
            plan.close()
    finally:
        ctx.set_option("debug_flags", 0)


def sizes(chunks, taps):
    """What drx_estimate_words must return for chunks [(x, L)]: (16 sizes from the helper module, k = 0 defined)."""
    res = [F.chunk_residuals(x, L, taps) for x, L in chunks]
    est = [sum(1 + sum(1 + n_i for n_i in F.chunk_wave_words(d, L, k)) for d, (x, L) in zip(res, chunks)) for k in range(16)]
    z = np.concatenate([np.where(d < 0, -2 * d.astype(np.int64) - 1, 2 * d.astype(np.int64)) for d in res])
    return est, int(z.max()) < 32768


@pytest.mark.parametrize("name", ["t1_lead1_mag3", "t1_lead-32767_mag32767", "t4_lead1_mag3", "t4_lead-3_mag3", "t5_lead1_mag200",
                                  "t5_lead2_mag3", "t64_lead1_mag200", "t64_lead2_mag3", "i32_extremes", "mixed7"])
def test_estimate_words(ctx, name):
    """All 16 sizes, uniform and ragged plans.  RiceParameter 1 (k = 0) is defined only while every zig-zag value is below
    32768 (tests/fuzz_parity.py keeps its k = 0 cases inside the same rule): the entry is compared for
    such data only, and the small-coefficient filters over gauss50 are such data."""
    taps = F.FILTERS[name]
    k0_seen = False
    for kind in ("gauss50", "uniform", "steps"):
        N, L = 4 * 300 + 77, 300
        x = F.make_data(kind, 3 * N)
        plan = ctx.plan_uniform(3, N, F.opts_of(8, L, taps))
        est, k0 = sizes([(x[c * N:(c + 1) * N], L) for c in range(3)], taps)
        got = plan.estimate_words(dev(ctx, x))
        assert [int(v) for v in got[1:]] == est[1:], (name, kind)
        if k0:
            assert int(got[0]) == est[0], (name, kind)
            k0_seen = True
        plan.close()
        Ns, Ls = [700, 64 * 3 + 5, 333, 1000], [100, 64, 0, 7]
        x = F.make_data(kind, sum(Ns), seed=1)
        plan = ctx.plan(Ns, Ls, 8, taps=taps)
        at = np.concatenate([[0], np.cumsum(Ns)])
        est, k0 = sizes([(x[at[c]:at[c + 1]], Ls[c]) for c in range(len(Ns))], taps)
        got = plan.estimate_words(dev(ctx, x))
        assert [int(v) for v in got[1:]] == est[1:], (name, kind, "ragged")
        if k0:
            assert int(got[0]) == est[0], (name, kind, "ragged")
        plan.close()
    if max(abs(t) for t in taps) <= 3:
        assert k0_seen, name


def test_host_path_with_64_taps_and_its_refusals(ctx, O):
    """drx_filter_chunk_host both ways: cd_values of 3 + 64 entries, WaveformLength -1 (the whole chunk one waveform)."""
    import deltarice_amd as dr
    for name in ("t64_lead1_mag200", "t64_lead-1_mag32767", "t64_lead-3_mag200", "t63_lead1_mag3"):
        taps = F.FILTERS[name]
        opts = (8, 0xFFFFFFFF, len(taps)) + tuple(t & 0xFFFFFFFF for t in taps)
        assert len(opts) == 3 + len(taps)
        for kind in ("uniform", "gauss50"):
            x = F.make_data(kind, 2077)
            w = O.encode_chunk(x, opts)
            eb = ctx.filter_chunk(x, opts, reverse=False)
            assert eb == w.tobytes(), (name, kind)
            y = np.frombuffer(ctx.filter_chunk(eb, opts, reverse=True), np.int16)
            assert np.array_equal(y, O.decode_chunk(w, opts)), (name, kind)
            if F.lossless(taps):
                assert np.array_equal(y, x), (name, kind)
    x = F.make_data("gauss50", 500)
    t64 = tuple(t & 0xFFFFFFFF for t in F.FILTERS["t64_lead1_mag200"])
    refused = {"65 taps": (8, 100, 65) + t64 + (1,),
               "cd_nelmts one short": (8, 100, 64) + t64[:-1],
               "taps[0] = 0 at 64 taps": (8, 100, 64, 0) + t64[1:]}
    for why, opts in refused.items():
        with pytest.raises(dr.DeltaRiceError) as e:
            ctx.filter_chunk(x, opts, reverse=False)
        assert e.value.status == 1, why  # DRX_ERR_ARG
    plan = ctx.plan([500], [100], 8)
    with pytest.raises(dr.DeltaRiceError):
        ctx.plan([500], [100], 8, taps=(1,) * 65)
    with pytest.raises(dr.DeltaRiceError):
        ctx.plan([500], [100], 8, taps=(0,) + (1,) * 63)
    plan.close()


def test_delta_with_zero_taps_gives_the_delta_plans_bytes(ctx):
    """(1,-1,0) and (1,-1,0,0) are general filters to the library (three and four taps) and the delta filter in value."""
    for name in ("delta0", "delta00"):
        for li, L in enumerate(wave_lens(len(F.FILTERS[name]))):
            N, m, x, opts = batch(name, L, li)
            w, off = ctx.plan_uniform(3, N, opts).encode(dev(ctx, x)).to_numpy()
            dw, doff = ctx.plan_uniform(3, N, (m, L)).encode(dev(ctx, x)).to_numpy()
            assert np.array_equal(off, doff) and np.array_equal(w, dw), (name, L)


# ---- the parallel inverse (drx_iir.hip, and inside the block decoder drx_blocks.hip): up to four taps, lead +-1 --------------

EXTREME = {"x_half": (1, 32767, -32768, 65535), "x_i32": (-1, 70000, F.I32_MIN, F.I32_MAX), "x_i32_lead1": (1, F.I32_MAX, F.I32_MIN, 65536)}
PARALLEL = {**{n: t for n, t in F.FILTERS.items() if fast_decode(t)}, **EXTREME}
# (chunks, waveforms per chunk, WaveformLength): the smallest the existing tests take each form at (test_gpu_long_filters.py)
SEPARATE_SHAPES = [(1, 2, 8192), (1, 3, 8193), (1, 3, 24577), (1, 2, 32768 + 100)]
FUSED_SHAPES = [(2, 800, 9001), (2, 1600, 3000)]


@functools.lru_cache(maxsize=4)
def long_data(kind, n):
    if kind == "rails":  # a third each: all -32768, all 32767, alternating
        x = np.full(n, -32768, np.int16)
        x[n // 3:2 * (n // 3)] = 32767
        x[2 * (n // 3) + 1::2] = 32767
        return x
    return F.make_data(kind, n)


@pytest.mark.parametrize("name", list(PARALLEL))
def test_parallel_inverse(ctx, O, name):
    """Run tables are powers of the filter's companion matrix over Z / 2^16: coefficients near 2^15 and 2^31 with full-range
    samples.  Each form against x, against the lane-per-waveform decoder, and (first two shapes of the separate pass, first of
    the fused one) the encoder against the oracle's bytes."""
    taps = PARALLEL[name]
    assert "identity_mod" in PARALLEL and "half_range" in PARALLEL
    try:
        for fused, shapes in ((False, SEPARATE_SHAPES), (True, FUSED_SHAPES)):
            for si, (n_chunks, W, L) in enumerate(shapes):
                N = W * L - (L // 3 if W > 2 else 0)  # a shorter last waveform where there is room for one
                for kind in ("uniform", "rails"):
                    what = (name, n_chunks, W, L, kind)
                    x = long_data(kind, n_chunks * N)
                    xd = dev(ctx, x)
                    opts = F.opts_of(8, L, taps)
                    plan = ctx.plan_uniform(n_chunks, N, opts)
                    enc = plan.encode(xd)
                    if si < (1 if fused else 2):
                        ref_w, ref_off = O.encode_batch(x, N, opts)
                        w, off = enc.to_numpy()
                        assert np.array_equal(off, ref_off) and np.array_equal(w, ref_w), what
                    if name == "identity_mod" and not fused:  # (1, 65536): the residuals are the samples themselves
                        w1, off1 = ctx.plan_uniform(n_chunks, N, (8, L, 1, 1)).encode(xd).to_numpy()
                        w, off = enc.to_numpy()
                        assert np.array_equal(off, off1) and np.array_equal(w, w1), what
                    outs = {}
                    for flags in (0, D.DBG_NO_LONG_PATHS) + ((D.DBG_IIR_SEPARATE,) if fused else ()):
                        ctx.set_option("debug_flags", flags)
                        outs[flags] = plan.decode(enc)
                        path = plan.last_decode_path()
                        ctx.set_option("debug_flags", 0)
                        if flags == D.DBG_NO_LONG_PATHS:
                            assert path & LANES_ANY and not path & (D.PATH_BLOCKS | D.PATH_SIMPLE), (what, path)
                        elif fused and flags == 0:
                            assert path & D.PATH_BLOCKS and path & D.PATH_IIR_FUSED and not path & D.PATH_IIR, (what, path)
                        else:
                            assert path & D.PATH_BLOCKS and path & D.PATH_IIR and not path & D.PATH_IIR_FUSED, (what, path)
                    for flags, y in outs.items():
                        assert torch.equal(y, xd), (what, flags)
                        assert torch.equal(y, outs[D.DBG_NO_LONG_PATHS]), (what, flags)
                    plan.close()
    finally:
        ctx.set_option("debug_flags", 0)


# ---- a ragged plan ---------------------------------------------------------------------------------------------------------

def test_ragged_plan(ctx, O):
    """The ragged geometry of test_gpu_routes.BATCHES under a 64-tap filter and under (-3, 2, 2): bytes per chunk, decode and
    select against the oracle."""
    from test_gpu_routes import BATCHES
    Ns, Ls = BATCHES["ragged"][0], BATCHES["ragged"][1]
    x = np.concatenate([F.make_data(kind, n) for kind, n in zip(("gauss50", "uniform", "steps", "gauss50", "rails_alternating", "uniform"), Ns)])
    at = np.concatenate([[0], np.cumsum(Ns)])
    for taps in (F.FILTERS["t64_lead1_mag200"], (-3, 2, 2)):
        copts = [F.opts_of(8, L if L else n, taps) for n, L in zip(Ns, Ls)]
        words = [O.encode_chunk(x[at[c]:at[c + 1]], copts[c]) for c in range(len(Ns))]
        want = np.concatenate([O.decode_chunk(w, o) for w, o in zip(words, copts)])
        if F.lossless(taps):
            assert np.array_equal(want, x)
        plan = ctx.plan(Ns, Ls, 8, taps=taps)
        enc = plan.encode(dev(ctx, x))
        for c in range(len(Ns)):
            assert enc.chunk_bytes(c) == words[c].tobytes(), (taps[:3], c)
        assert (plan.last_encode_path() == D.ENC_TWO_PASS) == (len(taps) > 4), plan.last_encode_path()
        y = plan.decode(enc).cpu().numpy()
        assert plan.last_decode_path() == D.PATH_SIMPLE
        assert np.array_equal(y, want), taps[:3]
        waves = [(int(at[c]) + s, n) for c in range(len(Ns)) for s, n in F.waveforms(Ns[c], Ls[c])]
        ends = np.cumsum([len(F.waveforms(n, L)) for n, L in zip(Ns, Ls)]) - 1  # every chunk's last waveform
        sel = np.concatenate([[0], ends, ends, np.random.default_rng(9).integers(0, len(waves), 27)])
        rows = plan.decode_select(enc, sel).cpu().numpy()
        assert plan.last_decode_path() == D.PATH_SELECT
        for i, g in enumerate(sel):
            s, n = waves[g]
            assert np.array_equal(rows[i, :n], want[s:s + n]) and not rows[i, n:].any(), (taps[:3], i, int(g))
        plan.close()
