"""GPU: drx_decode_windows for few long waveforms -- a workgroup per block of a waveform's stream (drx_windows_blocks.hip).

The streams are the oracle's, the expected rows numpy's over the oracle's input (tests/decode_windows_reference.py), the
comparison torch.equal.  Every cell asserts DRX_PATH_WINDOWS alone, plan.finish() == 0 and the form the call took, through the
walk and through the side-band."""
import numpy as np
import pytest

from decode_windows_reference import extents, windows_multi
from deltarice_amd import _lib as D
from find_pulses_reference import ARGPEAK, START, WIDTH, find_pulses
from test_gpu_decode_windows import check, dev
from test_gpu_find_pulses_blocks import L2, crafted
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, header_table

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS, ALL = D.WINDOWS_FORM_LANES, D.WINDOWS_FORM_BLOCKS, D.WINDOWS_FORM_FALLBACK_ALL


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


@pytest.fixture(scope="module")
def long2(ctx, O):
    st, x = stream_of(ctx, O, "long-2")
    yield st, x
    st.plan.close()


def sorted_cases(rng, st, K=4, width=256):
    """sorted starts all over the waveforms with counts, and unsorted ones without"""
    W = st.length.size
    starts = rng.integers(-100, st.length[:, None] + 100, (W, K))
    counts = rng.integers(0, K + 2, W)
    counts[0], counts[-1] = 0, K + 1
    return [(np.sort(starts, axis=1), counts, -64, width, -1), (starts, None, 0, width - 1, 7)]


# --------------------------------------------------------------------------- 1. which batches take which form
@pytest.mark.parametrize("name,form", [("long-2", BLOCKS), ("whole-chunk", BLOCKS), ("stream-quiet", LANES), ("short", LANES), ("fir4", LANES)])
def test_forms(ctx, O, name, form):
    st, x = stream_of(ctx, O, name)
    try:
        assert st.plan.last_windows_form() == 0  # no such call yet
        if BATCHES[name][3] is not None:  # (a filter whose lead is +-1: the samples come back as they went in)
            assert torch.equal(st.plan.decode(st.enc), st.xd)
        cases = sorted_cases(np.random.default_rng(1), st)
        check(ctx, st, x, cases, form, what=name)
        if name == "long-2":
            for flag in (D.DBG_WINDOWS_LANES, D.DBG_NO_LONG_PATHS, D.DBG_LONG_NOT_BLOCKS):
                check(ctx, st, x, cases[:1], LANES, flags=flag, what=name)
            check(ctx, st, x, cases, BLOCKS | ALL, flags=D.DBG_WINDOWS_ALL_FALLBACK, what=name)
            check(ctx, st, x, cases[:1], BLOCKS, flags=D.DBG_PULSES_LANES, what=name)  # (the pulse call's flag, not this call's)
            check(ctx, st, x, cases[:1], BLOCKS, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. tiling: the rows are the decoded batch
@pytest.mark.parametrize("w", [1000, 333])
def test_tiling_is_the_decode(ctx, long2, w):
    st, x = long2
    W, L = st.length.size, 50000
    K = -(-L // w)
    decoded = st.plan.decode(st.enc).view(W, L)
    assert torch.equal(decoded, st.xd.view(W, L))
    tiles = np.broadcast_to(np.arange(K, dtype=np.int64) * w, (W, K))
    for starts in (tiles, tiles[:, ::-1]):
        sd = dev(ctx, starts, np.int64)
        for sideband in (False, True):
            got = st.plan.decode_windows(st.enc, sd, w, pad=-5, wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.last_windows_form() == BLOCKS and st.plan.finish() == 0
            if starts is not tiles:
                got = got.flip(1)
            flat = got.reshape(W, K * w)
            assert torch.equal(flat[:, :L], decoded), (w, sideband)
            assert bool((flat[:, L:] == -5).all()), (w, sideband)


# --------------------------------------------------------------------------- 3. one window wider than the waveform
def test_wide_window(ctx, long2):
    st, x = long2
    W, L = st.length.size, 50000
    check(ctx, st, x, [(np.full((W, 1), -32), None, 0, L + 64, 99)], BLOCKS, what="wide")


# --------------------------------------------------------------------------- 4. the windows of drx_find_pulses' records
def test_windows_from_find_pulses(ctx, O):
    x = crafted()
    flat = np.ascontiguousarray(x).reshape(-1)
    Ns, Ls = [2 * L2] * 2, [L2] * 2
    st = Stream(ctx, O, flat, Ns, Ls, 8)
    try:
        # row 0: runs every 37 samples, row 1: one run over the whole row (a threshold below all of it), row 2: a square wave,
        # row 3: nothing over its threshold
        tab = np.array([100, int(x[1].min()) - 1, 100, 5000], np.int64)
        n, p = find_pulses(flat, Ns, Ls, 0, 1, 1, 8, tab)
        assert n[0] > 8 and n[2] > 8 and n[3] == 0
        assert n[1] == 1 and p[1, 0, START] + p[1, 0, WIDTH] == L2  # a pulse that ends at the last sample
        gn, gp = st.plan.find_pulses(st.enc, dev(ctx, tab, np.int64), 1, 1, 8)
        assert torch.equal(gn.cpu(), torch.from_numpy(n)) and torch.equal(gp.cpu(), torch.from_numpy(p))
        for col in (START, ARGPEAK):
            want = torch.from_numpy(windows_multi(flat, Ns, Ls, p[:, :, col], n, -64, 256, 0)).to(ctx.device)
            starts = gp[:, :, col]
            assert starts.stride() == (5 * 8, 5)
            for flags, form in ((0, BLOCKS), (D.DBG_WINDOWS_LANES, LANES)):
                ctx.set_option("debug_flags", flags)
                for sideband in (False, True):
                    got = st.plan.decode_windows(st.enc, starts, 256, count=gn, offset=-64, wave_words=st.table if sideband else None)
                    assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.last_windows_form() == form and st.plan.finish() == 0
                    assert torch.equal(got, want), (col, flags, sideband)
    finally:
        ctx.set_option("debug_flags", 0)
        st.plan.close()


# --------------------------------------------------------------------------- 5. sparse windows, and none
def test_sparse_and_none(ctx, long2):
    import deltarice_amd as dr
    st, x = long2
    W, L = st.length.size, 50000
    rng = np.random.default_rng(5)
    starts = rng.integers(L - 300, L - 256, (W, 2))
    one = np.ones(W, np.int64)
    check(ctx, st, x, [(starts, one, 0, 256, -1)], BLOCKS, what="one window in the last 300 samples")
    check(ctx, st, x, [(starts, np.zeros(W, np.int64), 0, 256, -1)], BLOCKS, what="no live window")
    # ... which must still validate the stream: a broken header chain is reported with every count 0
    header = st.words.copy()
    header[int(st.offs[1]) + 1] += 1
    broken = dr.EncodedBatch(torch.from_numpy(header.view(np.int32)).to(ctx.device), st.enc.chunk_word_off, st.enc.total_words)
    with pytest.raises(dr.DeltaRiceError) as e:
        st.plan.decode_windows(broken, dev(ctx, starts, np.int64), 256, count=dev(ctx, np.zeros(W), np.int32))
    assert e.value.status == 4 and st.plan.last_windows_form() == BLOCKS
    check(ctx, st, x, [(starts, one, 0, 256, -1)], BLOCKS, what="the plan stays usable")


# --------------------------------------------------------------------------- 6. verdicts
def test_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [3 * 40000], [40000]
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    w = st.words
    h1 = 1 + 1 + int(w[1])  # the header of waveform 1: behind the chunk's word, waveform 0's header and its payload
    n1 = int(w[h1])
    width = 256
    inside = np.array([[100, 20000, 30000]] * 3, np.int64)          # every window ends in front of sample 30 256
    to_the_end = np.array([[100, 20000, 40000 - 200]] * 3, np.int64)  # the last window reaches the last sample
    assert (extents(Ns, Ls, inside, None, 0, width) == 30256).all() and (extents(Ns, Ls, to_the_end, None, 0, width) == 40000).all()
    want = {k: torch.from_numpy(windows_multi(x, Ns, Ls, s, None, 0, width, -1)).to(ctx.device) for k, s in (("inside", inside), ("end", to_the_end))}
    sd = {"inside": dev(ctx, inside, np.int64), "end": dev(ctx, to_the_end, np.int64)}

    def batch_of(words):
        off = torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device)
        return dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), off, int(words.size)), words

    def clean():
        for k in ("inside", "end"):
            got = plan.decode_windows(good, sd[k], width, pad=-1)
            assert torch.equal(got, want[k]) and plan.last_decode_path() == D.PATH_WINDOWS and plan.last_windows_form() == BLOCKS

    # a header one smaller, the payload's last word taken out (the chain stays consistent: the codes run past the payload)
    short = np.delete(w, h1 + n1)
    short[h1] = n1 - 1
    # a payload whose codes end one word early: a word of padding more, counted in the header
    early = np.insert(w, h1 + 1 + n1, np.uint32(0))
    early[h1] = n1 + 1
    try:
        clean()
        for cname, (enc, words) in {"header": batch_of(short), "payload": batch_of(early)}.items():
            table = torch.from_numpy(header_table(words, np.array([0, words.size]), Ns, Ls).view(np.int32)).to(ctx.device)
            for kw in ({}, dict(wave_words=table)):
                # damaged behind its last window: the rows are right and the verdict is the lane form's
                got = plan.decode_windows(enc, sd["inside"], width, pad=-1, **kw)
                assert plan.finish() == 0 and plan.last_windows_form() == BLOCKS, (cname, sorted(kw))
                assert torch.equal(got, want["inside"]), (cname, sorted(kw))
                # damaged inside a window
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.decode_windows(enc, sd["end"], width, pad=-1, **kw)
                assert e.value.status == 4 and plan.last_windows_form() == BLOCKS, (cname, sorted(kw))
                clean()  # the plan stays usable, and its next call starts clean
    finally:
        plan.close()
