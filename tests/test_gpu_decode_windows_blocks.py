"""GPU: drx_decode_windows for few long waveforms -- a workgroup per block of a waveform's stream (drx_windows_blocks.hip).

The streams are the oracle's, the expected rows numpy's over the oracle's input (tests/decode_windows_reference.py), the
comparison torch.equal.  Every cell asserts DRX_PATH_WINDOWS alone, plan.finish() == 0 and the form the call took, through the
walk and through the side-band.  Every output is filled before the call with a sentinel that is not the call's pad: three
kernels write a row of this form (the pads, the blocks, the lane kernel over the listed waveforms), and a row that one of them
leaves out must show."""
import copy

import numpy as np
import pytest

from decode_windows_reference import extents, windows_multi
from deltarice_amd import _lib as D
from find_pulses_reference import ARGPEAK, START, WIDTH, find_pulses
from test_gpu_decode_windows import check, dev, prefilled, random_starts
from test_gpu_find_pulses_blocks import L2, crafted
from test_gpu_noise_levels import LEVELS, noise
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, expected_rows, header_table

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS, ALL = D.WINDOWS_FORM_LANES, D.WINDOWS_FORM_BLOCKS, D.WINDOWS_FORM_FALLBACK_ALL
CAP = D.PULSES_STAGE_CAP


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


def tiles(st, w, reverse=False):
    """[W, K] starts: windows of w samples side by side over the longest waveform, first to last or last to first"""
    K = -(-int(st.length.max()) // w)
    t = np.broadcast_to(np.arange(K, dtype=np.int64) * w, (st.length.size, K))
    return np.ascontiguousarray(t[:, ::-1] if reverse else t)


def check_tiling(ctx, st, x, w, form, pad=-5, reverse=True, **kw):
    """A tiling of every waveform against numpy, and its rows side by side against plan.decode() of the batch (pad behind a
    waveform's last sample)."""
    W = st.length.size
    decoded = st.plan.decode(st.enc)
    assert torch.equal(decoded, st.xd)
    t = tiles(st, w, reverse)
    want = expected_rows(decoded, st.start, st.length, np.arange(W), t.shape[1] * w, pad)
    for got in check(ctx, st, x, [(t, None, 0, w, pad)], form, **kw):
        assert torch.equal((got.flip(1) if reverse else got).reshape(W, -1), want), (w, reverse, kw.get("what"))


# --------------------------------------------------------------------------- 1. which batches take which form
@pytest.mark.parametrize("name,form", [("long-2", BLOCKS), ("whole-chunk", BLOCKS), ("stream-quiet", LANES), ("short", LANES), ("fir4", LANES)])
def test_forms(ctx, O, name, form):
    st, x = stream_of(ctx, O, name)
    try:
        assert st.plan.last_windows_form() == 0 and st.plan.last_windows_listed() == 0  # no such call yet
        if BATCHES[name][3] is not None:  # (a filter whose lead is +-1: the samples come back as they went in)
            assert torch.equal(st.plan.decode(st.enc), st.xd)
        cases = sorted_cases(np.random.default_rng(1), st)
        check(ctx, st, x, cases, form, what=name, listed=0)  # (Gaussian noise is never flagged; the lane form lists nothing)
        if name == "long-2":
            for flag in (D.DBG_WINDOWS_LANES, D.DBG_NO_LONG_PATHS, D.DBG_LONG_NOT_BLOCKS):
                check(ctx, st, x, cases[:1], LANES, flags=flag, what=name, listed=0)
            check(ctx, st, x, cases, BLOCKS | ALL, flags=D.DBG_WINDOWS_ALL_FALLBACK, what=name, listed=st.plan.total_waves)
            check(ctx, st, x, cases[:1], BLOCKS, flags=D.DBG_PULSES_LANES, what=name)  # (the pulse call's flag, not this call's)
            check(ctx, st, x, cases[:1], BLOCKS, what=name, listed=0)
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
    forward = np.broadcast_to(np.arange(K, dtype=np.int64) * w, (W, K))
    for starts in (forward, forward[:, ::-1]):
        sd = dev(ctx, starts, np.int64)
        for sideband in (False, True):
            got = st.plan.decode_windows(st.enc, sd, w, pad=-5, out=prefilled(ctx, (W, K, w), -5), wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_WINDOWS and st.plan.last_windows_form() == BLOCKS and st.plan.finish() == 0
            assert st.plan.last_windows_listed() == 0
            if starts is not forward:
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
                    got = st.plan.decode_windows(st.enc, starts, 256, count=gn, offset=-64, out=prefilled(ctx, want.shape, 0),
                                                 wave_words=st.table if sideband else None)
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
            got = plan.decode_windows(good, sd[k], width, pad=-1, out=prefilled(ctx, want[k].shape, -1))
            assert torch.equal(got, want[k]) and plan.last_decode_path() == D.PATH_WINDOWS and plan.last_windows_form() == BLOCKS
            assert plan.last_windows_listed() == 0  # (noise: no waveform goes to the lane kernel)

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
                # damaged behind its last window: the rows are right and the verdict is the lane form's -- the blocks, which parse
                # every waveform to its end, judge the damaged one suspect: it is listed, the two others are not, and its rows
                # are the lane kernel's
                got = plan.decode_windows(enc, sd["inside"], width, pad=-1, out=prefilled(ctx, want["inside"].shape, -1), **kw)
                assert plan.finish() == 0 and plan.last_windows_form() == BLOCKS, (cname, sorted(kw))
                assert torch.equal(got, want["inside"]), (cname, sorted(kw))
                assert 1 <= plan.last_windows_listed() < 3, (cname, sorted(kw), plan.last_windows_listed())
                # damaged inside a window
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.decode_windows(enc, sd["end"], width, pad=-1, **kw)
                assert e.value.status == 4 and plan.last_windows_form() == BLOCKS, (cname, sorted(kw))
                assert 1 <= plan.last_windows_listed() < 3, (cname, sorted(kw), plan.last_windows_listed())
                clean()  # the plan stays usable, and its next call starts clean
    finally:
        plan.close()


# --------------------------------------------------------------------------- 7. the block geometries
def test_geometry_classes(ctx, O):
    """9 / 11 / 15 / 19 stream words per lane by the stream's bits per sample, and waveforms of one or two blocks (64 / 128
    lanes per block) in the outer classes: windows all over every waveform, and a tiling whose rows are the decoded batch."""
    rng = np.random.default_rng(41)
    seen = set()
    for sigma, m in LEVELS:
        x = noise(rng, sigma, 2 * 3 * 90000)
        st = Stream(ctx, O, x, [3 * 90000] * 2, [90000] * 2, m)
        try:
            bits = st.words.size * 32.0 / x.size
            seen.add(9 if bits < 5.4 else 11 if bits < 8.2 else 15 if bits < 11.7 else 19)
            check(ctx, st, x, sorted_cases(rng, st), BLOCKS, what=(sigma, m), listed=0)
            check_tiling(ctx, st, x, 333, BLOCKS, what=(sigma, m), listed=0)
        finally:
            st.plan.close()
    assert seen == {9, 11, 15, 19}, seen
    for sigma, m, L in [(1, 8, 5000), (2000, 2048, 4000), (1, 8, 12000), (2000, 2048, 9000)]:
        N = 7 * L - L // 3
        x = noise(rng, sigma, 3 * N)
        st = Stream(ctx, O, x, [N] * 3, [L] * 3, m)
        try:
            check(ctx, st, x, sorted_cases(rng, st), BLOCKS, what=(sigma, m, L), listed=0)
            check_tiling(ctx, st, x, 333, BLOCKS, what=(sigma, m, L), listed=0)
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 8. more codes on a lane than its share
def test_second_parse(ctx, O):
    """A stretch of 170 000 samples with a step of one count every 500 samples, inside noise of sigma 2, at RiceParameter 2.  A
    sample that repeats the one before costs 2 bits there (a zero quotient and one remainder bit), a step 3, and the fall of
    39 counts that comes every 20 000 samples 40.  A lane of the block scheme holds at least 9 stream words = 288 bits (the
    smallest of the classes 9 / 11 / 15 / 19), so inside the stretch a lane of any class holds at least (288 - 40) / 3 = 82
    codes and nearly always 288 / 2 = 144 -- above 76, the largest
    share of the staging buffer a lane has: every block inside the stretch decodes again from its lanes' first codes, in
    passes of kOutCap = 256 x 76 = 19 456 samples, and a block there holds more samples than one pass (256 lanes x 144).  No
    counter reports the second parse: this reasoning is what says that it runs.  The steps make a misplaced sample show."""
    L, q0, q1 = 240000, 30000, 200000
    rng = np.random.default_rng(42)
    x = noise(rng, 2, 2 * 2 * L).reshape(4, L)
    i = np.arange(q0, q1)
    for g in range(4):
        x[g, q0:q1] = ((i + 125 * g) // 500) % 40 - 20  # (the steps of the four waveforms at different samples)
    x = np.ascontiguousarray(x).reshape(-1)
    st = Stream(ctx, O, x, [2 * L] * 2, [L] * 2, 2)
    W = 4
    try:
        bits = (st.table.cpu().numpy().astype(np.int64) * 32).sum() / x.size
        assert bits < 5.4  # the class of 9 words per lane
        for reverse in (False, True):
            check_tiling(ctx, st, x, 1000, BLOCKS, reverse=reverse, what="second parse, tiling", listed=0)
        g = np.arange(W)[:, None]
        cases = [
            # astride the stretch's beginning and its end
            (np.array([[q0 - 100, q1 - 100]] * W) - 7 * g, None, 0, 256, -1),
            # one window over the whole stretch: wider than a pass, and than a block
            (np.full((W, 1), q0 - 500) - 3 * g, None, 0, q1 - q0 + 1000, 9),
            # sparse windows that lie inside the stretch alone, each astride a step, sorted and with counts; and unsorted
            (np.array([[50000, 90000, 120030, 180000]] * W) - 125 * g - 32, np.array([4, 2, 0, 5]), 0, 64, -1),
            (np.array([[180000, 50000, 120030, 90000]] * W) - 125 * g - 3, None, 0, 7, 0),
        ]
        assert q1 - q0 + 1000 > 256 * 76
        check(ctx, st, x, cases, BLOCKS, what="second parse", listed=0)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 9. streams that do not fall into step
def test_listed_waveforms(ctx, O, long2):
    """The waveforms that the block parse flags are written again, all their rows, by the lane kernel over a list:
    plan.last_windows_listed() says how many.  Noise lists none; the debug flag lists all; the four patterns that statistics
    and pulses test as "streams that do not fall into step" list what they list (printed); a waveform damaged behind its last
    window is listed, and its sound neighbours are not."""
    import deltarice_amd as dr
    st, x = long2
    W = st.plan.total_waves
    cases = sorted_cases(np.random.default_rng(61), st)
    check(ctx, st, x, cases, BLOCKS, what="noise", listed=0)
    check(ctx, st, x, cases, BLOCKS | ALL, flags=D.DBG_WINDOWS_ALL_FALLBACK, what="noise", listed=W)
    check(ctx, st, x, cases[:1], LANES, flags=D.DBG_WINDOWS_LANES, what="noise", listed=0)
    n = 3 * 300000
    i = np.arange(n)
    patterns = {
        "slope 1 sawtooth": (i % 60000 - 30000),
        "square wave": np.where((i // 50) % 2 == 0, 100, -100),
        "alternating +-1": np.where(i % 2 == 0, 7, 8),
        "ramp with noise stretches": np.where((i // 40000) % 3 == 0, np.random.default_rng(46).normal(0, 10, n), i % 60000 - 30000),
    }
    seen = {}
    for case, v in patterns.items():
        y = np.ascontiguousarray(v).astype(np.int16)
        ps = Stream(ctx, O, y, [300000] * 3, [100000] * 3, 8)
        PW = ps.plan.total_waves
        try:
            seen[case] = []

            def record(k, into=seen[case]):
                into.append(k)
                return 0 <= k <= PW

            check(ctx, ps, y, sorted_cases(np.random.default_rng(62), ps), BLOCKS, what=case, listed=record)
            check_tiling(ctx, ps, y, 1000, BLOCKS, what=case, listed=record)
            check(ctx, ps, y, sorted_cases(np.random.default_rng(63), ps)[:1], BLOCKS | ALL, flags=D.DBG_WINDOWS_ALL_FALLBACK, what=case, listed=PW)
        finally:
            ps.plan.close()
    print("last_windows_listed() by pattern:", {k: sorted(set(v)) for k, v in seen.items()})
    # None of the four patterns lists a waveform under this call on an MI355X (every value recorded above was 0 when this test
    # was written), so the list that a call makes on its own is held to the case that must make one: test_verdicts' stream,
    # waveform 1 damaged behind its last window.  The blocks parse every waveform to its end and judge that one suspect; the
    # lane kernel over the list writes its rows again and judges it to e_g, where it is sound.
    Ns, Ls = [3 * 40000], [40000]
    z = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    vs = Stream(ctx, O, z, Ns, Ls, 8)
    try:
        w = vs.words
        h1 = 1 + 1 + int(w[1])  # the header of waveform 1
        n1 = int(w[h1])
        short = np.delete(w, h1 + n1)  # a header one smaller, the payload's last word taken out
        short[h1] = n1 - 1
        early = np.insert(w, h1 + 1 + n1, np.uint32(0))  # a word of padding more, counted in the header
        early[h1] = n1 + 1
        t = np.ascontiguousarray(np.broadcast_to(np.arange(30, dtype=np.int64)[::-1] * 1000, (3, 30)))  # tiles of samples [0, 30 000), last first
        cases = [(t, None, 0, 1000, -5), (np.array([[-70, 14000, 29000, 29500]] * 3), np.array([5, 4, 3]), 0, 333, -1)]
        for starts, counts, offset, width, _ in cases:
            assert (extents(Ns, Ls, starts, counts, offset, width) <= 30000).all()
        for cname, words in (("header", short), ("payload", early)):
            ds = copy.copy(vs)
            off = torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device)
            ds.enc = dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), off, int(words.size))
            ds.table = torch.from_numpy(header_table(words, np.array([0, words.size]), Ns, Ls).view(np.int32)).to(ctx.device)
            check(ctx, ds, z, cases, BLOCKS, what=("damaged behind its last window", cname), listed=lambda k: 1 <= k < 3)
        check(ctx, vs, z, cases, BLOCKS, what="the sound stream", listed=0)
    finally:
        vs.plan.close()


# --------------------------------------------------------------------------- 10. a ragged plan of long waveforms
def test_ragged_long_batch(ctx, O):
    Ns, Ls = [2048 * 5 + 9, 30000 * 3, 150001, 9001 * 4 - 3000], [2048, 30000, 0, 9001]
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    W = st.plan.total_waves
    try:
        assert torch.equal(st.plan.decode(st.enc), st.xd)
        assert st.plan.last_decode_path() & D.PATH_BLOCKS, st.plan.last_decode_path()  # (this shape: the block decoder's)
        cases = sorted_cases(np.random.default_rng(64), st)
        check(ctx, st, x, cases, BLOCKS, what="ragged", listed=0)
        check_tiling(ctx, st, x, 333, BLOCKS, what="ragged", listed=0)
        check(ctx, st, x, cases, BLOCKS | ALL, flags=D.DBG_WINDOWS_ALL_FALLBACK, what="ragged", listed=W)
        check_tiling(ctx, st, x, 333, BLOCKS | ALL, reverse=False, flags=D.DBG_WINDOWS_ALL_FALLBACK, what="ragged", listed=W)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 11. where the buffers lie
def test_placements(ctx, O):
    Ns, Ls = [3 * 20000] * 2, [20000] * 2
    rng = np.random.default_rng(9)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    K, width, offset, pad = 3, 50, -9, -2
    try:
        starts = np.sort(random_starts(rng, st, K), axis=1)
        counts = np.array([0, 3, 2, 4, 1, 3])  # a waveform without a live window, dead slots, a count above K
        want = torch.from_numpy(windows_multi(x, Ns, Ls, starts, counts, offset, width, pad)).to(ctx.device)
        # the starts as a column of wider records (the strides of drx_find_pulses' output), and at an address that is 8 mod 16
        records = torch.full((W, K, 5), 12345, dtype=torch.int64, device=ctx.device)
        records[:, :, 3] = dev(ctx, starts, np.int64)
        odd8 = window(W * K, torch.int64, 8, device=ctx.device)
        odd8.t.copy_(dev(ctx, starts, np.int64).reshape(-1))
        cw = window(W, torch.int32, 4, device=ctx.device)
        cw.t.copy_(dev(ctx, counts, np.int32))
        assert odd8.t.data_ptr() % 16 == 8 and cw.t.data_ptr() % 8 == 4
        givens = {"column": records[:, :, 3], "8 mod 16": odd8.t.view(W, K)}
        assert givens["column"].stride() == (5 * K, 5)
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            # (byte offset of d_out, samples between a waveform's rows, samples between waveforms beyond the least, pre-fill)
            for obyte, o_win, extra, fill, given in ((0, width, 0, 0x5A5A, "column"), (2, width + 1, 0, -1, "8 mod 16"), (6, width + 7, 3, 0x5A5A, "column"),
                                                     (14, width, 5, -1, "8 mod 16"), (10, width + 1, 1, 0x5A5A, "column")):
                o_wave = (K - 1) * o_win + width + extra
                yw = window((W - 1) * o_wave + (K - 1) * o_win + width, torch.int16, obyte, fill=fill, device=ctx.device)
                assert yw.t.data_ptr() % 16 == obyte
                # (the second pass: the lane kernel over the list writes every row again, and meets the same guards and gaps)
                for flags, form, listed in ((0, BLOCKS, 0), (D.DBG_WINDOWS_ALL_FALLBACK, BLOCKS | ALL, W)):
                    for sideband in (False, True):
                        yw.t.fill_(fill)
                        rows = None

                        def launch():
                            nonlocal rows
                            rows = plan.decode_windows_async(ww.t, ow.t, givens[given], width, count=cw.t, offset=offset, pad=pad, out=yw.t,
                                                             out_strides=(o_wave, o_win), in_words=total, wave_words=st.table if sideband else None)
                        ctx.set_option("debug_flags", flags)
                        try:
                            assert run(ctx, plan, launch) == 0
                        finally:
                            ctx.set_option("debug_flags", 0)
                        assert plan.last_decode_path() == D.PATH_WINDOWS and plan.last_windows_form() == form and plan.last_windows_listed() == listed
                        same = torch.equal(rows, want)
                        # everything that is not a row kept the pre-fill: the rows put back, the whole buffer is the pre-fill
                        rows.fill_(fill)
                        intact = yw.intact() and ow.intact() and ww.intact() and odd8.intact() and cw.intact() and bool((yw.t == fill).all())
                        assert same and intact, (pname, obyte, o_win, extra, fill, given, flags, sideband, "rows differ" * (not same),
                                                 "guard or gap written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
        assert bool((records[:, :, [0, 1, 2, 4]] == 12345).all())
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


# --------------------------------------------------------------------------- 12. more window slots than a block has threads
def test_many_slots(ctx, O, long2):
    """300 slots of 8 samples: the threads of a block (64, 128 or 256) test the live windows a stride apart, and only slots
    of the second or a later round meet the waveform -- slot 299 of every waveform and slot 257 of one; every other start lies
    far behind the waveform's end."""
    small = np.random.default_rng(65).normal(0, 1, 3 * 7 * 5000).astype(np.int16)
    sst = Stream(ctx, O, small, [7 * 5000] * 3, [5000] * 3, 8)
    try:
        for (st, x), what in ((long2, "long-2"), ((sst, small), "3 x 7 x 5000")):
            W = st.length.size
            rng = np.random.default_rng(66)
            starts = np.full((W, 300), 10 ** 9, np.int64) + rng.integers(0, 1000, (W, 300))
            starts[:, 299] = rng.integers(0, st.length - 8)
            g0 = W // 2
            starts[g0, 257] = rng.integers(0, st.length[g0] - 8)
            cut = np.where(np.arange(W) % 2 == 0, 299, 300)  # slot 299 cut off in every second waveform ...
            cut[g0] = 299  # ... and in the one whose slot 257 stays
            assert extents(st.Ns, st.Ls, starts, cut, 0, 8)[g0] == starts[g0, 257] + 8
            check(ctx, st, x, [(starts, None, 0, 8, -1), (starts, cut, 0, 8, 11)], BLOCKS, what=("many slots", what), listed=0)
    finally:
        sst.plan.close()


# --------------------------------------------------------------------------- 13. rows beyond 2^32 bytes
def test_rows_beyond_4_gib(ctx, O):
    L, K, width = 4000, 3, 40
    o_wave, o_win = (1 << 31) + 24, 1000  # a waveform's rows lie more than 2^31 samples behind the one before
    rng = np.random.default_rng(10)
    x = rng.normal(0, 10, 3 * L).astype(np.int16)
    st = Stream(ctx, O, x, [3 * L], [L], 8)
    try:
        try:
            out = torch.empty(2 * o_wave + (K - 1) * o_win + width, dtype=torch.int16, device=ctx.device)  # 8.6 GB, of which 9 rows are touched
        except (RuntimeError, MemoryError) as e:
            pytest.skip(f"no room for the output: {e}")
        assert out.numel() * 2 > 1 << 33
        starts = np.sort(random_starts(rng, st, K, -10, 10), axis=1)
        want = torch.from_numpy(windows_multi(x, st.Ns, st.Ls, starts, None, 0, width, -9)).to(ctx.device)
        for flags, form in ((0, BLOCKS), (D.DBG_WINDOWS_ALL_FALLBACK, BLOCKS | ALL)):
            for sideband in (False, True):
                rows = None

                def launch():
                    nonlocal rows
                    rows = st.plan.decode_windows_async(st.enc.words, st.enc.chunk_word_off, dev(ctx, starts, np.int64), width, pad=-9, out=out,
                                                        out_strides=(o_wave, o_win), in_words=st.enc.total_words,
                                                        wave_words=st.table if sideband else None)
                out.as_strided((3, K, width), (o_wave, o_win, 1)).fill_(0x5A5A)
                ctx.set_option("debug_flags", flags)
                try:
                    assert run(ctx, st.plan, launch) == 0 and st.plan.last_decode_path() == D.PATH_WINDOWS
                finally:
                    ctx.set_option("debug_flags", 0)
                assert st.plan.last_windows_form() == form
                assert torch.equal(rows, want), (flags, sideband)
        del out, rows
    finally:
        ctx.set_option("debug_flags", 0)
        st.plan.close()
        torch.cuda.empty_cache()


# --------------------------------------------------------------------------- 14. every sample as the only one a block stores
def test_every_sample_alone(ctx, O):
    """21 waveforms of the same 5000 samples: the same stream 21 times, cut into blocks at the same samples.  Call c gives
    waveform g one window of one sample at 21 c + g, so every sample of the waveform is once the only sample that any window
    of its waveform holds -- the first and the last sample of every block among them, wherever the blocks' borders lie."""
    L, W = 5000, 21
    one = np.clip(np.random.default_rng(67).normal(0, 3, L), -90, 90).astype(np.int16)  # (no sample is the pad)
    x = np.tile(one, W)
    st = Stream(ctx, O, x, [7 * L] * 3, [L] * 3, 8)
    try:
        tab = st.table.cpu().numpy()
        assert (tab == tab[0]).all()
        cases = [((21 * c + np.arange(W))[:, None], None, 0, 1, 99) for c in range(-(-L // W))]
        check(ctx, st, x, cases, BLOCKS, what="every sample alone", listed=0)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 15. among the plan's other calls
def test_sequences_on_one_plan(ctx, O):
    import deltarice_amd as dr
    from wave_stats_reference import wave_stats_heads
    st, x = stream_of(ctx, O, "long-2")
    plan, W, total = st.plan, st.plan.total_waves, st.enc.total_words
    taps = (1, -1, 1, -1)
    fst = Stream(ctx, O, x, st.Ns, st.Ls, 8, taps)  # the same samples under another filter ...
    fst.plan.close()
    fst = copy.copy(fst)
    fst.plan = plan  # ... on this plan
    cases = sorted_cases(np.random.default_rng(68), st)
    want_s = torch.from_numpy(wave_stats_heads(x, st.Ns, st.Ls, [100])[0]).to(ctx.device)
    tab = np.random.default_rng(58).integers(25, 55, W)  # 2.5 to 5.5 sigma: rows that overflow and rows without a pulse
    td = dev(ctx, tab, np.int64)

    def windows(form, s=st, flags=0, sidebands=(False,), listed=0):
        check(ctx, s, x, cases, form, flags=flags, sidebands=sidebands, what="sequence", listed=listed)

    def stats(enc, form):
        assert torch.equal(plan.wave_stats(enc, head=100), want_s)
        assert plan.last_stats_form() == form

    def pulses(mp):
        n, p = find_pulses(x, st.Ns, st.Ls, 0, 1, 1, mp, tab)
        return torch.from_numpy(n).to(ctx.device), torch.from_numpy(p).to(ctx.device)

    try:
        windows(LANES, flags=D.DBG_WINDOWS_LANES)  # (the block form's scratch does not exist yet)
        windows(BLOCKS)
        assert torch.equal(plan.decode(st.enc), st.xd) and plan.last_decode_path() & D.PATH_BLOCKS  # (shares the block scratch)
        assert plan.last_windows_listed() == 0  # (not this call's path)
        windows(BLOCKS)
        stats(st.enc, D.STATS_FORM_BLOCKS)
        windows(BLOCKS, sidebands=(True,))
        assert plan.last_stats_form() == D.STATS_FORM_BLOCKS and plan.last_pulses_form() == 0
        gn, gp = plan.find_pulses(st.enc, td, 1, 1, 3 * CAP)
        wn, wp = pulses(3 * CAP)
        assert plan.last_pulses_form() == D.PULSES_FORM_BLOCKS and torch.equal(gn, wn) and torch.equal(gp, wp)
        windows(BLOCKS)
        windows(BLOCKS | ALL, flags=D.DBG_WINDOWS_ALL_FALLBACK, listed=W)
        windows(BLOCKS)
        assert plan.last_stats_form() == D.STATS_FORM_BLOCKS and plan.last_pulses_form() == D.PULSES_FORM_BLOCKS
        plan.set_filter(taps)
        windows(LANES, s=fst, sidebands=(False, True))  # (the serial kernel)
        plan.set_filter(None)
        windows(BLOCKS, sidebands=(False, True))
        assert plan.last_stats_form() == D.STATS_FORM_BLOCKS and plan.last_pulses_form() == D.PULSES_FORM_BLOCKS
        # the device chain: the records and counts of find_pulses go into decode_windows as they lie on the device, with no
        # finish and no host read between the two launches
        wn, wp = pulses(4)
        assert (wn == 0).any() and (wn > 4).any()
        want = torch.from_numpy(windows_multi(x, st.Ns, st.Ls, wp[:, :, START].cpu().numpy(), wn.cpu().numpy(), -64, 256, 0)).to(ctx.device)
        for flags, form in ((0, BLOCKS), (D.DBG_WINDOWS_LANES, LANES)):
            for sideband in (False, True):
                out = prefilled(ctx, want.shape, 0)
                cn = torch.full((W,), 77, dtype=torch.int32, device=ctx.device)
                cp = torch.full((W * 4 * D.PULSE_COLS,), 77, dtype=torch.int64, device=ctx.device)
                ww = st.table if sideband else None
                ctx.set_option("debug_flags", flags)
                try:
                    ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
                    gn, gp = plan.find_pulses_async(st.enc.words, st.enc.chunk_word_off, td, 1, 1, 4, count=cn, out=cp, in_words=total, wave_words=ww)
                    rows = plan.decode_windows_async(st.enc.words, st.enc.chunk_word_off, gp[:, :, START], 256, count=gn, offset=-64, out=out,
                                                     in_words=total, wave_words=ww)
                    assert plan.finish() == 0
                finally:
                    ctx.set_option("debug_flags", 0)
                assert plan.last_decode_path() == D.PATH_WINDOWS and plan.last_windows_form() == form and plan.last_windows_listed() == 0
                assert plan.last_pulses_form() == D.PULSES_FORM_BLOCKS
                assert torch.equal(gn, wn) and torch.equal(gp, wp), (flags, sideband)
                assert torch.equal(rows, want), (flags, sideband)
        # a corrupt call, then the same arguments on the good stream: the status is clean and the rows are right
        header = st.words.copy()
        header[int(st.offs[1]) + 1] += 1  # the first waveform header of chunk 1: a broken chain
        broken = copy.copy(st)
        broken.enc = dr.EncodedBatch(torch.from_numpy(header.view(np.int32)).to(ctx.device), st.enc.chunk_word_off, st.enc.total_words)
        for starts, counts, offset, width, pad in cases:
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.decode_windows(broken.enc, dev(ctx, starts, np.int64), width, count=dev(ctx, counts, np.int32), offset=offset, pad=pad)
            assert e.value.status == 4 and plan.last_windows_form() == BLOCKS
            windows(BLOCKS)
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()
