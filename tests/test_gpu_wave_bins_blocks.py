"""GPU: drx_wave_bins for few long waveforms under the context option "bins_impl" = 1 -- a workgroup per block of a waveform's
stream (csrc/drx_bins_blocks.hip, csrc/drx_blocks_bins.inc).

The batches that drx_wave_stats gives to its block form take that form; drx_plan_last_bins_form says which form ran,
drx_plan_last_decode_path keeps saying DRX_PATH_BINS alone.  The streams are the oracle's, the expected rows numpy's over the
oracle's input (tests/wave_bins_reference.py), the comparison torch.equal on all four columns of every row, by the walk and by
the side-band.  Every test leaves bins_impl and debug_flags at 0.

Shapes are small: a waveform of a few blocks (a block holds some 4 000 to 19 000 samples) meets every path a long one meets.
The default shape is 2 chunks x 3 waveforms of 24 000 samples, the last of each chunk a third shorter."""
import types

import numpy as np
import pytest

import block_cells as bc
from deltarice_amd import _lib as D
from test_gpu_noise_levels import LEVELS, noise
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, header_table
from test_gpu_wave_bins import I64_MAX, I64_MIN, data_of, plateau_rows
from test_gpu_wave_stats_blocks import crafted
from wave_bins_reference import default_n_bins, wave_bins
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANES, BLOCKS, ALL = D.BINS_FORM_LANES, D.BINS_FORM_BLOCKS, D.BINS_FORM_FALLBACK_ALL
L0 = 24000
SHAPE = ([2 * L0 + (L0 - L0 // 3)] * 2, [L0] * 2)


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.set_option("bins_impl", 0)
    c.set_option("debug_flags", 0)
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def bins_of(L):
    return (1, 7, 16, 17, 64, 250, 1000, 4999, L - 1, L, L + 1, 1 << 31)


def check(ctx, st, y, bin, n_bins, start=None, offset=0, form=BLOCKS, what="", flags=0, listed=None, sidebands=(False, True), impl=1):
    """One (bin, n_bins, origin) x {walk, side-band} on st under bins_impl `impl` and `flags` against numpy over the samples y;
    the path and the form of every call.  listed: a predicate over drx_plan_last_bins_listed (default: anything from 0 to
    total_waves; the count goes into the message).  Returns the listed counts."""
    plan = st.plan
    ask, n_bins = n_bins, default_n_bins(st.Ns, st.Ls, bin, offset) if n_bins is None else n_bins
    want = wave_bins(y, st.Ns, st.Ls, bin, n_bins, None if start is None else start.cpu().numpy(), offset)
    want = torch.from_numpy(want).to(ctx.device)
    seen = []
    ctx.set_option("bins_impl", impl)
    ctx.set_option("debug_flags", flags)
    try:
        for sideband in sidebands:
            got = plan.wave_bins(st.enc, bin, ask, start=start, offset=offset, wave_words=st.table if sideband else None)
            k = plan.last_bins_listed()
            seen.append(k)
            cell = (what, impl, flags, bin, n_bins, offset, sideband, "listed", k)
            assert plan.last_decode_path() == D.PATH_BINS, cell
            assert plan.last_bins_form() == form, (cell, plan.last_bins_form())
            assert (listed(k) if listed else 0 <= k <= plan.total_waves) and (form != LANES or k == 0), cell
            assert got.dtype == torch.int64 and got.shape == want.shape, cell
            if not torch.equal(got, want):
                bad = torch.nonzero((got != want).any(dim=2))
                g, b = (int(v) for v in bad[0])
                raise AssertionError((cell, f"{bad.shape[0]} rows differ; row ({g}, {b})", got[g, b].tolist(), want[g, b].tolist()))
    finally:
        ctx.set_option("bins_impl", 0)
        ctx.set_option("debug_flags", 0)
    return seen


def stream_of(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    return Stream(ctx, O, x, Ns, Ls, m, taps), x


def origins_of(ctx, st, lo, hi, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, st.plan.total_waves)).to(ctx.device)


# --------------------------------------------------------------------------- the merge regimes, from the geometry model
def regimes_of(O, x, Ns, Ls, m, bin, n_bins):
    """The merge regimes (1: one bin per block, 2: the LDS table, 3: more bins than the table holds) that the FIRST block of
    waveform 0 provably takes at origin 0, from tests/block_cells.py's model of the block geometry: the block holds the codes
    that start in its lanes x words-per-lane stream words, so its sample count follows from the code lengths; the table holds
    (words of the block's image or of its staging buffer) / 6 entries, and the smaller and the larger of the two bound it."""
    k = m.bit_length() - 1
    cell = types.SimpleNamespace(Ns=Ns, Ls=Ls, k=k, m=m)
    words = np.concatenate([O.encode_chunk(x[sum(Ns[:c]):sum(Ns[:c + 1])], (m, Ls[c])) for c in range(len(Ns))])
    sw = bc.blk_segw_bits10(bc.blk_bits10(int(words.size), int(sum(Ns))))
    L = Ls[0] or Ns[0]
    lanes = bc.nt_for_len(L, k)
    bits, wave = bc.code_lengths(x, cell)
    d0 = int(x[0])
    z0 = ((d0 << 1) ^ (d0 >> 15)) & 0xFFFF
    first = (z0 >> k) + 1 + k if (z0 >> k) < 8 else 25
    starts = np.concatenate(([0], first + np.concatenate(([0], np.cumsum(bits[wave == 0])))))[:L]  # bit at which each code starts
    S = int((starts < 32 * lanes * sw).sum())  # samples of the first block
    met = min(-(-S // bin), n_bins)
    cap_lo = min((lanes * sw + 16) // 6, lanes * (bc.blk_lane_cap(sw) // 2 + 1) // 6)
    cap_hi = max((lanes * sw + 16) // 6, lanes * (bc.blk_lane_cap(sw) // 2 + 1) // 6)
    if met == 1:
        return {1}
    if 2 <= met <= cap_lo:
        return {2}
    return {3} if met > cap_hi else set()


# --------------------------------------------------------------------------- 1. which batches take which form
@pytest.mark.parametrize("name,form", [("long-2", BLOCKS), ("long-40", BLOCKS), ("whole-chunk", BLOCKS),
                                       ("stream-quiet", LANES), ("short", LANES), ("fir4", LANES)])
def test_forms(ctx, O, name, form):
    import deltarice_amd as dr
    st, x = stream_of(ctx, O, name)
    W = st.plan.total_waves
    try:
        assert st.plan.last_bins_form() == 0  # no binned-statistics call yet
        check(ctx, st, x, 1000, None, None, 0, form, what=name)
        if name == "long-2":
            start = origins_of(ctx, st, -1000, 51001, 22)
            check(ctx, st, x, 4999, 12, start, 0, BLOCKS, what=name)
            for flags in (D.DBG_BINS_LANES, D.DBG_NO_LONG_PATHS, D.DBG_LONG_NOT_BLOCKS):
                check(ctx, st, x, 1000, None, None, 0, LANES, what=name, flags=flags)
            for bin, n_bins, origin in ((1000, None, None), (4999, 12, start), (50000, 1, None)):
                check(ctx, st, x, bin, n_bins, origin, 0, BLOCKS | ALL, what=name, flags=D.DBG_BINS_ALL_FALLBACK, listed=lambda k: k == W)
            check(ctx, st, x, 1000, None, None, 0, BLOCKS, what=name)
            check(ctx, st, x, 1000, None, None, 0, LANES, what=name, impl=0)
            for bad in (2, -1):
                with pytest.raises(dr.DeltaRiceError) as e:
                    ctx.set_option("bins_impl", bad)
                assert e.value.status == 1, bad
            check(ctx, st, x, 1000, None, None, 0, BLOCKS, what=(name, "behind the refused values"))
    finally:
        ctx.set_option("bins_impl", 0)
        ctx.set_option("debug_flags", 0)
        st.plan.close()


# --------------------------------------------------------------------------- 2. bins x origins x n_bins on the default shape
KINDS = ["sigma-10", "sigma-400", "ramp", "constant", "alternating"]


@pytest.mark.parametrize("kind", KINDS)
def test_bins_origins_and_counts(ctx, O, kind):
    Ns, Ls = SHAPE
    x = data_of(kind, sum(Ns))
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, W = st.plan, st.plan.total_waves
    try:
        rng = np.random.default_rng(11)
        stats = plan.wave_stats(st.enc)
        ends = torch.tensor([I64_MIN, I64_MAX] * (W // 2), dtype=torch.int64, device=ctx.device)
        origins = {
            "none": (None, (0,)),
            "random": (torch.from_numpy(rng.integers(-300, L0 + 301, W)).to(ctx.device), (0,)),
            "argmax": (stats[:, D.STAT_ARGMAX], (-64,)),  # the column as it is: a stride of 8
            "int64 ends": (ends, (-1, 1)),
        }
        assert origins["argmax"][0].stride(0) == D.STAT_COLS
        listed = []
        for bin in bins_of(L0):
            for oname, (start, offsets) in origins.items():
                for offset in offsets:
                    full = default_n_bins(Ns, Ls, bin, offset)
                    for n_bins in sorted({1, max(full * 2 // 5, 1), full + 5}) + [None]:  # (stops mid-waveform; None: the default)
                        listed += check(ctx, st, x, bin, n_bins, start, offset, BLOCKS, what=(kind, oname, "listed so far", sum(listed)))
    finally:
        plan.close()


def test_the_sweep_meets_every_merge_regime(O):
    """CPU work only (in this module for the sweep's own tables): the (kind, bin) cells of the sweep above hold, at origin 0 and
    the default n_bins, a first block in one bin, one in a handful of bins, and one in more bins than the table holds."""
    Ns, Ls = SHAPE
    seen = {}
    for kind in ("sigma-10", "sigma-400"):
        x = data_of(kind, sum(Ns))
        for bin in bins_of(L0):
            for r in regimes_of(O, x, Ns, Ls, 8, bin, default_n_bins(Ns, Ls, bin)):
                seen.setdefault(r, []).append((kind, bin))
    assert set(seen) == {1, 2, 3}, seen
    assert any(b == 1000 for _, b in seen[2]) and any(b == 1 for _, b in seen[3]) and any(b == L0 for _, b in seen[1]), seen


# --------------------------------------------------------------------------- 3. the block geometries
def test_geometry_classes(ctx, O):
    """9 / 11 / 15 / 19 stream words per lane by the stream's bits per sample, and waveforms of one or two blocks (64 / 128
    lanes per block) in the outer classes: the eight streams of test_gpu_wave_stats_blocks.py::test_geometry_classes."""
    rng = np.random.default_rng(41)
    seen = set()
    shapes = [(sigma, m, 90000, [3 * 90000] * 2, [90000] * 2) for sigma, m in LEVELS]
    shapes += [(sigma, m, L, [7 * L - L // 3] * 3, [L] * 3) for sigma, m, L in [(1, 8, 5000), (2000, 2048, 4000), (1, 8, 12000), (2000, 2048, 9000)]]
    for sigma, m, L, Ns, Ls in shapes:
        x = noise(rng, sigma, sum(Ns))
        st = Stream(ctx, O, x, Ns, Ls, m)
        try:
            if L == 90000:
                bits = st.words.size * 32.0 / x.size
                seen.add(9 if bits < 5.4 else 11 if bits < 8.2 else 15 if bits < 11.7 else 19)
            start = origins_of(ctx, st, -300, L + 301, 43)
            for bin in (17, 1000, L):
                check(ctx, st, x, bin, None, start, 0, BLOCKS, what=(sigma, m, L))
        finally:
            st.plan.close()
    assert seen == {9, 11, 15, 19}, seen


# --------------------------------------------------------------------------- 4. more codes on a lane than its share
def test_quiet_stretches_take_the_second_parse(ctx, O):
    rng = np.random.default_rng(42)
    x = noise(rng, 200, 2 * 2 * 120000).reshape(4, 120000)
    x[:, 30000:70000] = 0
    x[1, 90000:] = 7
    x = np.ascontiguousarray(x).reshape(-1)
    st = Stream(ctx, O, x, [2 * 120000] * 2, [120000] * 2, 256)
    try:
        check(ctx, st, x, 10000, None, None, 0, BLOCKS, what="quiet stretches")     # borders at both ends of the zero stretch
        check(ctx, st, x, 250, None, None, 29900, BLOCKS, what="quiet stretches")   # ... and inside it, from just in front of it
        check(ctx, st, x, 1, 45000, None, 29990, BLOCKS, what="quiet stretches")    # ... and a bin per sample of it
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 5. streams that do not fall into step
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
        check(ctx, st, x, 1000, None, None, 0, BLOCKS, what=case)  # (exact whatever is listed: the count is in the message)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 6. crafted rows
def test_crafted_rows(ctx, O):
    x, _ = crafted()
    L = x.shape[1]
    flat = x.reshape(-1)
    st = Stream(ctx, O, flat, [2 * L] * 2, [L] * 2, 8)
    try:
        start = origins_of(ctx, st, -300, L + 301, 51)
        for bin in (16, 1000, 50000):
            check(ctx, st, flat, bin, None, None, 0, BLOCKS, what="crafted")
            check(ctx, st, flat, bin, None, start, 0, BLOCKS, what="crafted")
        want = wave_bins(flat, st.Ns, st.Ls, 50000, 1)
        assert want[2].tolist() == [[-32768 * L, L << 30, -32768, -32768]] and want[3, 0, 2:].tolist() == [-32768, 32767]
    finally:
        st.plan.close()


def test_plateau_rows_narrow_to_wide(ctx, O):
    """Sixteen squares of +-16384 sum to 2^32, which a 32-bit chain returns as 0: the rows of
    test_gpu_wave_bins.py::test_bins_and_stats_narrow_to_wide as they are -- 30 waveforms of 700, a lane per waveform under
    either bins_impl -- and stretched to 24 000 samples (the quiet part repeated in front), which the blocks take: there the
    plateau lies inside one lane's share of a block."""
    x = plateau_rows()
    W, L = x.shape
    st = Stream(ctx, O, x.reshape(-1), [W * L], [L], 8)
    try:
        for bin in (16, 250):
            check(ctx, st, x.reshape(-1), bin, None, None, 0, LANES, what="plateaus")
    finally:
        st.plan.close()
    rng = np.random.default_rng(19)
    long = rng.normal(0, 10, (6, L0)).astype(np.int16)
    for r in range(6):
        at = 1000 + 3777 * r
        long[r, at:at + L] = x[6 * (r % 5) + r]  # a row of every plateau value but one twice
    sq = (long.astype(np.int64) ** 2)[:, :L0 // 16 * 16].reshape(6, -1, 16).sum(axis=2)
    assert (sq == 1 << 32).any()
    st = Stream(ctx, O, long.reshape(-1), [3 * L0] * 2, [L0] * 2, 8)
    try:
        start = origins_of(ctx, st, -40, L0, 18)
        for bin in (16, 17, 64, 250, L0):
            check(ctx, st, long.reshape(-1), bin, None, None, 0, BLOCKS, what="long plateaus")
            check(ctx, st, long.reshape(-1), bin, None, start, 0, BLOCKS, what="long plateaus")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. a ragged plan of long waveforms
def test_ragged_long_batch(ctx, O):
    Ns, Ls = [2048 * 5 + 9, 30000 * 3, 150001, 9001 * 4 - 3000], [2048, 30000, 0, 9001]
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    W = st.plan.total_waves
    try:
        per_wave_L = np.array([L or N for N, L in zip(Ns, Ls)], np.int64)[st.chunk]
        start = torch.from_numpy(np.random.default_rng(61).integers(-300, per_wave_L + 301)).to(ctx.device)
        for bin in (100, 2048, 9001):
            check(ctx, st, x, bin, None, None, 0, BLOCKS, what="ragged")
            check(ctx, st, x, bin, 40, start, -64, BLOCKS, what="ragged")
        check(ctx, st, x, 2048, None, start, 0, BLOCKS | ALL, what="ragged", flags=D.DBG_BINS_ALL_FALLBACK, listed=lambda k: k == W)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 8. where the buffers lie
def test_placements(ctx, O):
    st, x = stream_of(ctx, O, "long-2")
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    bin, n_bins, offset = 4999, 12, -100
    stride = n_bins * D.BIN_COLS + 3  # odd: the rows of every other waveform are 16-byte aligned, the others are not
    start_np = np.random.default_rng(8).integers(-1000, 51001, W)
    want = torch.from_numpy(wave_bins(x, st.Ns, st.Ls, bin, n_bins, start_np, offset)).to(ctx.device)
    ctx.set_option("bins_impl", 1)
    try:
        for pname, P in PLACEMENTS.items():  # the words at byte offsets 0, 4, 8 and 12
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(st.Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            for sstride in (1, 8):
                sw = window((W - 1) * sstride + 1, torch.int64, 8 - P["off"], fill=0x5A5A, device=ctx.device)
                sw.t[::sstride].copy_(torch.from_numpy(start_np))
                for obyte in (8, 0):
                    for fill in (0x5A5A5A5A5A5A5A5A, -1):
                        sideband = fill == -1
                        yw = window((W - 1) * stride + n_bins * D.BIN_COLS, torch.int64, obyte, fill=fill, device=ctx.device)
                        assert yw.t.data_ptr() % 16 == obyte
                        args = (sw.t.data_ptr(), sstride, offset, bin, n_bins, yw.t.data_ptr(), stride)
                        if sideband:
                            launch = lambda: ctx._check(ctx.lib.drx_wave_bins_with_wave_words(  # noqa: E731
                                plan._h, ww.t.data_ptr(), total, ow.t.data_ptr(), st.table.data_ptr(), *args))
                        else:
                            launch = lambda: ctx._check(ctx.lib.drx_wave_bins(plan._h, ww.t.data_ptr(), total, ow.t.data_ptr(), *args))  # noqa: E731
                        run(ctx, plan, launch)
                        assert plan.last_decode_path() == D.PATH_BINS and plan.last_bins_form() == BLOCKS
                        padded = torch.full((W * stride,), fill, dtype=torch.int64, device=ctx.device)
                        padded[:yw.t.numel()] = yw.t
                        padded = padded.view(W, stride)
                        same = torch.equal(padded[:, :n_bins * D.BIN_COLS].reshape(W, n_bins, D.BIN_COLS), want)
                        gaps = bool((padded[:, n_bins * D.BIN_COLS:] == fill).all())
                        intact = yw.intact() and ow.intact() and ww.intact() and sw.intact()
                        assert same and gaps and intact, (pname, sstride, obyte, fill, "rows differ" * (not same), "gap written" * (not gaps),
                                                          "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
    finally:
        ctx.set_option("bins_impl", 0)
        plan.close()


# --------------------------------------------------------------------------- 9. verdicts
def test_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [3 * 40000], [40000]
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    bin, n_bins = 1000, 12  # the bins end at sample 12 000: every waveform is parsed to its end all the same
    want = torch.from_numpy(wave_bins(x, Ns, Ls, bin, n_bins)).to(ctx.device)
    w = st.words
    h1 = 1 + 1 + int(w[1])  # the header of waveform 1: behind the chunk's word, waveform 0's header and its payload
    n1 = int(w[h1])

    def batch_of(words):
        off = torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device)
        return dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), off, int(words.size)), words

    def clean():
        assert torch.equal(plan.wave_bins(good, bin, n_bins), want)
        assert plan.last_decode_path() == D.PATH_BINS and plan.last_bins_form() == BLOCKS

    # a header one smaller, the payload's last word taken out (the chain stays consistent: the codes run past the payload)
    short = np.delete(w, h1 + n1)
    short[h1] = n1 - 1
    # a payload whose codes end one word early: a word of padding more, counted in the header
    early = np.insert(w, h1 + 1 + n1, np.uint32(0))
    early[h1] = n1 + 1
    # a broken chain
    chain = w.copy()
    chain[h1] += 1
    ctx.set_option("bins_impl", 1)
    try:
        clean()
        for cname, (enc, words) in {"header": batch_of(short), "payload": batch_of(early), "chain": batch_of(chain)}.items():
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.wave_bins(enc, bin, n_bins)
            assert e.value.status == 4, cname
            assert plan.last_bins_form() == BLOCKS, cname
            clean()  # the plan stays usable, and its next call starts clean
            if cname != "chain":  # ... and by the side-band (the table that belongs to that stream)
                table = torch.from_numpy(header_table(words, np.array([0, words.size]), Ns, Ls).view(np.int32)).to(ctx.device)
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.wave_bins(enc, bin, n_bins, wave_words=table)
                assert e.value.status == 4, cname
                clean()
    finally:
        ctx.set_option("bins_impl", 0)
        plan.close()


# --------------------------------------------------------------------------- 10. among the plan's other calls
def test_sequences_on_one_plan(ctx, O):
    Ns, Ls, m, _, _ = BATCHES["long-2"]
    taps = (1, -1, 1, -1)
    xs = [np.random.default_rng(70 + i).normal(0, 10 + 30 * i, sum(Ns)).astype(np.int16) for i in range(3)]
    sts = [Stream(ctx, O, x, Ns, Ls, m) for x in xs]
    fst = Stream(ctx, O, xs[1], Ns, Ls, m, taps)  # other samples under another filter
    plan = sts[0].plan  # every call below is made on this plan

    def bins(st, x, n_bins, form, finish=True, **kw):
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        got = plan.wave_bins_async(st.enc.words, st.enc.chunk_word_off, 1000, n_bins, in_words=st.enc.total_words, **kw)
        assert plan.last_bins_form() == form
        if finish:
            assert plan.finish() == 0 and plan.last_decode_path() == D.PATH_BINS
        return got, torch.from_numpy(wave_bins(x, Ns, Ls, 1000, n_bins)).to(ctx.device)

    def same(pair):
        assert torch.equal(*pair)

    ctx.set_option("bins_impl", 1)
    try:
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        assert plan.last_bins_form() == 0
        same(bins(sts[0], xs[0], 50, BLOCKS))
        assert torch.equal(plan.decode(sts[1].enc), sts[1].xd) and plan.last_decode_path() & D.PATH_BLOCKS  # (shares the block scratch)
        same(bins(sts[1], xs[1], 7, BLOCKS))
        want = torch.from_numpy(wave_stats_heads(xs[2], Ns, Ls, [100])[0]).to(ctx.device)
        assert torch.equal(plan.wave_stats(sts[2].enc, head=100), want) and plan.last_stats_form() == D.STATS_FORM_BLOCKS
        same(bins(sts[0], xs[0], 55, BLOCKS, wave_words=sts[0].table))
        plan.set_filter(taps)
        same(bins(fst, xs[1], 3, LANES))
        plan.set_filter(None)
        same(bins(sts[2], xs[2], 51, BLOCKS))
        # bins_impl 0 -> 1 -> 0 -> 1 on a plan that has made no block call yet (its list comes with its first block call and
        # stays): the option decides call by call
        other = sts[1].plan
        for impl, form in ((0, LANES), (1, BLOCKS), (0, LANES), (1, BLOCKS)):
            ctx.set_option("bins_impl", impl)
            got = other.wave_bins(sts[1].enc, 1000, 9)
            assert other.last_bins_form() == form and other.last_bins_listed() == 0
            assert torch.equal(got, torch.from_numpy(wave_bins(xs[1], Ns, Ls, 1000, 9)).to(ctx.device))
        # a chain without finish between the calls: the results of all of them, one verdict at the end
        pairs = [bins(st, x, n, BLOCKS, finish=False) for st, x, n in ((sts[0], xs[0], 50), (sts[1], xs[1], 13), (sts[2], xs[2], 50), (sts[0], xs[0], 1))]
        assert plan.finish() == 0 and plan.last_decode_path() == D.PATH_BINS
        for pair in pairs:
            same(pair)
    finally:
        ctx.set_option("bins_impl", 0)
        ctx.set_option("debug_flags", 0)
        for st in sts:
            st.plan.close()
        fst.plan.close()
