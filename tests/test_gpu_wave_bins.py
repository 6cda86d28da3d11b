"""GPU: drx_wave_bins, the lane and the serial kernels -- four exact statistics per bin of every waveform, parsed from the
encoded stream.

The streams are the oracle's (oracle.encode_chunk), the expected rows numpy's over the oracle's input
(tests/wave_bins_reference.py), the comparison torch.equal on all four columns of every row.  Every call is made by the walk
and by the side-band and asserts DRX_PATH_BINS alone and the form."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, geometry, header_table  # noqa: F401  (Stream builds its side-band with header_table)
from test_gpu_wave_stats import FILTERS, flipped_payload, samples_of
from wave_bins_reference import default_n_bins, wave_bins
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
L0 = 7000
SHAPE = ([43 * L0 + 3000] * 3, [L0] * 3)  # 44 waveforms per chunk -- two wavefronts and a partial one -- the last one of 3000 samples


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


def bins_of(L):
    return (1, 7, 16, 17, 64, 250, 1000, L - 1, L, L + 1, 1 << 31)


def check(ctx, st, y, bin, n_bins, start=None, offset=0, what=""):
    """One (bin, n_bins, origin) x {walk, side-band} on st against numpy over the samples y.  start: an int64 tensor on the
    device, any stride, or None.  n_bins None: the call's default, which covers the longest waveform from the offset."""
    plan = st.plan
    ask, n_bins = n_bins, default_n_bins(st.Ns, st.Ls, bin, offset) if n_bins is None else n_bins
    want = wave_bins(y, st.Ns, st.Ls, bin, n_bins, None if start is None else start.cpu().numpy(), offset)
    assert want.shape == (plan.total_waves, n_bins, D.BIN_COLS)
    want = torch.from_numpy(want).to(ctx.device)
    for sideband in (False, True):
        got = plan.wave_bins(st.enc, bin, ask, start=start, offset=offset, wave_words=st.table if sideband else None)
        cell = (what, bin, n_bins, offset, sideband)
        assert plan.last_decode_path() == D.PATH_BINS and plan.last_bins_form() == D.BINS_FORM_LANES and plan.last_bins_listed() == 0, cell
        assert got.dtype == torch.int64 and got.shape == want.shape, cell
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).any(dim=2))
            g, b = (int(v) for v in bad[0])
            raise AssertionError((cell, f"{bad.shape[0]} rows differ; row ({g}, {b})", got[g, b].tolist(), want[g, b].tolist()))


def data_of(kind, n):
    rng = np.random.default_rng(len(kind))
    if kind == "sigma-10":
        return rng.normal(0, 10, n).astype(np.int16)
    if kind == "sigma-400":
        return rng.normal(0, 400, n).astype(np.int16)
    if kind == "ramp":
        return (np.arange(n) + 30000).astype(np.uint16).view(np.int16)  # slope 1, through the int16 wrap
    if kind == "constant":
        return np.full(n, -1234, np.int16)
    assert kind == "alternating"  # +-32767: no group is narrow
    return np.where(np.arange(n) & 1, 32767, -32767).astype(np.int16)


# --------------------------------------------------------------------------- 1. bins x origins x n_bins on the delta filter
@pytest.mark.parametrize("kind", ["sigma-10", "sigma-400", "ramp", "constant", "alternating"])
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
        for bin in bins_of(L0):
            for oname, (start, offsets) in origins.items():
                for offset in offsets:
                    full = default_n_bins(Ns, Ls, bin, offset)
                    for n_bins in sorted({1, max(full * 2 // 5, 1), full + 5}) + [None]:  # (stops mid-waveform; None: the default)
                        check(ctx, st, x, bin, n_bins, start, offset, what=(kind, oname))
    finally:
        plan.close()


# --------------------------------------------------------------------------- 2. other geometries, a lane per waveform
GEOMETRIES = ("short", "ragged", "whole-chunk")


@pytest.fixture(scope="module")
def streams(ctx, O):
    """name -> (Stream, samples, per-waveform origins), built once and shared by the cases of a geometry"""
    made = {}

    def get(name):
        if name not in made:
            Ns, Ls, m, taps, sigma = BATCHES[name]
            x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
            st = Stream(ctx, O, x, Ns, Ls, m, taps)
            longest = st.plan.longest_wave()
            start = torch.from_numpy(np.random.default_rng(12).integers(-300, longest + 301, st.plan.total_waves)).to(ctx.device)
            made[name] = (st, x, start)
        return made[name]

    yield get
    for st, _, _ in made.values():
        st.plan.close()


@pytest.mark.parametrize("which", range(11))
@pytest.mark.parametrize("name", GEOMETRIES)
def test_bins_other_geometries(ctx, streams, name, which):
    st, x, start = streams(name)
    bin = bins_of(st.plan.longest_wave())[which]
    full = default_n_bins(st.Ns, st.Ls, bin)
    ctx.set_option("debug_flags", D.DBG_BINS_LANES)
    try:
        check(ctx, st, x, bin, full + 5, None, 0, what=name)
        check(ctx, st, x, bin, None, start, 0, what=name)
        check(ctx, st, x, bin, max(full * 2 // 5, 1), start, -64, what=name)
    finally:
        ctx.set_option("debug_flags", 0)


def test_bins_gates_on_other_geometries(ctx, streams):
    for name in GEOMETRIES:
        st, x, start = streams(name)
        check(ctx, st, x, 250, 8, start, -500, what=name)


# few long waveforms: there is no block form yet, so every batch stays a lane per waveform under every flag
def test_bins_long_waveforms_stay_on_lanes(ctx, O):
    Ns, Ls, m, taps, sigma = BATCHES["long-2"]
    x = np.random.default_rng(21).normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        start = torch.from_numpy(np.random.default_rng(22).integers(-1000, 51001, st.plan.total_waves)).to(ctx.device)
        for flags in (0, D.DBG_BINS_LANES, D.DBG_NO_LONG_PATHS, D.DBG_LONG_NOT_BLOCKS, D.DBG_BINS_ALL_FALLBACK):
            ctx.set_option("debug_flags", flags)
            check(ctx, st, x, 1000, None, None, 0, what=("long-2", flags))  # (asserts BINS_FORM_LANES and nothing listed)
            check(ctx, st, x, 4999, 12, start, 0, what=("long-2", flags))
    finally:
        ctx.set_option("debug_flags", 0)
        st.plan.close()


# --------------------------------------------------------------------------- 3. general filters: the serial kernel
@pytest.mark.parametrize("name", ["fir4", "fir5"])
def test_bins_filters(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        L = st.plan.longest_wave()
        start = torch.from_numpy(np.random.default_rng(13).integers(-300, L + 301, st.plan.total_waves)).to(ctx.device)
        for bin in (64, L):
            full = default_n_bins(Ns, Ls, bin)
            check(ctx, st, x, bin, full, None, 0, what=name)
            check(ctx, st, x, bin, full + 5, start, -7, what=name)
            check(ctx, st, x, bin, 1, start, 0, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. where the buffers lie
def test_bins_placements(ctx, O):
    Ns, Ls = SHAPE
    x = np.random.default_rng(7).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    bin, n_bins, offset = 250, 12, -100
    stride = n_bins * D.BIN_COLS + 3  # odd: the rows of every other waveform are 16-byte aligned, the others are not
    start_np = np.random.default_rng(8).integers(-300, L0 + 301, W)
    want = torch.from_numpy(wave_bins(x, Ns, Ls, bin, n_bins, start_np, offset)).to(ctx.device)
    SENT = 0x5A5A5A5A5A5A5A5A
    try:
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            sw = window(W, torch.int64, 8 - P["off"], device=ctx.device)
            sw.t.copy_(torch.from_numpy(start_np))
            for obyte in (8, 0):
                for sideband in (False, True):
                    yw = window((W - 1) * stride + n_bins * D.BIN_COLS, torch.int64, obyte, fill=SENT, device=ctx.device)
                    assert yw.t.data_ptr() % 16 == obyte
                    args = (sw.t.data_ptr(), 1, offset, bin, n_bins, yw.t.data_ptr(), stride)
                    if sideband:
                        launch = lambda: ctx._check(ctx.lib.drx_wave_bins_with_wave_words(  # noqa: E731
                            plan._h, ww.t.data_ptr(), total, ow.t.data_ptr(), st.table.data_ptr(), *args))
                    else:
                        launch = lambda: ctx._check(ctx.lib.drx_wave_bins(plan._h, ww.t.data_ptr(), total, ow.t.data_ptr(), *args))  # noqa: E731
                    run(ctx, plan, launch)
                    assert plan.last_decode_path() == D.PATH_BINS and plan.last_bins_form() == D.BINS_FORM_LANES
                    padded = torch.full((W * stride,), SENT, dtype=torch.int64, device=ctx.device)
                    padded[:yw.t.numel()] = yw.t
                    padded = padded.view(W, stride)
                    same = torch.equal(padded[:, :n_bins * D.BIN_COLS].reshape(W, n_bins, D.BIN_COLS), want)
                    gaps = bool((padded[:, n_bins * D.BIN_COLS:] == SENT).all())
                    intact = yw.intact() and ow.intact() and ww.intact() and sw.intact()
                    assert same and gaps and intact, (pname, obyte, sideband, "rows differ" * (not same), "gap written" * (not gaps),
                                                      "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
    finally:
        plan.close()


# --------------------------------------------------------------------------- 5. verdicts and refusals
def test_bins_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    bin, n_bins = 10, 2  # the bins end at sample 20: every waveform is parsed to its end all the same
    want = torch.from_numpy(wave_bins(x, Ns, Ls, bin, n_bins)).to(ctx.device)

    def batch_of(w):
        return dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)

    def clean():
        assert torch.equal(plan.wave_bins(good, bin, n_bins), want) and plan.last_decode_path() == D.PATH_BINS

    try:
        clean()
        header = st.words.copy()
        header[int(st.offs[1]) + 1] += 1  # the first waveform header of chunk 1
        cases = {"header": batch_of(header), "payload": batch_of(flipped_payload(O, st.words, st.offs, Ns, Ls, 3)),
                 "short": dr.EncodedBatch(good.words, good.chunk_word_off, good.total_words - 1)}
        for cname, enc in cases.items():
            for sideband in (False, True) if cname == "payload" else (False,):
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.wave_bins(enc, bin, n_bins, wave_words=st.table if sideband else None)
                assert e.value.status == 4, (cname, sideband)
                clean()  # the plan stays usable, and its next call starts clean
        # DRX_ERR_ARG: nothing launched -- the status word keeps the verdict of the call before
        out = torch.full((plan.total_waves, n_bins, D.BIN_COLS), 0x5A5A, dtype=torch.int64, device=ctx.device)
        start = torch.zeros(plan.total_waves, dtype=torch.int64, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.wave_bins_async(cases["header"].words, good.chunk_word_off, bin, n_bins, out=out, in_words=good.total_words)
        lib, h, w, n, off, o, s = ctx.lib, plan._h, good.words.data_ptr(), good.total_words, good.chunk_word_off.data_ptr(), out.data_ptr(), start.data_ptr()
        row = n_bins * D.BIN_COLS
        assert lib.drx_wave_bins(h, None, n, off, None, 1, 0, bin, n_bins, o, row) == 1
        assert lib.drx_wave_bins(h, w, n, None, None, 1, 0, bin, n_bins, o, row) == 1
        assert lib.drx_wave_bins(h, w, n, off, None, 1, 0, bin, n_bins, None, row) == 1
        assert lib.drx_wave_bins(h, w, n, off, None, 1, 0, 0, n_bins, o, row) == 1          # bin == 0
        assert lib.drx_wave_bins(h, w, n, off, s, 0, 0, bin, n_bins, o, row) == 1           # start_stride == 0 with d_start
        assert lib.drx_wave_bins(h, w, n, off, None, 1, 0, bin, n_bins, o, row - 1) == 1    # rows would overlap
        assert lib.drx_wave_bins_with_wave_words(h, w, n, off, None, None, 1, 0, bin, n_bins, o, row) == 1
        assert lib.drx_wave_bins_with_wave_words(h, w, n, off, lib.drx_plan_wave_words(h), None, 1, 0, bin, n_bins, o, row) == 1
        assert lib.drx_wave_bins(h, w, n, off, None, 0, 0, bin, 0, o, 0) == 0               # n_bins == 0: DRX_OK, nothing launched
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.finish()
        assert e.value.status == 4
        clean()
        assert plan.wave_bins(good, bin, 0).shape == (plan.total_waves, 0, D.BIN_COLS)
    finally:
        plan.close()


# --------------------------------------------------------------------------- 6. RiceParameter
@pytest.mark.parametrize("m", [1, 2, 64, 32768])
def test_bins_rice_parameters(ctx, O, m):
    """The lane kernel's code-length arithmetic at the ends of k and beside them (every other cell of this module is m = 8):
    the shape and the data of test_gpu_wave_stats.py::test_stats_rice_parameters."""
    Ns, Ls = [65 * 300] * 2, [300] * 2
    for sigma in (10, 400):
        x = np.random.default_rng(m + sigma).normal(0, sigma, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, m)
        try:
            start = torch.from_numpy(np.random.default_rng(m).integers(-50, 351, st.plan.total_waves)).to(ctx.device)
            for bin in (16, 17, 250):
                full = default_n_bins(Ns, Ls, bin)
                for origin in (None, start):
                    check(ctx, st, x, bin, None, origin, 0, what=(m, sigma))
                    check(ctx, st, x, bin, max(full * 2 // 5, 1), origin, 0, what=(m, sigma))  # (stops mid-waveform)
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 7. the serial kernel under every kind of filter
@pytest.mark.parametrize("fname", list(FILTERS))
def test_bins_serial_filters(ctx, O, fname):
    """k_wave_bins_serial under a lead of -1, a lead that divides (held to the oracle's DECODE of its stream), three, five and
    64 taps."""
    taps = FILTERS[fname]
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(len(taps)).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        y = samples_of(O, st, x, 8, taps)
        start = torch.from_numpy(np.random.default_rng(14).integers(-50, 351, st.plan.total_waves)).to(ctx.device)
        for bin in (1, 64, 300):
            full = default_n_bins(Ns, Ls, bin)
            check(ctx, st, y, bin, None, None, 0, what=fname)
            check(ctx, st, y, bin, full + 5, start, -7, what=fname)
            check(ctx, st, y, bin, max(full * 2 // 5, 1), start, 0, what=fname)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 8. waveforms of one or two groups
SHORT_LS = (1, 15, 16, 17, 31, 32, 33)


def test_bins_short_waveforms(ctx, O):
    """Waveforms that are a first group alone, a first and a last, and one unmasked group between them: a chunk per length, 70
    waveforms each (a wavefront and a partial one) with a shorter last one wherever a length has one; then the batch of one
    sample."""
    Ls = list(SHORT_LS)
    Ns = [69 * L + max(1, L // 2) for L in Ls]
    x = np.random.default_rng(15).normal(0, 400, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        assert st.plan.total_waves == 70 * len(Ls) and int(st.length[-1]) == 16
        rng = np.random.default_rng(16)
        per_wave_L = np.array(Ls, np.int64)[st.chunk]
        start = torch.from_numpy(rng.integers(-20, per_wave_L + 21)).to(ctx.device)
        for bin in (1, 16, 17):
            full = default_n_bins(Ns, Ls, bin)
            check(ctx, st, x, bin, None, None, 0, what="short")
            check(ctx, st, x, bin, full + 2, start, 0, what="short")
            check(ctx, st, x, bin, max(full * 2 // 5, 1), start, -3, what="short")
    finally:
        st.plan.close()
    x = np.array([-123], np.int16)
    st = Stream(ctx, O, x, [1], [0], 8)
    try:
        for bin in (1, 16, 17):
            check(ctx, st, x, bin, None, None, 0, what="one sample")
            check(ctx, st, x, bin, 3, torch.tensor([-1], dtype=torch.int64, device=ctx.device), 0, what="one sample")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 9. a waveform that becomes wide in its middle
PLATEAU = 48
PLATEAU_VALUES = (16383, 16384, -16384, -32768, 20000)  # the first stays narrow: 16 x 16383^2 < 2^32
PLATEAU_STARTS = (5, 16, 23, 160, 167, 650)  # in the masked first group; group-aligned; inside a group; reaching the masked last group
WIDE_L = 700


def plateau_rows():
    """int16 [30, 700]: quiet rows (sigma 10), each with one plateau of 48 samples -- every value at every start."""
    rng = np.random.default_rng(17)
    x = rng.normal(0, 10, (len(PLATEAU_VALUES) * len(PLATEAU_STARTS), WIDE_L)).astype(np.int16)
    for r in range(x.shape[0]):
        s = PLATEAU_STARTS[r % len(PLATEAU_STARTS)]
        x[r, s:s + PLATEAU] = PLATEAU_VALUES[r // len(PLATEAU_STARTS)]
    return x


def test_bins_and_stats_narrow_to_wide(ctx, O):
    """The sticky `narrow` flag of k_wave_bins and k_wave_stats: while it holds, a group's sixteen squares are summed in 32
    bits.  Every row here starts quiet and meets a plateau later; at +-16384 sixteen squares sum to exactly 2^32, which a
    32-bit chain returns as 0.  The 16383 rows are the control: they must stay on the 32-bit chain and be right."""
    x = plateau_rows()
    W, L = x.shape
    # the case proves something only if a wide row holds a whole 16-aligned group whose squares reach 2^32, and a narrow row none
    sq = (x.astype(np.int64) ** 2)[:, :L // 16 * 16].reshape(W, -1, 16).sum(axis=2)
    wide = np.repeat(np.array([abs(v) > 16383 for v in PLATEAU_VALUES]), len(PLATEAU_STARTS))
    assert ((sq >= 1 << 32).any(axis=1) == wide).all() and wide.sum() == 4 * len(PLATEAU_STARTS)
    assert (sq[np.repeat(np.array([abs(v) == 16384 for v in PLATEAU_VALUES]), len(PLATEAU_STARTS))] == 1 << 32).sum() >= 2 * 2 * len(PLATEAU_STARTS)
    Ns, Ls = [W * L], [L]
    st = Stream(ctx, O, x.reshape(-1), Ns, Ls, 8)
    try:
        start = torch.from_numpy(np.random.default_rng(18).integers(-40, L, W)).to(ctx.device)
        for bin in (16, 17, 64, 250):
            check(ctx, st, x.reshape(-1), bin, None, None, 0, what="plateaus")
            check(ctx, st, x.reshape(-1), bin, None, start, 0, what="plateaus")
        want = torch.from_numpy(wave_stats_heads(x.reshape(-1), Ns, Ls, [100])[0]).to(ctx.device)
        for sideband in (False, True):
            got = st.plan.wave_stats(st.enc, head=100, wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_STATS and st.plan.last_stats_form() == D.STATS_FORM_LANES, sideband
            if not torch.equal(got, want):
                g = int(torch.nonzero((got != want).any(dim=1)).flatten()[0])
                raise AssertionError(("wave_stats", sideband, f"row {g}", got[g].tolist(), want[g].tolist()))
    finally:
        st.plan.close()
