"""GPU: drx_wave_stack, the persistent lane kernel and the serial kernel -- per position the number, the sum and the sum of squares
of the samples that the selected, aligned waveforms have there, parsed from the encoded stream.

The streams are the oracle's (oracle.encode_chunk), the expected rows numpy's over the oracle's input
(tests/wave_stack_reference.py), the comparison torch.equal on all three columns of every row.  Every call is made by the walk
and by the side-band and asserts DRX_PATH_STACK alone."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, geometry, header_table  # noqa: F401  (Stream builds its side-band with header_table)
from test_gpu_wave_bins import SHAPE, data_of
from test_gpu_wave_stats import FILTERS, flipped_payload, samples_of
from wave_bins_reference import wave_bins
from wave_stack_reference import default_width, wave_stack
from wave_stats_reference import wave_stats

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
L0 = 7000
assert SHAPE == ([43 * L0 + 3000] * 3, [L0] * 3)


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


def check(ctx, st, y, width, start=None, offset=0, select=None, what=""):
    """One (width, origin, selection) x {walk, side-band} on st against numpy over the samples y.  start: an int64 tensor on the
    device, any stride, or None; select: a bool or uint8 tensor on the device, or None.  width None: the call's default."""
    plan = st.plan
    ask, width = width, default_width(st.Ns, st.Ls, offset) if width is None else width
    want = wave_stack(y, st.Ns, st.Ls, width, None if start is None else start.cpu().numpy(), offset,
                      None if select is None else select.cpu().numpy())
    want = torch.from_numpy(want).to(ctx.device)
    for sideband in (False, True):
        got = plan.wave_stack(st.enc, ask, start=start, offset=offset, select=select, wave_words=st.table if sideband else None)
        cell = (what, width, offset, sideband)
        assert plan.last_decode_path() == D.PATH_STACK, cell
        assert got.dtype == torch.int64 and got.shape == want.shape == (width, D.STACK_COLS), cell
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).any(dim=1)).flatten()
            j = int(bad[0])
            raise AssertionError((cell, f"{bad.numel()} rows differ; row {j}", got[j].tolist(), want[j].tolist()))


def selections(W, rng, device):
    one = torch.zeros(W, dtype=torch.uint8, device=device)
    one[W * 2 // 3] = 1
    return {"none": torch.zeros(W, dtype=torch.bool, device=device), "one": one,
            "half": torch.from_numpy(rng.integers(0, 2, W).astype(np.uint8)).to(device).bool()}


# --------------------------------------------------------------------------- 1. widths x origins x selection on the delta filter
WIDTHS = (1, 15, 16, 17, 64, 1000, L0 - 1, L0, L0 + 1, None)


@pytest.mark.parametrize("kind", ["sigma-10", "sigma-400", "ramp", "constant", "alternating"])
def test_widths_origins_and_selections(ctx, O, kind):
    Ns, Ls = SHAPE
    x = data_of(kind, sum(Ns))
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, W = st.plan, st.plan.total_waves
    try:
        rng = np.random.default_rng(11)
        stats = plan.wave_stats(st.enc)
        ends = torch.tensor([I64_MIN, I64_MAX] * (W // 2), dtype=torch.int64, device=ctx.device)
        origins = {"none": (None, (0,)), "random": (torch.from_numpy(rng.integers(-300, L0 + 301, W)).to(ctx.device), (0,)),
                   "argmax": (stats[:, D.STAT_ARGMAX], (-64,)),  # the column as it is: a stride of 8
                   "int64 ends": (ends, (-1, 1))}
        for a in (-5, 0, L0 - 1, L0):  # equal origins through d_start
            origins[f"all {a}"] = (torch.full((W,), a, dtype=torch.int64, device=ctx.device), (0,))
        assert origins["argmax"][0].stride(0) == D.STAT_COLS
        sels = selections(W, rng, ctx.device)
        # a wavefront whose lanes are all unselected between two that have some: waveforms 64 .. 127
        gap = torch.ones(W, dtype=torch.uint8, device=ctx.device)
        gap[64:128] = 0
        for oname, (start, offsets) in origins.items():
            for offset in offsets:
                for width in WIDTHS:
                    check(ctx, st, x, width, start, offset, None, what=(kind, oname))
                for sname, select in sels.items():
                    for width in (17, 1000, None):
                        check(ctx, st, x, width, start, offset, select, what=(kind, oname, sname))
                check(ctx, st, x, None, start, offset, gap, what=(kind, oname, "gap"))
    finally:
        plan.close()


# --------------------------------------------------------------------------- 2. other geometries
@pytest.mark.parametrize("name", ["short", "ragged", "whole-chunk"])
def test_other_geometries(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        W, longest = st.plan.total_waves, st.plan.longest_wave()
        rng = np.random.default_rng(12)
        start = torch.from_numpy(rng.integers(-300, longest + 301, W)).to(ctx.device)
        half = torch.from_numpy(rng.integers(0, 2, W).astype(np.uint8)).to(ctx.device)
        check(ctx, st, x, None, None, 0, None, what=name)  # (whole-chunk: 261 001 positions, several tiles)
        check(ctx, st, x, None, start, 0, None, what=name)
        check(ctx, st, x, 300, start, -64, None, what=name)
        check(ctx, st, x, longest + 5, None, 0, half, what=name)
        check(ctx, st, x, 300, start, -64, half, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 3. general filters: the serial kernel
@pytest.mark.parametrize("fname", list(FILTERS))
def test_serial_filters(ctx, O, fname):
    taps = FILTERS[fname]
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(len(taps)).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        y = samples_of(O, st, x, 8, taps)
        W = st.plan.total_waves
        rng = np.random.default_rng(14)
        start = torch.from_numpy(rng.integers(-50, 351, W)).to(ctx.device)
        half = torch.from_numpy(rng.integers(0, 2, W).astype(np.uint8)).to(ctx.device)
        for width in (305, 17):
            for select in (None, half):
                check(ctx, st, y, width, None, 0, select, what=fname)
                check(ctx, st, y, width, start, -7, select, what=fname)
        check(ctx, st, y, None, None, 0, None, what=fname)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. the int32 partial sum's bound
@pytest.mark.parametrize("value", [-32768, 32767])
def test_seventy_thousand_extreme_waveforms(ctx, O, value):
    """70 000 waveforms of 8 samples, all at one end of int16: 65 535 x 32 768 is the most an int32 partial sum holds, so every
    row here is beyond it -- (70 000, 70 000 v, 70 000 v^2) exactly.  By default the batch spreads over 274 workgroups of one
    round each and no partial sum comes near the bound; under the context option "stack_workgroups" = 1 ONE workgroup takes
    all 274 rounds of 256 waveforms, and its sum is right only if it was flushed on the way (after 255 rounds: 65 280
    waveforms).  Width 8 is the narrow tile's kernel, width 600 the wide one's (the rows behind the eighth are nobody's)."""
    W, L = 70000, 8
    x = np.full(W * L, value, np.int16)
    st = Stream(ctx, O, x, [W * L], [L], 8)
    try:
        assert abs(W * value) > 1 << 31 and -(-W // 256) > 255
        for workgroups in (0, 1, 2):
            ctx.set_option("stack_workgroups", workgroups)
            for width in (L, 600):
                want = torch.zeros((width, D.STACK_COLS), dtype=torch.int64, device=ctx.device)
                want[:L] = torch.tensor([W, W * value, W * value * value], dtype=torch.int64, device=ctx.device)
                for sideband in (False, True):
                    got = st.plan.wave_stack(st.enc, width, wave_words=st.table if sideband else None)
                    assert st.plan.last_decode_path() == D.PATH_STACK
                    assert torch.equal(got, want), (workgroups, width, sideband, got[:L].tolist())
    finally:
        ctx.set_option("stack_workgroups", 0)
        st.plan.close()


def test_the_workgroup_cap_changes_no_row(ctx, O):
    """Selection, per-waveform origins and several tiles under one and three workgroups per tile; what the option refuses."""
    import deltarice_amd as dr
    Ns, Ls = SHAPE
    x = data_of("sigma-400", sum(Ns))
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        W = st.plan.total_waves
        rng = np.random.default_rng(19)
        start = torch.from_numpy(rng.integers(-300, L0 + 301, W)).to(ctx.device)
        half = torch.from_numpy(rng.integers(0, 2, W).astype(np.uint8)).to(ctx.device)
        for workgroups in (1, 3):
            ctx.set_option("stack_workgroups", workgroups)
            check(ctx, st, x, None, None, 0, None, what=workgroups)
            check(ctx, st, x, 300, start, -64, half, what=workgroups)
            check(ctx, st, x, 2 * 7168 + 5, start, -8000, None, what=workgroups)  # three tiles of positions
        for bad in (-1, 1 << 32):
            with pytest.raises(dr.DeltaRiceError) as e:
                ctx.set_option("stack_workgroups", bad)
            assert e.value.status == 1
    finally:
        ctx.set_option("stack_workgroups", 0)
        st.plan.close()


# --------------------------------------------------------------------------- 5. where the buffers lie
def test_placements(ctx, O):
    Ns, Ls = SHAPE
    x = np.random.default_rng(7).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    rng = np.random.default_rng(8)
    start_np, select_np = rng.integers(-300, L0 + 301, W), rng.integers(0, 2, W).astype(np.uint8)
    SENT = 0x5A5A5A5A5A5A5A5A
    cells = {(700, -100): None, (17, 0): None}
    for width, offset in cells:
        cells[(width, offset)] = torch.from_numpy(wave_stack(x, Ns, Ls, width, start_np, offset, select_np)).to(ctx.device)
    try:
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            sw = window(2 * W, torch.int64, 8 - P["off"], fill=I64_MAX, device=ctx.device)  # a strided start: every other element
            sw.t[::2].copy_(torch.from_numpy(start_np))
            bw = window(W, torch.uint8, P["x"] + 1, guard=0x5A, device=ctx.device)  # the selection at an odd address
            bw.t.copy_(torch.from_numpy(select_np))
            for (width, offset), want in cells.items():
                for obyte, stride in ((8, 3), (8, 5), (0, 5), (0, 3)):
                    for sideband in (False, True):
                        yw = window((width - 1) * stride + D.STACK_COLS, torch.int64, obyte, fill=SENT, device=ctx.device)  # rows of garbage
                        assert yw.t.data_ptr() % 16 == obyte
                        args = (sw.t.data_ptr(), 2, offset, width, bw.t.data_ptr(), yw.t.data_ptr(), stride)
                        if sideband:
                            launch = lambda: ctx._check(ctx.lib.drx_wave_stack_with_wave_words(  # noqa: E731
                                plan._h, ww.t.data_ptr(), total, ow.t.data_ptr(), st.table.data_ptr(), *args))
                        else:
                            launch = lambda: ctx._check(ctx.lib.drx_wave_stack(plan._h, ww.t.data_ptr(), total, ow.t.data_ptr(), *args))  # noqa: E731
                        run(ctx, plan, launch)
                        assert plan.last_decode_path() == D.PATH_STACK
                        padded = torch.full((width * stride,), SENT, dtype=torch.int64, device=ctx.device)
                        padded[:yw.t.numel()] = yw.t
                        padded = padded.view(width, stride)
                        same = torch.equal(padded[:, :D.STACK_COLS], want)
                        gaps = bool((padded[:, D.STACK_COLS:] == SENT).all())
                        intact = yw.intact() and ow.intact() and ww.intact() and sw.intact() and bw.intact()
                        assert same and gaps and intact, (pname, width, obyte, stride, sideband, "rows differ" * (not same),
                                                          "gap written" * (not gaps), "guard written" * (not intact))
            assert bool((ww.t[total:] == FF).all()) and bool((sw.t[1::2] == I64_MAX).all()), pname
    finally:
        plan.close()


# --------------------------------------------------------------------------- 6. verdicts and refusals
def test_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good, W = st.plan, st.enc, st.plan.total_waves
    want = torch.from_numpy(wave_stack(x, Ns, Ls, 300)).to(ctx.device)

    def batch_of(w):
        return dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)

    def clean():
        assert torch.equal(plan.wave_stack(good), want) and plan.last_decode_path() == D.PATH_STACK

    try:
        clean()
        header = st.words.copy()
        header[int(st.offs[1]) + 1] += 1  # the first waveform header of chunk 1
        flipped = flipped_payload(O, st.words, st.offs, Ns, Ls, 3)  # one waveform's codes no longer end in its last word
        # which waveform, and that the damage lies in a word behind the codes of its first 100 samples
        word = int(np.nonzero(flipped != st.words)[0][0])
        n_i = st.table.cpu().numpy().view(np.uint32).astype(np.int64)
        hdr = np.cumsum(n_i + 1) - (n_i + 1) + 1 + st.chunk  # every waveform's header word: a chunk header in front of each chunk
        g = int(np.searchsorted(hdr, word, side="right")) - 1
        first = int(hdr[g]) + 1
        assert int(st.words[hdr[g]]) == n_i[g] and first <= word < first + n_i[g], (g, word)
        assert (word - first) * 32 >= O.rice_unpack(st.words[first:first + n_i[g]], 100, 3)[1], (g, word)
        cases = {"header": batch_of(header), "payload": batch_of(flipped),
                 "short": dr.EncodedBatch(good.words, good.chunk_word_off, good.total_words - 1)}
        for cname, enc in cases.items():
            for sideband in (False, True) if cname == "payload" else (False,):
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.wave_stack(enc, wave_words=st.table if sideband else None)  # the window reaches every waveform's end
                assert e.value.status == 4, (cname, sideband)
                clean()  # the plan stays usable, and its next call starts clean
        # the same damage behind the window's end, or in a waveform that is not selected: DRX_OK and the exact rows
        others = torch.ones(W, dtype=torch.bool, device=ctx.device)
        others[g] = False
        for sideband in (False, True):
            ww = st.table if sideband else None
            assert torch.equal(plan.wave_stack(cases["payload"], 100, wave_words=ww), want[:100]), sideband
            got = plan.wave_stack(cases["payload"], select=others, wave_words=ww)
            assert torch.equal(got, torch.from_numpy(wave_stack(x, Ns, Ls, 300, select=others.cpu().numpy())).to(ctx.device)), sideband
        # a payload that runs out INSIDE a window which ends before the waveform does: the header of waveform v + 1 moved 15
        # words to the front, so that v keeps 15 words less and v + 1 has 15 more -- the chain still ends with its chunk and
        # both counts lie inside the bounds of 300 samples (38 .. 235 words), so only the lane of v can tell
        v = 70  # (the sixth waveform of chunk 1; its neighbour lies in the same chunk)
        assert st.chunk[v] == st.chunk[v + 1] and v not in (g, g - 1)
        cut = st.words.copy()
        cut[hdr[v]], cut[hdr[v + 1] - 15] = n_i[v] - 15, n_i[v + 1] + 15
        table = st.table.clone()
        table[v], table[v + 1] = int(n_i[v]) - 15, int(n_i[v + 1]) + 15
        kept = 32 * (int(n_i[v]) - 15)
        payload = st.words[hdr[v] + 1:hdr[v] + 1 + n_i[v]]
        assert n_i[v] - 15 >= 38 and O.rice_unpack(payload, 100, 3)[1] <= kept - 64 and O.rice_unpack(payload, 280, 3)[1] > kept
        without = torch.ones(W, dtype=torch.bool, device=ctx.device)
        without[v + 1] = False  # (its payload now begins with 15 words of its neighbour's)
        for sideband in (False, True):
            ww = table if sideband else None
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.wave_stack(batch_of(cut), 280, select=without, wave_words=ww)  # 280 < 300: not the end-of-payload check
            assert e.value.status == 4, sideband
            clean()
            got = plan.wave_stack(batch_of(cut), 100, select=without, wave_words=ww)  # the window ends in front of the cut
            assert torch.equal(got, torch.from_numpy(wave_stack(x, Ns, Ls, 100, select=without.cpu().numpy())).to(ctx.device)), sideband
            only = torch.zeros(W, dtype=torch.bool, device=ctx.device)
            only[:v] = True  # neither of the two is selected: nothing of them is parsed
            got = plan.wave_stack(batch_of(cut), select=only, wave_words=ww)
            assert torch.equal(got, torch.from_numpy(wave_stack(x, Ns, Ls, 300, select=only.cpu().numpy())).to(ctx.device)), sideband
        # a side-band that does not belong to the stream
        other = Stream(ctx, O, np.roll(x, 4321), Ns, Ls, 8)
        try:
            assert not torch.equal(other.table, st.table)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.wave_stack(good, wave_words=other.table)
            assert e.value.status == 4
        finally:
            other.plan.close()
        clean()
        # DRX_ERR_ARG: nothing launched -- the status word keeps the verdict of the call before
        out = torch.full((300, D.STACK_COLS), 0x5A5A, dtype=torch.int64, device=ctx.device)
        start = torch.zeros(W, dtype=torch.int64, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.wave_stack_async(cases["header"].words, good.chunk_word_off, 300, out=out, in_words=good.total_words)
        lib, h, w, n, off, o, s = ctx.lib, plan._h, good.words.data_ptr(), good.total_words, good.chunk_word_off.data_ptr(), out.data_ptr(), start.data_ptr()
        assert lib.drx_wave_stack(h, None, n, off, None, 1, 0, 300, None, o, 3) == 1
        assert lib.drx_wave_stack(h, w, n, None, None, 1, 0, 300, None, o, 3) == 1
        assert lib.drx_wave_stack(h, w, n, off, None, 1, 0, 300, None, None, 3) == 1
        assert lib.drx_wave_stack(h, w, n, off, s, 0, 0, 300, None, o, 3) == 1            # start_stride == 0 with d_start
        assert lib.drx_wave_stack(h, w, n, off, None, 1, 0, 300, None, o, 2) == 1         # rows would overlap
        assert lib.drx_wave_stack_with_wave_words(h, w, n, off, None, None, 1, 0, 300, None, o, 3) == 1
        assert lib.drx_wave_stack_with_wave_words(h, w, n, off, lib.drx_plan_wave_words(h), None, 1, 0, 300, None, o, 3) == 1
        assert lib.drx_wave_stack(h, w, n, off, None, 0, 0, 0, None, o, 3) == 0           # width == 0: DRX_OK, nothing launched
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.finish()
        assert e.value.status == 4
        clean()
        assert plan.wave_stack(good, 0).shape == (0, D.STACK_COLS)
    finally:
        plan.close()


# --------------------------------------------------------------------------- 7. among the plan's other calls
def test_in_sequence_on_one_plan(ctx, O):
    Ns, Ls = SHAPE
    x = np.random.default_rng(9).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, W = st.plan, st.plan.total_waves
    try:
        start = torch.from_numpy(np.random.default_rng(10).integers(-300, L0 + 301, W)).to(ctx.device)
        wide = torch.from_numpy(wave_stack(x, Ns, Ls, L0)).to(ctx.device)
        narrow = torch.from_numpy(wave_stack(x, Ns, Ls, 100, start.cpu().numpy(), -10)).to(ctx.device)
        stats = torch.from_numpy(wave_stats(x, Ns, Ls, 100)).to(ctx.device)
        bins = torch.from_numpy(wave_bins(x, Ns, Ls, 250, 8, start.cpu().numpy(), -500)).to(ctx.device)

        def others():
            assert torch.equal(plan.wave_stats(st.enc, head=100), stats) and plan.last_decode_path() == D.PATH_STATS
            assert torch.equal(plan.wave_bins(st.enc, 250, 8, start=start, offset=-500), bins) and plan.last_decode_path() == D.PATH_BINS
            assert torch.equal(plan.decode(st.enc), st.xd) and plan.last_decode_path() != D.PATH_STACK

        others()
        for _ in range(2):  # twice in a row: no stale accumulator
            assert torch.equal(plan.wave_stack(st.enc), wide) and plan.last_decode_path() == D.PATH_STACK
        assert torch.equal(plan.wave_stack(st.enc, 100, start=start, offset=-10), narrow)  # narrow behind wide
        assert torch.equal(plan.wave_stack(st.enc), wide)                                  # ... and the reverse
        assert torch.equal(plan.wave_stack(st.enc, 100, start=start, offset=-10, wave_words=st.table), narrow)
        assert plan.last_decode_path() == D.PATH_STACK and plan.finish() == 0
        others()
        # results of two halves of the batch add
        half = torch.arange(W, device=ctx.device) < W // 2
        assert torch.equal(plan.wave_stack(st.enc, select=half) + plan.wave_stack(st.enc, select=~half), wide)
    finally:
        plan.close()
