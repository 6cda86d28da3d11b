"""GPU: drx_decode_window -- `width` samples of every waveform from a per-waveform start, parsed from the encoded stream.

The streams are the oracle's (oracle.encode_chunk), the expected rows numpy's over the oracle's input
(tests/decode_window_reference.py; for a filter whose lead is not +-1, over the oracle's decode of that stream), the
comparison torch.equal on every row.  Every cell asserts DRX_PATH_WINDOW alone and plan.finish() == 0, through the walk and
through the side-band."""
import numpy as np
import pytest

from decode_window_reference import windows
from deltarice_amd import _lib as D
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, geometry, header_table  # noqa: F401  (Stream builds its side-band with header_table)
from test_gpu_wave_stats import FILTERS, crafted_rows, samples_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def on_device(ctx, start):
    return torch.from_numpy(np.asarray(start, np.int64)).to(ctx.device) if isinstance(start, np.ndarray) else start


def check(ctx, st, y, cases, sidebands=(False, True), what=""):
    """Every (start, offset, width, pad) x {walk, side-band} on st against numpy over the samples y."""
    geom = (st.start, st.length, st.chunk)
    for start, offset, width, pad in cases:
        want = torch.from_numpy(windows(y, st.Ns, st.Ls, start, offset, width, pad, geom)).to(ctx.device)
        assert want.shape == (st.plan.total_waves, width)
        sd = on_device(ctx, start)
        for sideband in sidebands:
            cell = (what, "per-lane" if isinstance(start, np.ndarray) else start, offset, width, pad, sideband)
            got = st.plan.decode_window(st.enc, sd, width, offset=offset, pad=pad, wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_WINDOW and st.plan.finish() == 0, cell
            assert got.dtype == torch.int16 and got.shape == want.shape, cell
            if not torch.equal(got, want):
                bad = torch.nonzero((got != want).any(dim=1)).flatten()
                g = int(bad[0])
                j = int(torch.nonzero(got[g] != want[g]).flatten()[0])
                raise AssertionError((cell, f"{bad.numel()} rows differ; row {g} from column {j}", got[g, j:j + 8].tolist(),
                                      want[g, j:j + 8].tolist()))


def lane_starts(rng, st, lo=-50, hi=50):
    """a start per waveform from [lo, len + hi)"""
    return rng.integers(lo, st.length + hi)


# --------------------------------------------------------------------------- 1. every batch of the route table
@pytest.mark.parametrize("name", list(BATCHES))
def test_window_every_batch(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        check(ctx, st, samples_of(O, st, x, m, taps), [(None, 0, 100, 0), (lane_starts(rng, st), 0, 96, -1)], what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. group and round edges
@pytest.fixture(scope="module")
def edges(ctx, O):
    Ns, Ls = [130 * 200 + 37] * 3, [200] * 3  # 131 waveforms per chunk: lanes in two chunks, the last waveform of 37 samples
    x = np.random.default_rng(2).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    yield st, x
    st.plan.close()


@pytest.mark.parametrize("start", [-5, 0, 1, 15, 16, 17, 63, 64, 65, 199, 200, 250])
def test_window_group_and_round_edges(ctx, edges, start):
    st, x = edges
    check(ctx, st, x, [(start, 0, width, 0x1234) for width in (1, 2, 15, 16, 17, 64, 65, 200, 201, 300)], what="edges")


def test_window_per_lane_starts_of_mixed_parity(ctx, edges):
    st, x = edges
    rng = np.random.default_rng(22)
    starts = lane_starts(rng, st, -20, 20)
    assert (starts & 1).any() and not (starts & 1).all()
    check(ctx, st, x, [(starts, 0, width, -2) for width in (1, 16, 33, 64, 201)] + [(starts, -7, 32, 7), (starts & ~1, 0, 31, 7),
                                                                                      (starts | 1, 0, 48, 7)], what="mixed parity")


# --------------------------------------------------------------------------- 3. refills and the early end
@pytest.fixture(scope="module")
def long_rows(ctx, O):
    Ns, Ls = [130 * 7000] * 2, [7000] * 2
    x = np.random.default_rng(3).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    yield st, x
    st.plan.close()


def test_window_refills_and_early_end(ctx, long_rows):
    st, x = long_rows
    rng = np.random.default_rng(33)
    check(ctx, st, x, [(None, 0, 500, 0), (3000, 0, 256, 0), (6700, 0, 300, -1), (6800, 0, 300, -1), (None, 0, 7000, 0),
                       (lane_starts(rng, st), 0, 256, 5), (lane_starts(rng, st), -64, 255, 5)], what="7000")
    ctx.set_option("profile", 1)
    try:
        for width in (500, 7000):
            st.plan.decode_window(st.enc, None, width)
            print(f"window [0, {width}) of 260 x 7000: walk / kernel / - / call ms = {st.plan.last_timings()}")
    finally:
        ctx.set_option("profile", 0)


# --------------------------------------------------------------------------- 4. nothing behind the window counts
def code_bits(x2d, k):
    """bits of every sample's code under the delta filter: int64 [W, L] (src/deltaRice.c:207-228)"""
    d = np.diff(x2d.astype(np.int32), axis=1, prepend=0).astype(np.int16).astype(np.int32)  # the int16 residual
    z = np.where(d >= 0, 2 * d, -2 * d - 1)
    q = z >> k
    return np.where(q < 8, q + 1 + k, 25).astype(np.int64)


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_window_ignores_what_lies_behind_it(ctx, O, long_rows, fill):
    import deltarice_amd as dr
    st, x = long_rows
    W, L, k = st.plan.total_waves, 7000, 3
    rng = np.random.default_rng(44)
    width = 200
    starts = rng.integers(-30, 3500 - width, W)  # every window ends in front of sample 3500
    ends = np.clip(starts + width, 0, L)
    bits = np.cumsum(code_bits(x.reshape(W, L), k), axis=1)
    end_bit = np.where(ends > 0, bits[np.arange(W), np.maximum(ends, 1) - 1], 0)  # behind the window's last code
    n = header_table(st.words, st.offs, st.Ns, st.Ls).astype(np.int64)
    assert np.array_equal((bits[:, -1] + 31) // 32, n)  # (the host's code lengths are the stream's)
    words, at, damaged = st.words.copy(), 0, 0
    for g in range(W):
        at = int(st.offs[st.chunk[g]]) + 1 if g == 0 or st.chunk[g] != st.chunk[g - 1] else at
        lo, hi = at + 1 + int((end_bit[g] + 31) // 32), at + 1 + int(n[g])  # the payload words wholly behind that code
        words[lo:hi] = {"zeros": 0, "ones": 0xFFFFFFFF}.get(fill, rng.integers(0, 1 << 32, hi - lo, dtype=np.uint64).astype(np.uint32))
        damaged += hi - lo
        at = hi
    assert damaged > st.words.size // 3 and np.array_equal(header_table(words, st.offs, st.Ns, st.Ls), n.astype(np.uint32))
    bad = dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), st.enc.chunk_word_off, st.enc.total_words)
    want = torch.from_numpy(windows(x, st.Ns, st.Ls, starts, 0, width, -3)).to(ctx.device)
    sd = on_device(ctx, starts)
    for sideband in (False, True):
        got = st.plan.decode_window(bad, sd, width, pad=-3, wave_words=st.table if sideband else None)
        assert st.plan.last_decode_path() == D.PATH_WINDOW and st.plan.finish() == 0, (fill, sideband)
        assert torch.equal(got, want), (fill, sideband)
    with pytest.raises(dr.DeltaRiceError) as e:  # the control: a call that parses every payload to its end
        st.plan.wave_stats(bad)
    assert e.value.status == 4, fill


# --------------------------------------------------------------------------- 5. RiceParameter
@pytest.mark.parametrize("m", [1, 8, 64, 32768])
def test_window_rice_parameters(ctx, O, m):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    for sigma in (10, 400):
        rng = np.random.default_rng(m + sigma)
        x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, m)
        try:
            check(ctx, st, x, [(None, 0, 100, 0), (lane_starts(rng, st), 0, 96, -1), (None, 0, 300, 0)], what=(m, sigma))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 6. crafted rows
def test_window_crafted_rows(ctx, O):
    # all -32768, the ramp through the int16 wrap (at sample 2768), an escape every sample: the first 7000 samples of the
    # statistics tests' rows (crafted_rows() places a sample at index 69 990, so it is made at its own length and cut)
    x = np.ascontiguousarray(crafted_rows(W=70, L=70000)[:, :7000])
    W, L = x.shape
    assert (x[0] == -32768).all() and x[3, 2767] == 32767 and x[3, 2768] == -32768 and x[2, 1] == 16000
    st = Stream(ctx, O, x.reshape(-1), [W * L], [L], 8)
    try:
        check(ctx, st, x.reshape(-1), [(-40, 0, 300, 77), (L - 100, 0, 257, 77), (2700, 0, 128, 0), (None, 0, L, 0)], what="crafted")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. filters through the serial kernel
@pytest.mark.parametrize("fname", list(FILTERS))
def test_window_filters(ctx, O, fname):
    taps = FILTERS[fname]
    Ns, Ls = [65 * 300] * 2, [300] * 2
    rng = np.random.default_rng(len(taps))
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        check(ctx, st, samples_of(O, st, x, 8, taps), [(lane_starts(rng, st), 0, 96, -1), (lane_starts(rng, st), -3, 301, 9),
                                                       (None, 0, 100, 0)], what=fname)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 8. ragged plans, the smallest batch
def test_window_ragged_lengths_and_one_sample(ctx, O):
    Ns, Ls = [64 * 70 + 5, 512 * 3, 7000 * 2 + 100, 999], [64, 512, 7000, 0]
    rng = np.random.default_rng(6)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        check(ctx, st, x, [(None, 0, 100, 0), (lane_starts(rng, st), 0, 96, -1), (-3, 0, 70, 4)], what="ragged lengths")
    finally:
        st.plan.close()
    x = np.array([-123], np.int16)
    st = Stream(ctx, O, x, [1], [0], 8)
    try:
        check(ctx, st, x, [(None, 0, 1, 0), (-1, 0, 3, 8), (1, 0, 2, 8), (np.array([0]), 0, 16, 8)], what="one sample")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 9. where the buffers lie
def test_window_placements(ctx, O):
    Ns, Ls = [130 * 200 + 37] * 3, [200] * 3
    rng = np.random.default_rng(9)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    x.reshape(-1)[rng.integers(0, x.size, 500)] = 3000  # (pulses: the argmax column is not flat)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    width, offset, pad = 50, -9, -2
    try:
        stats = plan.wave_stats(st.enc)
        col = stats[:, D.STAT_ARGMAX]  # a column of a real statistics result: stride 8
        assert col.stride(0) == D.STAT_COLS and not col.is_contiguous()
        starts = col.cpu().numpy()
        assert (starts & 1).any() and not (starts & 1).all()
        odd8 = window(W, torch.int64, 8, device=ctx.device)  # an address that is 8 mod 16
        odd8.t.copy_(col)
        assert odd8.t.data_ptr() % 16 == 8
        givens = {"contiguous": col.contiguous(), "stats column": col, "8 mod 16": odd8.t}
        want = torch.from_numpy(windows(x, Ns, Ls, starts, offset, width, pad)).to(ctx.device)
        for pname, P in PLACEMENTS.items():
            ww = window(total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(st.enc.chunk_word_off)
            for obyte, stride, fill, given in ((0, width, 0x5A5A, "stats column"), (2, width + 1, -1, "contiguous"), (4, width + 7, 0x5A5A, "8 mod 16"),
                                               (14, width, -1, "stats column"), (2, width + 7, 0x5A5A, "stats column"),
                                               (14, width + 1, -1, "8 mod 16"), (0, width + 1, -1, "contiguous"), (4, width, 0x5A5A, "contiguous")):
                yw = window((W - 1) * stride + width, torch.int16, obyte, fill=fill, device=ctx.device)
                assert yw.t.data_ptr() % 16 == obyte
                for sideband in (False, True):
                    yw.t.fill_(fill)
                    run(ctx, plan, lambda: plan.decode_window_async(ww.t, ow.t, givens[given], width, offset=offset, pad=pad, out=yw.t,
                                                                    out_stride=stride, in_words=total,
                                                                    wave_words=st.table if sideband else None))
                    assert plan.last_decode_path() == D.PATH_WINDOW
                    rows = torch.as_strided(yw.t, (W, width), (stride, 1))
                    gaps = torch.as_strided(yw.t, (W - 1, stride - width), (stride, 1), yw.t.storage_offset() + width) if stride > width else None
                    same = torch.equal(rows, want)
                    intact = yw.intact() and ow.intact() and ww.intact() and odd8.intact() and (gaps is None or bool((gaps == fill).all()))
                    assert same and intact, (pname, obyte, stride, fill, given, sideband, "rows differ" * (not same), "guard or gap written" * (not intact))
            assert bool((ww.t[total:] == FF).all()), pname
        assert torch.equal(stats, plan.wave_stats(st.enc))  # (the column the windows read was not written)
    finally:
        plan.close()


# --------------------------------------------------------------------------- 10. rows beyond 2^32 bytes
def test_window_rows_beyond_4_gib(ctx, O):
    W, L, width, stride = 70000, 16, 8, 40000
    rng = np.random.default_rng(10)
    x = rng.normal(0, 10, W * L).astype(np.int16)
    st = Stream(ctx, O, x, [W * L], [L], 8)
    try:
        try:
            out = torch.empty((W - 1) * stride + width, dtype=torch.int16, device=ctx.device)  # 5.6 GB, of which the rows are touched
        except (RuntimeError, MemoryError) as e:
            pytest.skip(f"no room for the output: {e}")
        assert out.numel() * 2 > 1 << 32
        starts = rng.integers(-4, L, W)
        want = torch.from_numpy(windows(x, st.Ns, st.Ls, starts, 0, width, -9)).to(ctx.device)
        pick = torch.from_numpy(np.concatenate([[0, W - 1], rng.integers(0, W, 1000)])).to(ctx.device)
        at = (pick * stride)[:, None] + torch.arange(width, device=ctx.device)[None, :]
        for sideband in (False, True):
            out[at] = 0x5A5A
            run(ctx, st.plan, lambda: st.plan.decode_window_async(st.enc.words, st.enc.chunk_word_off, on_device(ctx, starts), width, pad=-9,
                                                                  out=out, out_stride=stride, in_words=st.enc.total_words,
                                                                  wave_words=st.table if sideband else None))
            assert st.plan.last_decode_path() == D.PATH_WINDOW
            assert torch.equal(out[at], want[pick]), sideband
        del out
    finally:
        st.plan.close()
        torch.cuda.empty_cache()


# --------------------------------------------------------------------------- 11. verdicts
def test_window_verdicts(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [65 * 300] * 2, [300] * 2
    rng = np.random.default_rng(11)
    x = rng.normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good, W = st.plan, st.enc, st.plan.total_waves
    starts = lane_starts(rng, st, -20, -120)  # every window holds samples and ends in front of its waveform's end
    starts[7] = 200  # (the lane of the truncated payload below: samples [200, 264) of 300)
    sd = on_device(ctx, starts)
    want = torch.from_numpy(windows(x, Ns, Ls, starts, 0, 64, -1)).to(ctx.device)

    def batch_of(w):
        return dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)

    def clean():
        got = plan.decode_window(good, sd, 64, pad=-1)
        assert torch.equal(got, want) and plan.last_decode_path() == D.PATH_WINDOW and plan.finish() == 0

    try:
        clean()
        header = st.words.copy()
        header[int(st.offs[1]) + 1] += 1  # the first waveform header of chunk 1: a broken chain
        # a payload truncated inside a window: waveform 7 keeps the words its first 230 codes take and loses the rest, and the
        # chain is mended around it (its header says so, the chunk's words close up).  That is still a header every walk
        # accepts (at least 1 + k bits per sample), so it is the lane that must notice that its window's codes run out
        g, at = 7, 1
        for _ in range(g):
            at += int(st.words[at]) + 1
        n = int(st.words[at])
        keep = (int(np.cumsum(code_bits(x[:300 * (g + 1)].reshape(-1, 300), 3), axis=1)[g, 229]) + 31) // 32
        need = (int(np.cumsum(code_bits(x[:300 * (g + 1)].reshape(-1, 300), 3), axis=1)[g, 263]) + 31) // 32
        assert (300 * 4 + 31) // 32 <= keep < need <= n
        cut = np.concatenate([st.words[:at], [np.uint32(keep)], st.words[at + 1:at + 1 + keep], st.words[at + 1 + n:]]).astype(np.uint32)
        offs = st.offs.copy()
        offs[1:] -= n - keep
        short = dr.EncodedBatch(torch.from_numpy(cut.view(np.int32)).to(ctx.device), torch.from_numpy(offs).to(ctx.device), int(offs[-1]))
        table = st.table.clone()
        table[g] = keep
        for cname, enc, kw in (("header", batch_of(header), {}), ("payload", short, {}), ("payload, side-band", short, dict(wave_words=table))):
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.decode_window(enc, sd, 64, pad=-1, **kw)
            assert e.value.status == 4, cname
            clean()  # the plan stays usable, and its next call starts clean
        # DRX_ERR_ARG, nothing launched: the status word keeps the verdict of the call before
        out = torch.full((W, 64), 0x5A5A, dtype=torch.int16, device=ctx.device)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        broken = batch_of(header)
        plan.decode_window_async(broken.words, good.chunk_word_off, sd, 64, out=out, in_words=good.total_words)
        lib, w, off, h, nw, o = ctx.lib, good.words.data_ptr(), good.chunk_word_off.data_ptr(), plan._h, good.total_words, out.data_ptr()
        assert lib.drx_decode_window(h, w, nw, off, sd.data_ptr(), 1, 0, 64, 0, None, 64) == 1
        assert lib.drx_decode_window(h, None, nw, off, sd.data_ptr(), 1, 0, 64, 0, o, 64) == 1
        assert lib.drx_decode_window(h, w, nw, None, sd.data_ptr(), 1, 0, 64, 0, o, 64) == 1
        assert lib.drx_decode_window(h, w, nw, off, sd.data_ptr(), 1, 0, 64, 0, o, 63) == 1
        assert lib.drx_decode_window(h, w, nw, off, sd.data_ptr(), 0, 0, 64, 0, o, 64) == 1
        assert lib.drx_decode_window_with_wave_words(h, w, nw, off, None, sd.data_ptr(), 1, 0, 64, 0, o, 64) == 1
        assert lib.drx_decode_window_with_wave_words(h, w, nw, off, lib.drx_plan_wave_words(h), sd.data_ptr(), 1, 0, 64, 0, o, 64) == 1
        assert lib.drx_decode_window(h, w, nw, off, sd.data_ptr(), 1, 0, 0, 0, o, 64) == 0  # width 0: DRX_OK, nothing launched
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.finish()
        assert e.value.status == 4
        torch.cuda.synchronize()
        clean()
        before = out.clone()
        assert lib.drx_decode_window(h, w, nw, off, sd.data_ptr(), 1, 0, 0, 0, o, 64) == 0 and plan.finish() == 0
        torch.cuda.synchronize()
        assert torch.equal(out, before) and plan.last_decode_path() == D.PATH_WINDOW
        # a decode behind a window call reports its own path
        assert torch.equal(plan.decode(good), st.xd) and plan.last_decode_path() not in (0, D.PATH_WINDOW)
        clean()
    finally:
        plan.close()
