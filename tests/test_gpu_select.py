"""GPU: drx_decode_select -- selected waveforms of a batch, bit-exact against the samples the CPU oracle was given.

Except in the user-size case the streams are the oracle's (not the encoder's under test), and the expected rows are cut
from the oracle's input.  Every cell asserts DRX_PATH_SELECT."""
import numpy as np
import pytest

from conftest import golden_case_names
from deltarice_amd import _lib as D
from test_gpu_placement import FF, PLACEMENTS, SLACK, Batch, run, window
from test_gpu_routes import BATCHES, make_plan

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


def geometry(Ns, Ls):
    """-> (first sample, length, chunk) of every waveform, by a loop over the chunks."""
    start, length, chunk, at = [], [], [], 0
    for c, (N, L) in enumerate(zip(Ns, Ls)):
        L = L if L > 0 else N
        for i in range(0, N, L):
            start.append(at + i)
            length.append(min(L, N - i))
            chunk.append(c)
        at += N
    return np.array(start, np.int64), np.array(length, np.int64), np.array(chunk, np.int64)


def header_table(words, offs, Ns, Ls):
    """n_i of every waveform, by walking the header chains of the oracle's stream on the host (the side-band)."""
    out = []
    for c, (N, L) in enumerate(zip(Ns, Ls)):
        L = L if L > 0 else N
        at = int(offs[c]) + 1
        for _ in range(-(-N // L)):
            out.append(int(words[at]))
            at += int(words[at]) + 1
        assert at == int(offs[c + 1])
    return np.array(out, np.uint32)


def expected_rows(xd, start, length, sel, stride, fill=0):
    """[n_sel, stride] on the device: row i = the samples of waveform sel[i], `fill` behind them."""
    s = torch.from_numpy(start[sel]).to(xd.device)[:, None]
    n = torch.from_numpy(length[sel]).to(xd.device)[:, None]
    j = torch.arange(stride, device=xd.device)[None, :]
    rows = xd[(s + j).clamp_(max=xd.numel() - 1)]
    return torch.where(j < n, rows, torch.full_like(rows, fill))


class Stream:
    """An oracle-encoded batch on the device, its plan, geometry and side-band."""

    def __init__(self, ctx, O, x, Ns, Ls, m, taps=None):
        import deltarice_amd as dr
        ftaps = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()
        words, offs, at = [], [0], 0
        for N, L in zip(Ns, Ls):
            w = O.encode_chunk(x[at:at + N], ((m, L) if L else (m,)) + ftaps)
            words.append(w)
            offs.append(offs[-1] + w.size)
            at += N
        self.words = np.concatenate(words)
        self.offs = np.array(offs, np.int64)
        self.Ns, self.Ls = Ns, Ls
        self.xd = torch.from_numpy(x).to(ctx.device)
        self.enc = dr.EncodedBatch(torch.from_numpy(self.words.view(np.int32)).to(ctx.device),
                                   torch.from_numpy(self.offs).to(ctx.device), int(offs[-1]))
        self.plan = make_plan(ctx, Ns, Ls, m, taps)
        self.start, self.length, self.chunk = geometry(Ns, Ls)
        self.table = torch.from_numpy(header_table(self.words, self.offs, Ns, Ls).view(np.int32)).to(ctx.device)

    def check(self, sel, sideband=False, what=""):
        sel = np.asarray(sel, np.int64)
        y = self.plan.decode_select(self.enc, sel, wave_words=self.table if sideband else None)
        assert self.plan.last_decode_path() == D.PATH_SELECT, what
        assert y.shape == (sel.size, self.plan.longest_wave()), what
        assert np.array_equal(self.plan.wave_lengths(sel), self.length[sel]), what
        want = expected_rows(self.xd, self.start, self.length, sel, y.shape[1])
        assert torch.equal(y, want), (what, sideband, sel[:8].tolist())


def selections(st, rng):
    """name -> waveform indices: singles (first, last, the short last-of-chunk one), 64 random, all reversed, duplicates,
    all of one chunk."""
    W = st.start.size
    sels = {"first": [0], "last": [W - 1]}
    L = np.array([l if l > 0 else n for n, l in zip(st.Ns, st.Ls)])
    short = [i for i in range(W) if st.length[i] < L[st.chunk[i]]]
    if short:
        sels["short-last"] = [short[0]]
    sels["random64"] = rng.integers(0, W, 64)
    sels["reversed"] = np.arange(W)[::-1]
    d = rng.integers(0, W, 5)
    sels["duplicates"] = np.concatenate([d, d[::-1], d[:2], d[:2]])
    c = int(st.chunk[W // 2])
    sels["one-chunk"] = np.nonzero(st.chunk == c)[0]
    return sels


# --------------------------------------------------------------------------- 1. every batch of the route table
@pytest.mark.parametrize("name", list(BATCHES))
def test_select_every_batch(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        for sname, sel in selections(st, rng).items():
            for sideband in (False, True):
                st.check(sel, sideband, (name, sname))
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. the reference's own bytes
@pytest.mark.parametrize("name", golden_case_names())
def test_select_golden(ctx, O, golden, name):
    import deltarice_amd as dr
    g = golden[name]
    x = O.decode_chunk(g["words"], g["opts"])
    o = g["opts"]
    L = o[1] if len(o) > 1 and 0 < o[1] < 0x80000000 else 0
    start, length, _ = geometry([x.size], [L])
    W = start.size
    plan = ctx.plan_uniform(1, x.size, o)
    enc = dr.EncodedBatch(torch.from_numpy(g["words"].view(np.int32)).to(ctx.device),
                          torch.tensor([0, g["words"].size], dtype=torch.int64, device=ctx.device), int(g["words"].size))
    xd = torch.from_numpy(x).to(ctx.device)
    picks = np.arange(W) if W <= 64 else np.random.default_rng(W).choice(W, 64, replace=False)
    try:
        for w in picks:
            y = plan.decode_select(enc, [int(w)])
            assert plan.last_decode_path() == D.PATH_SELECT
            want = expected_rows(xd, start, length, np.array([w]), y.shape[1])
            assert torch.equal(y, want), (name, int(w))
    finally:
        plan.close()


# --------------------------------------------------------------------------- 3. parses that do not fall into step
def hard_streams(L):
    n = 3 * L + L // 3  # three waveforms and a short one
    i = np.arange(n, dtype=np.int64)
    yield "ramp", 8, (i & 0xFFFF).astype(np.uint16).view(np.int16)       # every delta 1 (mod 2^16): all codes the same length
    yield "zeros-k0", 1, np.zeros(n, np.int16)                             # one bit per sample
    yield "pm32767", 8, np.where(i & 1, -32767, 32767).astype(np.int16)    # the largest swing of the samples
    yield "pm16000", 8, np.where(i & 1, -16000, 16000).astype(np.int16)    # deltas of +-32000: every code an escape


@pytest.mark.parametrize("L", [7000, 50000])
def test_select_streams_that_do_not_resynchronise(ctx, O, L):
    for name, m, x in hard_streams(L):
        st = Stream(ctx, O, np.concatenate([x, x]), [x.size] * 2, [L] * 2, m)  # two chunks
        try:
            W = st.start.size
            st.check(np.arange(W), False, (name, L))
            st.check([W - 1, 0, 3], True, (name, L))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 4. where the buffers lie
@pytest.mark.parametrize("name", ["stream-quiet", "ragged", "short"])
def test_select_placements(ctx, name):
    b = Batch(ctx, name)
    plan = b.plan
    Ns, Ls = BATCHES[name][:2]
    start, length, _ = geometry(Ns, Ls)
    W = start.size
    rng = np.random.default_rng(W)
    sel = np.concatenate([[0, W - 1], rng.integers(0, W, 40), np.argsort(length)[:3]])
    stride = plan.longest_wave() + 3
    want = expected_rows(b.xd, start, length, sel, stride, fill=0x5A5A)
    try:
        for pname, P in PLACEMENTS.items():
            ww = window(b.total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:b.total].copy_(b.ref_w)
            ow = window(len(Ns) + 1, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(b.ref_off)
            yw = window(sel.size * stride, torch.int16, P["y"], fill=0x5A5A, device=ctx.device)
            out = yw.t.view(sel.size, stride)
            run(ctx, plan, lambda: plan.decode_select_async(ww.t, ow.t, sel, out=out, in_words=b.total))
            assert plan.last_decode_path() == D.PATH_SELECT
            same, intact = torch.equal(out, want), yw.intact() and ow.intact() and ww.intact()
            assert same and intact, (name, pname, "samples differ" * (not same), "guard written" * (not intact))
            assert bool((ww.t[b.total:] == FF).all()), (name, pname)
    finally:
        plan.close()


# --------------------------------------------------------------------------- 5. what is looked at, and what is reported
def test_select_leaves_untouched_chunks_alone_and_reports_touched_ones(ctx, O):
    import deltarice_amd as dr
    n_chunks, Wc, L = 6, 40, 7000
    x = np.random.default_rng(5).normal(0, 10, n_chunks * Wc * L).astype(np.int16)
    st = Stream(ctx, O, x, [Wc * L] * n_chunks, [L] * n_chunks, 8)
    plan = st.plan
    good = st.enc
    try:
        bad_c = 2
        others = np.nonzero(st.chunk != bad_c)[0]
        w = st.words.copy()
        w[st.offs[bad_c]:st.offs[bad_c + 1]] = 0xFFFFFFFF
        broken = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)
        for sideband in (False, True):
            tab = st.table if sideband else None
            y = plan.decode_select(broken, others, wave_words=tab)  # DRX_OK: the overwritten chunk is not looked at
            assert torch.equal(y, expected_rows(st.xd, st.start, st.length, others, L)), sideband
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.decode_select(broken, [bad_c * Wc + 7], wave_words=tab)
            assert e.value.status == 4, sideband
        # a selected waveform whose payload is replaced by zero bits: the stream runs out before its samples do
        g = 3 * Wc + 5
        at = int(st.offs[3]) + 1
        for _ in range(5):
            at += int(st.words[at]) + 1
        w = st.words.copy()
        w[at + 1:at + 1 + int(w[at])] = 0
        overrun = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.decode_select(overrun, [g])
        assert e.value.status == 4
        # ... and by one bits: every code the shortest there is, 7000 samples end 875 words into a payload of ~2000
        w = st.words.copy()
        w[at + 1:at + 1 + int(w[at])] = 0xFFFFFFFF
        early = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.decode_select(early, [g])
        assert e.value.status == 4
        y = plan.decode_select(early, [g - 1, g + 1])  # its neighbours are whole
        assert torch.equal(y, expected_rows(st.xd, st.start, st.length, np.array([g - 1, g + 1]), L))
        # a side-band table from another stream
        other = Stream(ctx, O, np.roll(x, 12345), st.Ns, st.Ls, 8)
        try:
            assert not torch.equal(other.table, st.table)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.decode_select(good, others[:50], wave_words=other.table)
            assert e.value.status == 4
        finally:
            other.plan.close()
        st.check(others[::-1], False, "the plan is still usable")
    finally:
        plan.close()


# --------------------------------------------------------------------------- 6. arguments, and the plan's other calls
def test_select_arguments_and_shared_tables(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [7000 * 20 + 100] * 3, [7000] * 3
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, enc = st.plan, st.enc
    W = plan.total_waves
    try:
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.decode_select(enc, [0, W])
        assert e.value.status == 1
        small = torch.full((2, 6999), 0x5A5A, dtype=torch.int16, device=ctx.device)
        with pytest.raises(dr.DeltaRiceError) as e:
            plan.decode_select(enc, [0, 1], out=small)
        assert e.value.status == 1
        # ... and through the C ABI itself: nothing is launched, nothing written
        idx = (np.array([0, 1], np.uint64)).ctypes.data_as(D.C.POINTER(D.C.c_uint64))
        out = torch.full((2, 7000), 0x5A5A, dtype=torch.int16, device=ctx.device)
        torch.cuda.synchronize()
        rc = ctx.lib.drx_decode_select(plan._h, enc.words.data_ptr(), enc.total_words, enc.chunk_word_off.data_ptr(), idx, 2,
                                       out.data_ptr(), 6999)
        assert rc == 1
        rc = ctx.lib.drx_decode_select(plan._h, enc.words.data_ptr(), enc.total_words, enc.chunk_word_off.data_ptr(), None, 2,
                                       out.data_ptr(), 7000)
        assert rc == 1
        assert ctx.lib.drx_decode_select(plan._h, None, 0, None, None, 0, None, 0) == 0  # n_sel == 0: DRX_OK
        plan.finish()
        assert bool((out == 0x5A5A).all())
        y = plan.decode_select(enc, [])
        assert y.shape == (0, 7000)
        # the short last waveform fits a row of its own length
        last = torch.full((1, 100), 0x5A5A, dtype=torch.int16, device=ctx.device)
        plan.decode_select(enc, [20], out=last)
        assert torch.equal(last.view(-1), st.xd[20 * 7000:20 * 7000 + 100])
        # a full decode after a select on the same plan, and a select after a full decode
        st.check([5, 40], False, "select")
        assert torch.equal(plan.decode(enc), st.xd)
        assert plan.last_decode_path() != D.PATH_SELECT
        st.check([41, 5, 62], False, "select after decode")
        st.check([1], True, "side-band select")
        assert torch.equal(plan.decode(enc), st.xd)
        with pytest.raises(dr.DeltaRiceError):
            plan.decode_select(enc, torch.tensor([0], device=ctx.device))  # a selection lives on the host
    finally:
        plan.close()


# --------------------------------------------------------------------------- 7. a user's size
def test_select_at_a_users_size(ctx):
    n_chunks, Wc, L = 100, 2000, 7000
    g = torch.Generator(device=ctx.device).manual_seed(77)
    x = (torch.randn(n_chunks * Wc * L, device=ctx.device, generator=g) * 10).to(torch.int16)
    plan = ctx.plan_uniform(n_chunks, Wc * L, (8, L))
    try:
        enc = plan.encode(x)
        table = plan.wave_words_device()
        sel = np.random.default_rng(77).choice(n_chunks * Wc, 4096, replace=False)
        rows = x.view(-1, L).index_select(0, torch.from_numpy(sel).to(ctx.device))
        for tab in (None, table):
            y = plan.decode_select(enc, sel, wave_words=tab)
            assert plan.last_decode_path() == D.PATH_SELECT
            assert torch.equal(y, rows), tab is not None
    finally:
        plan.close()
