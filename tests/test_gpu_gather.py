"""GPU: drx_gather_encoded -- selected waveforms copied into a new encoded batch, byte for byte against the CPU oracle's
encoding of the gathered samples.

Except in the user-size case the streams are the oracle's (not the encoder's under test); the expected bytes of every output
chunk are oracle.encode_chunk of the samples its entries name, under the chunk's WaveformLength and the source's RiceParameter
and taps.  Every cell asserts DRX_PATH_GATHER.  No tolerance anywhere: every comparison is exact."""
import numpy as np
import pytest

from conftest import golden_case_names
from deltarice_amd import _lib as D
from test_gather_abi import brute_force_gather
from test_gpu_placement import FF, PLACEMENTS, SLACK, run, window
from test_gpu_routes import BATCHES
from test_gpu_select import Stream, geometry, selections

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def ftaps(taps):
    return (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()


class Expected:
    """The oracle's bytes for a gather: words, offsets, N_c and L_c of every output chunk, n_i of every entry, the samples."""

    def __init__(self, O, x, start, length, sel, cw, m, taps):
        sel = np.asarray(sel, np.int64)
        words, self.offs, self.N, self.L, rows = [], [0], [], [], []
        for c0 in range(0, sel.size, cw):
            ent = sel[c0:c0 + cw]
            s = np.concatenate([x[start[g]:start[g] + length[g]] for g in ent])
            L = int(length[ent[0]])
            w = O.encode_chunk(s, (m, L) + ftaps(taps))
            words.append(w)
            rows.append(s)
            self.offs.append(self.offs[-1] + w.size)
            self.N.append(s.size)
            self.L.append(L)
        self.words = np.concatenate(words) if words else np.zeros(0, np.uint32)
        self.samples = np.concatenate(rows) if rows else np.zeros(0, np.int16)
        self.total = self.offs[-1]
        n_i = []  # the header chain of the expected bytes
        for c, c0 in enumerate(range(0, sel.size, cw)):
            at = self.offs[c] + 1
            for _ in sel[c0:c0 + cw]:
                n_i.append(int(self.words[at]))
                at += int(self.words[at]) + 1
            assert at == self.offs[c + 1]
        self.n_i = np.array(n_i, np.uint32)


def compare(g, want, total, what):
    """A Gathered against an Expected: bytes, offsets, total, geometry, side-band."""
    assert total == want.total == g.enc.total_words, (what, total, want.total)
    assert np.array_equal(g.enc.chunk_word_off.cpu().numpy(), np.array(want.offs, np.int64)), what
    got = g.enc.words[:total].cpu().numpy().view(np.uint32)
    assert got.tobytes() == want.words.tobytes(), (what, int(np.argmax(got != want.words)) if got.size == want.words.size else -1)
    assert g.chunk_samples.tolist() == want.N and g.wave_lens.tolist() == want.L, what
    assert np.array_equal(g.wave_words.cpu().numpy().view(np.uint32), want.n_i), what


def round_trip(ctx, g, want, what):
    """The result is a batch: its own plan decodes it to the gathered samples, with and without its side-band."""
    gp = g.plan(ctx)
    try:
        xs = torch.from_numpy(want.samples).to(ctx.device)
        assert torch.equal(gp.decode(g.enc), xs), what
        y = torch.empty_like(xs)
        run(ctx, gp, lambda: gp.decode_with_wave_words(g.enc.words, g.enc.chunk_word_off, g.wave_words, out=y,
                                                       in_words=g.enc.total_words))
        assert torch.equal(y, xs), (what, "side-band")
    finally:
        gp.close()


def valid_part(length, sel):
    """The entries of a refused list that have the commonest length of the list, in list order (any chunking of them is valid)."""
    sel = np.asarray(sel, np.int64)
    vals, counts = np.unique(length[sel], return_counts=True)
    return sel[length[sel] == vals[np.argmax(counts)]]


def check(ctx, O, st, x, m, taps, sel, cw, what, trips=True):
    """One list at one chunking, side-band off and on.  A list that breaks the one-length rule must be refused; its valid
    part is then gathered instead, and where a short waveform exists, a chunk that ends in it."""
    import deltarice_amd as dr
    sel = np.asarray(sel, np.int64)
    ok, bad = brute_force_gather(st.length, sel.tolist(), cw)
    if ok is None:
        for tab in (None, st.table):
            with pytest.raises(dr.DeltaRiceError) as e:
                st.plan.gather_encoded(st.enc, sel, cw, wave_words=tab)
            assert e.value.status == 1 and f"entry {bad} " in str(e.value), (what, bad, str(e.value))
        keep = valid_part(st.length, sel)
        short = sel[st.length[sel] < st.length[keep[0]]]
        if short.size:  # ... and a chunk that ends in the short one: cw - 1 whole ones in front of it
            n_front = min(cw, 7) - 1
            check(ctx, O, st, x, m, taps, np.concatenate([keep[:n_front], short[:1]]), n_front + 1, what + ("ends-short",), trips)
        sel = keep
    want = Expected(O, x, st.start, st.length, sel, cw, m, taps)
    for tab in (None, st.table):
        g = st.plan.gather_encoded(st.enc, sel, cw, wave_words=tab)
        assert st.plan.last_decode_path() == D.PATH_GATHER, what
        compare(g, want, g.enc.total_words, what + (tab is not None,))
        assert g.enc.words.numel() == want.total, what  # sized by the d_out == NULL call, allocated exactly
        if trips and tab is None:
            round_trip(ctx, g, want, what)


def make(ctx, O, name):
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    return Stream(ctx, O, x, Ns, Ls, m, taps), x, m, taps, rng


# --------------------------------------------------------------------------- 1, 2. every batch of the route table
@pytest.mark.parametrize("name", list(BATCHES))
def test_gather_every_batch(ctx, O, name):
    st, x, m, taps, rng = make(ctx, O, name)
    W = st.start.size
    try:
        for sname, sel in selections(st, rng).items():
            for cw in sorted({1, 7, max(1, len(sel))}):
                check(ctx, O, st, x, m, taps, sel, cw, (name, sname, cw))
        # all waveforms in order with the source's chunking: the source stream itself (uniform batches)
        if len(set(st.Ns)) == 1 and len(set(st.Ls)) == 1:
            g = st.plan.gather_encoded(st.enc, np.arange(W), W // len(st.Ns))
            assert g.enc.words[:g.enc.total_words].cpu().numpy().view(np.uint32).tobytes() == st.words.tobytes(), name
            assert np.array_equal(g.enc.chunk_word_off.cpu().numpy(), st.offs), name
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 3. the reference's own bytes
@pytest.mark.parametrize("name", golden_case_names())
def test_gather_golden(ctx, O, golden, name):
    import deltarice_amd as dr
    g = golden[name]
    o = g["opts"]
    x = O.decode_chunk(g["words"], o)
    L = o[1] if len(o) > 1 and 0 < o[1] < 0x80000000 else 0
    start, length, _ = geometry([x.size], [L])
    W = start.size
    plan = ctx.plan_uniform(1, x.size, o)
    enc = dr.EncodedBatch(torch.from_numpy(g["words"].view(np.int32)).to(ctx.device),
                          torch.tensor([0, g["words"].size], dtype=torch.int64, device=ctx.device), int(g["words"].size))
    try:
        same = plan.gather_encoded(enc, np.arange(W), W)  # all waveforms, in order, the source's waveforms per chunk
        assert plan.last_decode_path() == D.PATH_GATHER
        assert same.enc.total_words == g["words"].size
        assert same.enc.words.cpu().numpy().view(np.uint32).tobytes() == g["words"].tobytes(), name
        assert same.enc.chunk_word_off.cpu().tolist() == [0, g["words"].size]
        # reversed (a short last waveform stays last): the oracle's bytes for the reversed rows
        full = np.nonzero(length == length[0])[0]
        rev = np.concatenate([full[::-1], np.nonzero(length < length[0])[0]])
        if W > 1 and length[-1] < length[0]:
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.gather_encoded(enc, np.arange(W)[::-1], W)
            assert e.value.status == 1
        rice_m, taps = plan._rice_m, plan._taps
        want = Expected(O, x, start, length, rev, W, rice_m, taps)
        got = plan.gather_encoded(enc, rev, W)
        compare(got, want, got.enc.total_words, (name, "reversed"))
    finally:
        plan.close()


# --------------------------------------------------------------------------- 4. identity and re-chunking at size; both copy forms
def test_gather_rechunks_at_size_and_both_copy_forms_agree(ctx, O):
    st, x, m, taps, _ = make(ctx, O, "stream-quiet")  # 4 chunks of 2100 x 7000
    W = st.start.size
    every = np.arange(W)
    try:
        g4 = st.plan.gather_encoded(st.enc, every, 2100)
        assert st.plan.last_decode_path() == D.PATH_GATHER
        assert g4.enc.words.cpu().numpy().view(np.uint32).tobytes() == st.words.tobytes()
        assert np.array_equal(g4.enc.chunk_word_off.cpu().numpy(), st.offs)
        for cw in (W, 1):  # 1 chunk, 8400 chunks
            want = Expected(O, x, st.start, st.length, every, cw, m, taps)
            g = st.plan.gather_encoded(st.enc, every, cw)
            compare(g, want, g.enc.total_words, ("rechunk", cw))
            assert len(want.N) == (1 if cw == W else W)
            round_trip(ctx, g, want, ("rechunk", cw))
        # the copy form the code length does not choose: a workgroup per run of entries here
        perm = np.random.default_rng(4).permutation(W)
        a = st.plan.gather_encoded(st.enc, perm, 300)
        ctx.set_option("debug_flags", D.DBG_GATHER_OTHER_COPY)
        b = st.plan.gather_encoded(st.enc, perm, 300)
        ctx.set_option("debug_flags", 0)
        assert a.enc.total_words == b.enc.total_words and torch.equal(a.enc.words, b.enc.words)
        assert torch.equal(a.enc.chunk_word_off, b.enc.chunk_word_off) and torch.equal(a.wave_words, b.wave_words)
        want = Expected(O, x, st.start, st.length, perm, 300, m, taps)
        compare(b, want, b.enc.total_words, "tiles forced")
    finally:
        ctx.set_option("debug_flags", 0)
        st.plan.close()
    st, x, m, taps, _ = make(ctx, O, "short")  # ... and a wavefront per entry where the default is the tile
    try:
        full = np.nonzero(st.length == 100)[0]
        perm = np.random.default_rng(5).permutation(full)
        want = Expected(O, x, st.start, st.length, perm, 1000, m, taps)
        a = st.plan.gather_encoded(st.enc, perm, 1000)
        compare(a, want, a.enc.total_words, "tiles by default")
        ctx.set_option("debug_flags", D.DBG_GATHER_OTHER_COPY)
        b = st.plan.gather_encoded(st.enc, perm, 1000)
        ctx.set_option("debug_flags", 0)
        compare(b, want, b.enc.total_words, "waves forced")
        assert torch.equal(a.enc.words, b.enc.words)
    finally:
        ctx.set_option("debug_flags", 0)
        st.plan.close()


# --------------------------------------------------------------------------- 5. where the buffers lie
@pytest.mark.parametrize("name", ["short", "ragged", "long-2"])
def test_gather_placements(ctx, O, name):
    st, x, m, taps, rng = make(ctx, O, name)
    plan = st.plan
    W = st.start.size
    full = valid_part(st.length, np.arange(W))
    sel = np.concatenate([full[:1], full[-1:], rng.choice(full, 40), full[:3]])
    cw = 6
    want = Expected(O, x, st.start, st.length, sel, cw, m, taps)
    n_out = len(want.N)
    total_in = int(st.offs[-1])
    try:
        for flags in (0, D.DBG_GATHER_OTHER_COPY):
            ctx.set_option("debug_flags", flags)
            for pname, P in PLACEMENTS.items():
                for sideband in (False, True):
                    cell = (name, flags, pname, sideband)
                    ww = window(total_in + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
                    ww.t[:total_in].copy_(st.enc.words[:total_in])
                    ow = window(len(st.Ns) + 1, torch.int64, P["off"], device=ctx.device)
                    ow.t.copy_(st.enc.chunk_word_off)
                    tw = window(W, torch.int32, (P["w"] + 4) % 16, device=ctx.device)
                    tw.t.copy_(st.table)
                    out = window(want.total, torch.int32, P["x"] // 4 * 4, fill=FF, device=ctx.device)
                    oo = window(n_out + 1, torch.int64, (P["off"] + 8) % 16, fill=-1, device=ctx.device)
                    on = window(sel.size, torch.int32, P["y"] // 4 * 4, fill=FF, device=ctx.device)
                    total = run(ctx, plan, lambda: plan.gather_encoded_async(
                        ww.t, ow.t, sel, cw, out_words=out.t, in_words=total_in, wave_words=tw.t if sideband else None,
                        out_chunk_word_off=oo.t, out_wave_words=on.t))
                    assert plan.last_decode_path() == D.PATH_GATHER, cell
                    assert total == want.total, cell
                    assert out.t.cpu().numpy().view(np.uint32).tobytes() == want.words.tobytes(), cell
                    assert oo.t.cpu().tolist() == want.offs, cell
                    assert np.array_equal(on.t.cpu().numpy().view(np.uint32), want.n_i), cell
                    intact = all(w.intact() for w in (ww, ow, tw, out, oo, on))
                    assert intact, (cell, "guard written")
                    assert bool((ww.t[total_in:] == FF).all()), cell
                    assert torch.equal(tw.t, st.table) and torch.equal(ow.t, st.enc.chunk_word_off), cell
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


# --------------------------------------------------------------------------- 6. sizing and capacity
@pytest.mark.parametrize("name", ["short", "fir4"])
def test_gather_sizing_and_capacity(ctx, O, name):
    import deltarice_amd as dr
    st, x, m, taps, rng = make(ctx, O, name)
    plan = st.plan
    full = valid_part(st.length, np.arange(st.start.size))
    sel = rng.choice(full, 500)
    cw = 64
    want = Expected(O, x, st.start, st.length, sel, cw, m, taps)
    n_out = len(want.N)
    try:
        for flags in (0, D.DBG_GATHER_OTHER_COPY):
            ctx.set_option("debug_flags", flags)
            # d_out == NULL: the total and both tables, nothing else
            oo = window(n_out + 1, torch.int64, 8, fill=-1, device=ctx.device)
            on = window(sel.size, torch.int32, 4, fill=FF, device=ctx.device)
            total = run(ctx, plan, lambda: plan.gather_encoded_async(st.enc.words, st.enc.chunk_word_off, sel, cw, None,
                                                                     st.enc.total_words, None, oo.t, on.t))
            assert total == want.total and plan.last_decode_path() == D.PATH_GATHER
            assert oo.t.cpu().tolist() == want.offs and oo.intact()
            assert np.array_equal(on.t.cpu().numpy().view(np.uint32), want.n_i) and on.intact()
            # one word short: DRX_ERR_CAPACITY, finish reports the total needed, the output keeps every word it held
            short = window(want.total - 1, torch.int32, 4, fill=FF, device=ctx.device)
            ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
            plan.gather_encoded_async(st.enc.words, st.enc.chunk_word_off, sel, cw, short.t, st.enc.total_words)
            need = D.C.c_uint64()
            rc = ctx.lib.drx_plan_finish(plan._h, D.C.byref(need))
            assert rc == 3 and need.value == want.total, (rc, need.value)
            assert bool((short.t == FF).all()) and short.intact()
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.gather_encoded(st.enc, sel, cw, out_words=short.t)
            assert e.value.status == 3
            assert bool((short.t == FF).all()) and short.intact()
            # exactly the total: succeeds
            exact = window(want.total, torch.int32, 12, fill=FF, device=ctx.device)
            g = plan.gather_encoded(st.enc, sel, cw, out_words=exact.t)
            compare(g, want, g.enc.total_words, (name, flags, "exact"))
            assert exact.intact()
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


# --------------------------------------------------------------------------- 7. what is looked at, and what is reported
def test_gather_leaves_untouched_chunks_alone_and_reports_touched_ones(ctx, O):
    import deltarice_amd as dr
    n_chunks, Wc, L = 6, 40, 7000
    x = np.random.default_rng(5).normal(0, 10, n_chunks * Wc * L).astype(np.int16)
    st = Stream(ctx, O, x, [Wc * L] * n_chunks, [L] * n_chunks, 8)
    plan, good = st.plan, st.enc
    try:
        keep_c = (1, 4)
        sel = np.random.default_rng(6).permutation(np.nonzero(np.isin(st.chunk, keep_c))[0])
        want = Expected(O, x, st.start, st.length, sel, 16, 8, None)
        w = st.words.copy()
        for c in range(n_chunks):
            if c not in keep_c:
                w[st.offs[c]:st.offs[c + 1]] = 0xFFFFFFFF  # headers and payload
        poisoned = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)
        for tab in (None, st.table):
            g = plan.gather_encoded(poisoned, sel, 16, wave_words=tab)
            compare(g, want, g.enc.total_words, ("poisoned", tab is not None))
        # the header chain of one touched chunk: a waveform's n_i one too many
        at = int(st.offs[4]) + 1
        for _ in range(5):
            at += int(st.words[at]) + 1
        w = st.words.copy()
        w[at] += 1
        broken = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), good.chunk_word_off, good.total_words)
        for tab in (None, st.table):
            out = torch.full((want.total + 64,), FF, dtype=torch.int32, device=ctx.device)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.gather_encoded(broken, sel, 16, wave_words=tab, out_words=out)
            assert e.value.status == 4, tab is not None
            assert bool((out == FF).all())  # nothing is copied out of a batch that failed validation
            g = plan.gather_encoded(broken, sel[st.chunk[sel] == 1], 16, wave_words=tab)  # chunk 4 is not looked at
            assert g.enc.total_words > 0
        # a side-band table from another stream
        other = Stream(ctx, O, np.roll(x, 12345), st.Ns, st.Ls, 8)
        try:
            assert not torch.equal(other.table, st.table)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.gather_encoded(good, sel, 16, wave_words=other.table)
            assert e.value.status == 4
            # ... and handed straight to a call with a buffer (no sizing call in front): nothing is written, by either copy form
            for flags in (0, D.DBG_GATHER_OTHER_COPY):
                ctx.set_option("debug_flags", flags)
                out = torch.full((want.total + 64,), FF, dtype=torch.int32, device=ctx.device)
                ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
                plan.gather_encoded_async(good.words, good.chunk_word_off, sel, 16, out, good.total_words, other.table)
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.finish()
                assert e.value.status == 4 and bool((out == FF).all()), flags
            ctx.set_option("debug_flags", 0)
        finally:
            other.plan.close()
        g = plan.gather_encoded(good, sel, 16)  # the plan is still usable
        compare(g, want, g.enc.total_words, "after the errors")
    finally:
        plan.close()


def test_gather_looks_at_the_stream_every_time(ctx, O):
    """The same call twice with the stream rewritten in place in between (the next batch loaded into the same buffers): the
    second call gives the new batch's bytes, and DRX_ERR_CORRUPT where the new stream's header chain is broken.  Only the
    call right behind a sizing call may take that call's tables, and only once."""
    import deltarice_amd as dr
    n_chunks, Wc, L = 4, 30, 7000
    rng = np.random.default_rng(11)
    xa = rng.normal(0, 10, n_chunks * Wc * L).astype(np.int16)
    xb = rng.normal(0, 60, n_chunks * Wc * L).astype(np.int16)  # louder: other code lengths, other header positions
    a = Stream(ctx, O, xa, [Wc * L] * n_chunks, [L] * n_chunks, 8)
    b = Stream(ctx, O, xb, [Wc * L] * n_chunks, [L] * n_chunks, 8)
    plan = a.plan
    try:
        sel = rng.permutation(n_chunks * Wc)[:70]
        cw = 10
        wa = Expected(O, xa, a.start, a.length, sel, cw, 8, None)
        wb = Expected(O, xb, b.start, b.length, sel, cw, 8, None)
        assert wa.total != wb.total
        cap = max(int(a.offs[-1]), int(b.offs[-1]))  # one input buffer and one (upper-bound) output buffer for every call
        words = torch.zeros(cap, dtype=torch.int32, device=ctx.device)
        offs = torch.zeros(n_chunks + 1, dtype=torch.int64, device=ctx.device)
        out = torch.empty(max(wa.total, wb.total) + 16, dtype=torch.int32, device=ctx.device)

        def load(st, damage=None):
            w = st.words.copy()
            if damage is not None:
                w[damage] += 1
            words.fill_(FF)
            words[:w.size].copy_(torch.from_numpy(w.view(np.int32)).to(ctx.device))
            offs.copy_(torch.from_numpy(st.offs).to(ctx.device))

        def call(tab=None):
            out.fill_(FF)
            o, off, n_i = None, None, None
            def launch():
                nonlocal o, off, n_i
                o, off, n_i = plan.gather_encoded_async(words, offs, sel, cw, out, cap, tab)
            total = run(ctx, plan, launch)
            return total, off, n_i

        for flags in (0, D.DBG_GATHER_OTHER_COPY):
            ctx.set_option("debug_flags", flags)
            for tabs in ((None, None), (a.table, b.table)):
                load(a)
                total, off, n_i = call(tabs[0])
                assert total == wa.total and out[:total].cpu().numpy().view(np.uint32).tobytes() == wa.words.tobytes(), (flags, "a")
                load(b)  # the same addresses, the same list, the same capacities
                total, off, n_i = call(tabs[1])
                assert total == wb.total and off.cpu().tolist() == wb.offs, (flags, "b")
                assert out[:total].cpu().numpy().view(np.uint32).tobytes() == wb.words.tobytes(), (flags, "b")
                assert np.array_equal(n_i.cpu().numpy().view(np.uint32), wb.n_i) and bool((out[total:] == FF).all()), (flags, "b")
                at = int(b.offs[int(b.chunk[sel[0]])]) + 1  # the first header of a touched chunk: one word too many
                load(b, damage=at)
                with pytest.raises(dr.DeltaRiceError) as e:
                    call(tabs[1])
                assert e.value.status == 4 and bool((out == FF).all()), flags
        ctx.set_option("debug_flags", 0)
        # a sizing call hands its tables to the call behind it once: the call after that one walks again
        load(a)
        run(ctx, plan, lambda: plan.gather_encoded_async(words, offs, sel, cw, None, cap))
        total, _, _ = call()
        assert total == wa.total and out[:total].cpu().numpy().view(np.uint32).tobytes() == wa.words.tobytes()
        load(b)
        total, _, _ = call()
        assert total == wb.total and out[:total].cpu().numpy().view(np.uint32).tobytes() == wb.words.tobytes()
    finally:
        ctx.set_option("debug_flags", 0)
        a.plan.close()
        b.plan.close()


# --------------------------------------------------------------------------- 8. arguments
def test_gather_arguments(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = [7000 * 20 + 100] * 3, [7000] * 3
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, enc = st.plan, st.enc
    W = plan.total_waves
    lib = ctx.lib
    u64p = D.C.POINTER(D.C.c_uint64)
    try:
        out = torch.full((20000,), FF, dtype=torch.int32, device=ctx.device)
        off = torch.full((8,), -1, dtype=torch.int64, device=ctx.device)
        tab = torch.full((8,), FF, dtype=torch.int32, device=ctx.device)
        torch.cuda.synchronize()

        def call(idx, n_sel, cw, d_in=enc.words.data_ptr(), d_off=enc.chunk_word_off.data_ptr(), o=out.data_ptr(), cap=20000,
                 oo=off.data_ptr()):
            a = None if idx is None else np.asarray(idx, np.uint64)
            return lib.drx_gather_encoded(plan._h, d_in, enc.total_words, d_off, None if a is None else a.ctypes.data_as(u64p),
                                          n_sel, cw, o, cap, oo, tab.data_ptr())

        assert call([0, W], 2, 2) == 1                 # an index >= total_waves
        assert call([0, 1], 2, 0) == 1                 # out_chunk_waves == 0
        assert call([0, 1], 1 << 32, 2) == 1           # n_sel >= 2^32 (refused before the list is read)
        assert call([0, 1], 2, 2, d_in=None) == 1
        assert call([0, 1], 2, 2, d_off=None) == 1
        assert call(None, 2, 2) == 1
        assert call([0, 1], 2, 2, oo=None) == 1
        assert call([20, 0], 2, 2) == 1                # a whole waveform behind the short one
        assert b"entry 1 " in lib.drx_ctx_last_error(ctx._h)
        assert call([0, 20, 1], 3, 3) == 1             # ... in the middle of a chunk
        assert b"entry 1 " in lib.drx_ctx_last_error(ctx._h)
        assert call([20, 0], 2, 1) == 0                # ... alone in its chunk
        plan.finish()
        out.fill_(FF), off.fill_(-1), tab.fill_(FF)
        torch.cuda.synchronize()
        assert call([0, 1], 2, 2, o=None) == 1         # no buffer, but a capacity
        assert call(None, 0, 2, d_in=None, d_off=None, o=None, cap=0, oo=None) == 0  # n_sel == 0: DRX_OK
        plan.finish()
        assert bool((out == FF).all()) and bool((off == -1).all()) and bool((tab == FF).all())  # nothing was written
        # an output chunk of 2^31 samples or more: waveform 0 as often as it takes
        n_big = -(-(1 << 31) // 7000)
        assert call(np.zeros(n_big), n_big, n_big, o=None, cap=0) == 1 and b"2^31" in lib.drx_ctx_last_error(ctx._h)
        # the wrapper: the same refusals, and an empty list
        with pytest.raises(dr.DeltaRiceError):
            plan.gather_encoded(enc, [0, W], 2)
        with pytest.raises(dr.DeltaRiceError):
            plan.gather_encoded(enc, [0], 0)
        with pytest.raises(dr.DeltaRiceError):
            plan.gather_encoded(enc, torch.tensor([0], device=ctx.device), 1)  # a selection lives on the host
        g = plan.gather_encoded(enc, [], 5)
        assert g.enc.total_words == 0 and g.enc.chunk_word_off.cpu().tolist() == [0] and g.chunk_samples.size == 0
        # the plan's other calls around a gather
        want = Expected(O, x, st.start, st.length, np.array([5, 40, 20]), 3, 8, None)
        compare(plan.gather_encoded(enc, [5, 40, 20], 3), want, want.total, "gather")
        assert torch.equal(plan.decode(enc), st.xd)
        assert plan.last_decode_path() != D.PATH_GATHER
        st.check([41, 5, 62], False, "select after gather")
        compare(plan.gather_encoded(enc, [5, 40, 20], 3, wave_words=st.table), want, want.total, "gather after select")
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. a user's size
def test_gather_at_a_users_size(ctx, O):
    n_chunks, Wc, L = 100, 2000, 7000
    gen = torch.Generator(device=ctx.device).manual_seed(77)
    x = (torch.randn(n_chunks * Wc * L, device=ctx.device, generator=gen) * 10).to(torch.int16)
    plan = ctx.plan_uniform(n_chunks, Wc * L, (8, L))
    try:
        enc = plan.encode(x)
        table = plan.wave_words_device()
        rng = np.random.default_rng(77)
        W = n_chunks * Wc
        rows = x.view(-1, L)
        for sname, sel, cw in (("permutation", rng.permutation(W), Wc), ("one-percent", rng.choice(W, W // 100, replace=False), 500)):
            seld = torch.from_numpy(sel).to(ctx.device)
            for tab in (None, table):
                g = plan.gather_encoded(enc, sel, cw, wave_words=tab)
                assert plan.last_decode_path() == D.PATH_GATHER
                n_out = g.chunk_samples.size
                assert n_out == -(-sel.size // cw) and (g.wave_lens == L).all()
                offs = g.enc.chunk_word_off.cpu().numpy()
                for c in sorted({0, n_out // 2, n_out - 1}):  # spot chunks against the oracle's bytes
                    s = rows.index_select(0, seld[c * cw:(c + 1) * cw]).reshape(-1).cpu().numpy()
                    w = O.encode_chunk(s, (8, L))
                    assert g.enc.words[offs[c]:offs[c + 1]].cpu().numpy().view(np.uint32).tobytes() == w.tobytes(), (sname, c)
                gp = g.plan(ctx)  # ... the rest through the round trip
                try:
                    y = gp.decode(g.enc)
                    assert torch.equal(y.view(-1, L), rows.index_select(0, seld)), (sname, tab is not None)
                    del y
                finally:
                    gp.close()
    finally:
        plan.close()
