"""GPU: drx_transcode / drx_estimate_words_encoded -- an encoded batch re-coded at another RiceParameter without decoding.

The streams are the oracle's (oracle.encode_chunk), the expectations the oracle's bytes at the target parameter (for a filter
whose lead is not +-1: the oracle's decode of both streams), the comparisons tobytes() / torch.equal.  Every cell asserts
DRX_PATH_TRANSCODE alone."""
import ctypes as C
import math

import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_offsets64 import PAD, SMALL, Small, big  # noqa: F401  (big: the never-filled 17 GB buffer, a fixture)
from test_gpu_placement import FF, run, window
from test_gpu_select import Stream, header_table
from test_gpu_wave_stats import crafted_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGE = ([130 * 200 + 37] * 3, [200] * 3)  # 131 waveforms per chunk: two wavefronts and two lanes, the last one of 37 samples


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


def opts_of(m, L, taps):
    return ((m, L) if L else (m,)) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())


class Want:
    """The oracle's stream of the samples y at RiceParameter m: words, offsets, n_i table."""

    def __init__(self, O, y, Ns, Ls, m, taps=None):
        chunks, offs, at = [], [0], 0
        for N, L in zip(Ns, Ls):
            chunks.append(O.encode_chunk(y[at:at + N], opts_of(m, L, taps)))
            offs.append(offs[-1] + chunks[-1].size)
            at += N
        self.words, self.offs, self.total = np.concatenate(chunks), np.array(offs, np.uint64), int(offs[-1])
        self.n_i = header_table(self.words, offs, Ns, Ls)


def same_stream(t, want, what):
    """A Transcoded against a Want: total, offsets table, side-band, every word."""
    w, offs = t.enc.to_numpy()
    assert t.enc.total_words == want.total, (what, t.enc.total_words, want.total)
    assert offs.tobytes() == want.offs.tobytes(), (what, "offsets")
    assert t.wave_words.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes(), (what, "wave words")
    if w.tobytes() != want.words.tobytes():
        bad = np.nonzero(w != want.words)[0]
        raise AssertionError((what, f"{bad.size} words differ, the first at {int(bad[0])}", hex(int(w[bad[0]])), hex(int(want.words[bad[0]]))))


def check(ctx, st, want, m2, sidebands=(False, True), decodes_to=None, what=""):
    for sideband in sidebands:
        t = st.plan.transcode(st.enc, rice_m=m2, wave_words=st.table if sideband else None)
        assert st.plan.last_decode_path() == D.PATH_TRANSCODE, (what, m2, sideband)
        assert t.rice_m == m2
        same_stream(t, want, (what, m2, sideband))
    if decodes_to is not None:
        p2 = t.plan(ctx)
        try:
            assert torch.equal(p2.decode(t.enc), decodes_to), (what, m2, "decode of the result")
        finally:
            p2.close()


# --------------------------------------------------------------------------- 1. every small batch, five targets
@pytest.mark.parametrize("name", list(SMALL))
def test_transcode_every_batch(ctx, O, name):
    Ns, Ls, m, taps, sigma = SMALL[name]
    assert not taps or taps[0] in (1, -1)  # (byte-exact against the oracle's encode of the samples)
    x = np.random.default_rng(sum(map(ord, name))).normal(0, sigma, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m, taps)
    try:
        for m2 in sorted({1, 8, 32, 32768, m}):
            check(ctx, st, Want(O, x, Ns, Ls, m2, taps), m2, decodes_to=st.xd, what=name)
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 2. edges of the lane kernel
def test_transcode_wavefront_edges(ctx, O):
    Ns, Ls = EDGE
    x = np.random.default_rng(2).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        for m2 in (1, 8, 32, 32768):
            check(ctx, st, Want(O, x, Ns, Ls, m2), m2, decodes_to=st.xd, what="edges")
    finally:
        st.plan.close()


def test_transcode_short_waveforms(ctx, O):
    Ls = [1, 15, 16, 17, 63, 64, 65]
    Ns = [70 * L + L // 2 for L in Ls]  # 70 waveforms each, and a shorter last one where there is room for it
    x = np.random.default_rng(22).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    try:
        for m2 in (1, 8, 32, 32768):
            check(ctx, st, Want(O, x, Ns, Ls, m2), m2, decodes_to=st.xd, what="short waveforms")
    finally:
        st.plan.close()


@pytest.mark.parametrize("m", [1, 8, 64, 32768])
def test_transcode_rice_parameters(ctx, O, m):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    for sigma in (10, 400):
        x = np.random.default_rng(m + sigma).normal(0, sigma, sum(Ns)).astype(np.int16)
        st = Stream(ctx, O, x, Ns, Ls, m)
        try:
            for m2 in (1, 16, 32768):
                check(ctx, st, Want(O, x, Ns, Ls, m2), m2, sidebands=(False,), decodes_to=st.xd, what=(m, sigma))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 3. crafted rows
def test_transcode_crafted_rows(ctx, O):
    x = crafted_rows(W=70, L=70000)
    W, L = x.shape
    x = x.reshape(-1)
    st = Stream(ctx, O, x, [W * L], [L], 8)
    try:
        for m2 in (1, 4096):
            check(ctx, st, Want(O, x, [W * L], [L], m2), m2, sidebands=(False,), decodes_to=st.xd, what="crafted")
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 4. a lead that is not +-1
@pytest.mark.parametrize("taps", [(2, -1), (-3, 1, 1)])
def test_transcode_other_leads(ctx, O, taps):
    Ns, Ls = [65 * 300], [300]
    x = np.random.default_rng(len(taps)).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8, taps)
    try:
        y = O.decode_chunk(st.words, opts_of(8, 300, taps))
        for m2 in (1, 32, 32768):
            for sideband in (False, True):
                t = st.plan.transcode(st.enc, rice_m=m2, wave_words=st.table if sideband else None)
                assert st.plan.last_decode_path() == D.PATH_TRANSCODE
                w, offs = t.enc.to_numpy()
                assert offs.tolist() == [0, w.size] and int(w[0]) == Ns[0]
                assert O.decode_chunk(w, opts_of(m2, 300, taps)).tobytes() == y.tobytes(), (taps, m2, sideband)
                assert t.wave_words.cpu().numpy().view(np.uint32).tobytes() == header_table(w, offs, Ns, Ls).tobytes()
            p2 = t.plan(ctx)
            try:
                assert p2.decode(t.enc).cpu().numpy().tobytes() == y.tobytes(), (taps, m2, "decode of the result")
            finally:
                p2.close()
        t = st.plan.transcode(st.enc, rice_m=8)  # the plan's own parameter: the input, word for word
        assert t.enc.total_words == st.enc.total_words and t.enc.to_numpy()[0].tobytes() == st.words.tobytes()
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 5. codes no encoder writes
def pack_chunk(waves):
    """waves: per waveform a list of (value, bits) codes -> the chunk's words, N | { n_i | payload_i }."""
    out = [sum(len(w) for w in waves)]
    for codes in waves:
        bits = "".join(format(v, "0%db" % n) for v, n in codes)
        bits += "0" * (-len(bits) % 32)
        out += [len(bits) // 32] + [int(bits[i:i + 32], 2) for i in range(0, len(bits), 32)]
    return np.array(out, np.uint32)


def code_of(z, k, escape=None):
    """The code of zig-zag value z at k as (value, bits): ordinary where z >> k < 8 unless an escape is asked for."""
    q = z >> k
    if escape is None:
        escape = q >= 8
    return ((1 << 16) | z, 25) if escape else ((1 << k) | (z & ((1 << k) - 1)), q + 1 + k)


def test_transcode_noncanonical_codes(ctx, O):
    rng = np.random.default_rng(5)
    W, L = 67, 100
    # k = 3: one code in four an escape that carries a value an ordinary code would hold
    small = [[code_of(int(z), 3, escape=bool(e)) for z, e in zip(rng.integers(0, 64, L), rng.integers(0, 4, L) == 0)] for _ in range(W)]
    # k = 15: ordinary codes with q up to 7, values up to 2^18 - 1, which fold to int16 as the decoder folds them
    wide = [[code_of(int(z), 15, escape=False) for z in rng.integers(0, 1 << 18, L)] for _ in range(W)]
    assert any(bits >= 2 + 1 + 15 for w in wide for _, bits in w)  # (q >= 2: the value does not fit 16 bits)
    for k, waves, targets in ((3, small, (1, 8, 32)), (15, wide, (1, 8, 32768))):
        words = pack_chunk(waves)
        y = O.decode_chunk(words, (1 << k, L))
        st = Stream(ctx, O, y, [W * L], [L], 1 << k)  # (its plan and geometry; the stream under test is the packed one)
        try:
            import deltarice_amd as dr
            enc = dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device),
                                  torch.tensor([0, words.size], dtype=torch.int64, device=ctx.device), int(words.size))
            assert st.words.tobytes() != words.tobytes()
            assert torch.equal(st.plan.decode(enc), st.xd)
            for m2 in targets:
                t = st.plan.transcode(enc, rice_m=m2)
                assert st.plan.last_decode_path() == D.PATH_TRANSCODE
                same_stream(t, Want(O, y, [W * L], [L], m2), ("non-canonical", k, m2))
        finally:
            st.plan.close()


# --------------------------------------------------------------------------- 6. the estimate
@pytest.mark.parametrize("name", ["edges", "ragged"])
def test_estimate_words_encoded(ctx, O, name):
    Ns, Ls, m = (EDGE + (8,)) if name == "edges" else SMALL["ragged"][:3]
    x = np.random.default_rng(6).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, m)
    try:
        want = [Want(O, x, Ns, Ls, 1 << k).total for k in range(16)]
        for sideband in (False, True):
            got = st.plan.estimate_words_encoded(st.enc, wave_words=st.table if sideband else None)
            assert st.plan.last_decode_path() == D.PATH_TRANSCODE
            assert got.dtype == np.uint64 and got.tolist() == want, (name, sideband)
        assert int(got[int(math.log2(m))]) == st.enc.total_words
        best = int(np.argmin(want))
        t = st.plan.transcode(st.enc)
        assert t.rice_m == 1 << best and t.enc.total_words == want[best]
        same_stream(t, Want(O, x, Ns, Ls, 1 << best), (name, "best"))
    finally:
        st.plan.close()


# --------------------------------------------------------------------------- 7. where the buffers lie, and how large
def test_transcode_placements_and_capacity(ctx, O):
    Ns, Ls = EDGE
    x = np.random.default_rng(7).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, total, W = st.plan, st.enc.total_words, st.plan.total_waves
    want = Want(O, x, Ns, Ls, 32)
    slack = 67
    try:
        for ib in (0, 4, 8, 12):
            ww = window(total + slack, torch.int32, ib, fill=FF, guard=FF, device=ctx.device)
            ww.t[:total].copy_(st.enc.words[:total])
            for ob in (0, 4, 8, 12):
                for fill in (FF, 0):
                    cell = (ib, ob, fill)
                    yw = window(want.total, torch.int32, ob, fill=fill, device=ctx.device)  # out_cap_words = the total
                    ow = window(len(Ns) + 1, torch.int64, 8 if ob & 4 else 0, fill=fill, device=ctx.device)
                    nw = window(W, torch.int32, ob, fill=fill, device=ctx.device)
                    assert ww.t.data_ptr() % 16 == ib and yw.t.data_ptr() % 16 == ob
                    got = run(ctx, plan, lambda: plan.transcode_async(ww.t, st.enc.chunk_word_off, 32, yw.t, total, None, ow.t, nw.t))
                    assert got == want.total and plan.last_decode_path() == D.PATH_TRANSCODE, cell
                    assert yw.t.cpu().numpy().view(np.uint32).tobytes() == want.words.tobytes(), cell
                    assert ow.t.cpu().numpy().view(np.uint64).tobytes() == want.offs.tobytes(), cell
                    assert nw.t.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes(), cell
                    assert yw.intact() and ow.intact() and nw.intact() and ww.intact(), cell
            assert bool((ww.t[total:] == FF).all()), ib
        # one word short: DRX_ERR_CAPACITY at finish, the total NEEDED reported, the whole window still holding its fill
        for fill in (FF, 0):
            yw = window(want.total - 1, torch.int32, 4, fill=fill, device=ctx.device)
            ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
            plan.transcode_async(st.enc.words, st.enc.chunk_word_off, 32, yw.t, total)
            n = C.c_uint64()
            assert ctx.lib.drx_plan_finish(plan._h, C.byref(n)) == 3 and n.value == want.total
            assert bool((yw.t == fill).all()) and yw.intact(), fill
        # the sizing call: both tables and nothing else
        ow = window(len(Ns) + 1, torch.int64, 8, fill=-1, device=ctx.device)
        nw = window(W, torch.int32, 4, fill=-1, device=ctx.device)
        got = run(ctx, plan, lambda: plan.transcode_async(st.enc.words, st.enc.chunk_word_off, 32, None, total, None, ow.t, nw.t))
        assert got == want.total
        assert ow.t.cpu().numpy().view(np.uint64).tobytes() == want.offs.tobytes() and ow.intact()
        assert nw.t.cpu().numpy().view(np.uint32).tobytes() == want.n_i.tobytes() and nw.intact()
        # arguments: DRX_ERR_ARG, nothing launched
        lib, w, off = ctx.lib, st.enc.words.data_ptr(), st.enc.chunk_word_off.data_ptr()
        assert lib.drx_transcode(plan._h, w, total, off, 16, None, 0, ow.t.data_ptr(), None) == 1
        assert lib.drx_transcode(plan._h, None, total, off, 5, None, 0, ow.t.data_ptr(), None) == 1
        assert lib.drx_transcode(plan._h, w, total, None, 5, None, 0, ow.t.data_ptr(), None) == 1
        assert lib.drx_transcode(plan._h, w, total, off, 5, None, 0, None, None) == 1
        assert lib.drx_transcode(plan._h, w, total, off, 5, None, 10, ow.t.data_ptr(), None) == 1
        assert plan.finish() == want.total  # (the status word as the sizing call left it)
    finally:
        plan.close()


# --------------------------------------------------------------------------- 8. corrupt input
def test_transcode_corrupt_input(ctx, O):
    import deltarice_amd as dr
    Ns, Ls = EDGE
    x = np.random.default_rng(8).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan, good = st.plan, st.enc
    want = Want(O, x, Ns, Ls, 32)
    words, offs = st.words, st.offs

    def header_at(c, i):  # word index of waveform i's header in chunk c
        at = int(offs[c]) + 1
        for _ in range(i):
            at += int(words[at]) + 1
        return at

    def batch_of(w, o=None, total=None):
        o = offs if o is None else o
        return dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), torch.from_numpy(np.asarray(o, np.int64)).to(ctx.device),
                               int(o[-1]) if total is None else total)

    cases = {}
    # one n_i shortened by a word, the chain repaired: the payload's last word leaves the stream, everything behind moves up
    h = header_at(1, 70)
    n = int(words[h])
    w = np.delete(words, h + n)
    w[h] = n - 1
    o = offs.copy()
    o[2:] -= 1
    cases["n_i shortened, chain repaired"] = batch_of(w, o)
    # a payload word zeroed
    h = header_at(0, 5)
    w = words.copy()
    w[h + 3] = 0
    cases["payload word zeroed"] = batch_of(w)
    # a payload's last word dropped: of a waveform in the middle (its header keeps its n_i), and of the stream's last one
    h = header_at(2, 100)
    cases["last word dropped"] = batch_of(np.delete(words, h + int(words[h])), total=good.total_words - 1)
    cases["stream a word short"] = dr.EncodedBatch(good.words, good.chunk_word_off, good.total_words - 1)
    cap = plan.max_encoded_words
    try:
        for cname, enc in cases.items():
            for fill in (FF, 0):
                yw = window(cap, torch.int32, 4, fill=fill, device=ctx.device)
                with pytest.raises(dr.DeltaRiceError) as e:
                    run(ctx, plan, lambda: plan.transcode_async(enc.words, enc.chunk_word_off, 32, yw.t, enc.total_words))
                assert e.value.status == 4, cname
                assert bool((yw.t == fill).all()) and yw.intact(), (cname, fill)
            with pytest.raises(dr.DeltaRiceError) as e:
                plan.estimate_words_encoded(enc)
            assert e.value.status == 4, cname
            same_stream(plan.transcode(good, rice_m=32), want, (cname, "the call after"))  # the plan stays usable
    finally:
        plan.close()


# --------------------------------------------------------------------------- 9. input offsets beyond 2^32 words
def test_transcode_large_input_offsets(ctx, O, big):  # noqa: F811
    from deltarice_amd.codec import EncodedBatch
    case = Small(ctx, "short")
    want = Want(O, case.x, case.Ns, case.Ls, 32)
    try:
        for B in case.bases()[2:]:  # 2^32 - h and 2^32 + 5
            big[B - PAD:B + case.total + PAD].fill_(-1)
            big[B:B + case.total].copy_(torch.from_numpy(case.words.view(np.int32)))
            enc = EncodedBatch(big, torch.from_numpy(case.offs + B).to(ctx.device), B + case.total)
            for table in (None, case.side):
                t = case.plan.transcode(enc, rice_m=32, wave_words=table)
                assert case.plan.last_decode_path() == D.PATH_TRANSCODE
                same_stream(t, want, ("short", B, table is not None))
            assert case.plan.estimate_words_encoded(enc)[5] == want.total
            torch.cuda.synchronize()
            assert bool((big[B - PAD:B] == -1).all().item()) and bool((big[B + case.total:B + case.total + PAD] == -1).all().item()), B
    finally:
        case.plan.close()


# --------------------------------------------------------------------------- 10. among the plan's other calls
def test_transcode_in_sequence_on_one_plan(ctx, O):
    Ns, Ls = [65 * 300] * 2, [300] * 2
    x = np.random.default_rng(10).normal(0, 10, sum(Ns)).astype(np.int16)
    st = Stream(ctx, O, x, Ns, Ls, 8)
    plan = st.plan
    want = Want(O, x, Ns, Ls, 64)
    try:
        ctx.set_option("profile", 1)
        enc = plan.encode(st.xd)
        assert enc.total_words == st.enc.total_words and torch.equal(enc.words[:enc.total_words], st.enc.words)
        out = torch.empty(plan.max_encoded_words, dtype=torch.int32, device=ctx.device)
        t = plan.transcode(enc, rice_m=64, out_words=out)
        assert plan.last_decode_path() == D.PATH_TRANSCODE
        ms = plan.last_timings()
        assert len(ms) == 4 and all(math.isfinite(v) and v >= 0 for v in ms) and ms[3] > 0, ms
        same_stream(t, want, "in sequence")
        assert plan.wave_words().tobytes() == header_table(st.words, st.offs, Ns, Ls).tobytes()  # the SOURCE's n_i
        assert torch.equal(plan.decode(enc), st.xd) and plan.last_decode_path() != D.PATH_TRANSCODE  # (the plan's m is still 8)
        assert plan.encode(st.xd).total_words == st.enc.total_words
    finally:
        ctx.set_option("profile", 0)
        plan.close()
