"""GPU: the end-of-payload verdict of the seven calls that read the stream a lane per waveform through the shared reader
(csrc/drx_lane_reader.inc): drx_wave_stats, drx_wave_bins, drx_decode_window, drx_decode_windows, drx_find_pulses,
drx_transcode, drx_transcode_filter.

The shape is the smallest that reaches every branch of the reader: 2 chunks of 70 waveforms x 100 samples, m = 8 -- three
wavefronts, the last partly filled, a wavefront whose lanes lie in two chunks, a masked last group (100 = 6 x 16 + 4) -- and
the same ragged: chunk 2 with WaveformLength 37 and a last waveform of 11 samples (rag_order's wavefronts).  Both geometries
run the serial kernels as well (a general prediction filter: csrc/drx_lane_stream.h's serial_frame()).

One waveform's payload is made a word too SHORT (its last word cut: the codes end after it) or a word too LONG (a zero word
appended: the codes end before it), its header word and the chunk offsets mended, so that every walk accepts the chain and it
is the lane that has to notice.  Each call then reports DRX_ERR_CORRUPT -- except drx_decode_window with a head window, which
reads no payload beyond its window's last code: it reports nothing and its rows are numpy's over the oracle's input.
drx_wave_bins parses every waveform to its end whatever its bins cover, and drx_decode_windows is given a window that reaches
every waveform's end.  The undamaged streams are held to the numpy models of the five calls and to the oracle's stream at the
new parameter and under the new filter."""
import numpy as np
import pytest

from decode_window_reference import windows
from decode_windows_reference import windows_multi
from deltarice_amd import _lib as D
from find_pulses_reference import find_pulses
from test_gpu_select import Stream, header_table
from wave_bins_reference import wave_bins
from wave_stats_reference import wave_stats_heads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M = 8
SHAPES = {  # name -> (Ns, Ls, taps)
    "uniform": ([70 * 100] * 2, [100] * 2, None),
    "ragged": ([70 * 100, 69 * 37 + 11], [100, 37], None),
    "serial": ([70 * 100] * 2, [100] * 2, (1, -2, 1)),
    "serial_ragged": ([70 * 100, 69 * 37 + 11], [100, 37], (1, -2, 1)),
}
# (chunk, waveform): an ordinary lane of the first wavefront, the two lanes either side of the chunk border, the batch's last
# waveform (in the ragged shape the short one)
VICTIMS = [(0, 5), (0, 69), (1, 0), (1, 69)]


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


@pytest.fixture(scope="module")
def streams(ctx, O):
    out = {}
    for name, (Ns, Ls, taps) in SHAPES.items():
        x = np.random.default_rng(len(name)).normal(0, 10, sum(Ns)).astype(np.int16)
        out[name] = (Stream(ctx, O, x, Ns, Ls, M, taps), x)
    yield out
    for st, _ in out.values():
        st.plan.close()


def damaged(ctx, st, c, i, by):
    """(EncodedBatch, side-band) of st with waveform i of chunk c a word shorter (by = -1) or longer (by = +1)"""
    import deltarice_amd as dr
    at = int(st.offs[c]) + 1
    for _ in range(i):
        at += int(st.words[at]) + 1
    n = int(st.words[at])
    L = int(st.length[int(np.flatnonzero(st.chunk == c)[0]) + i])
    assert (L * 4 + 31) // 32 <= n + by <= (L * 25 + 31) // 32  # (a header every walk accepts at k = 3)
    payload = st.words[at + 1:at + 1 + n]
    payload = payload[:-1] if by < 0 else np.concatenate([payload, [np.uint32(0)]])
    w = np.concatenate([st.words[:at], [np.uint32(n + by)], payload, st.words[at + 1 + n:]]).astype(np.uint32)
    offs = st.offs.copy()
    offs[c + 1:] += by
    enc = dr.EncodedBatch(torch.from_numpy(w.view(np.int32)).to(ctx.device), torch.from_numpy(offs).to(ctx.device), int(offs[-1]))
    table = torch.from_numpy(header_table(w, offs, st.Ns, st.Ls).view(np.int32)).to(ctx.device)
    return enc, table


FIR4 = (1, -1, 1, -1)  # the target of drx_transcode_filter: the fast kernels behind the delta source, the serial ones behind `serial`


def two_windows(plan):
    """starts [W, 2] of drx_decode_windows: sample 60 and sample 0 -- with a width of 100 the second reaches every waveform's end"""
    return torch.tensor([[60, 0]], dtype=torch.int64, device=plan.ctx.device).repeat(plan.total_waves, 1)


CALLS = {
    "wave_stats": lambda plan, enc, kw: plan.wave_stats(enc, head=40, **kw),
    "wave_bins": lambda plan, enc, kw: plan.wave_bins(enc, 10, 2, **kw),  # (the bins end at sample 20)
    "decode_windows": lambda plan, enc, kw: plan.decode_windows(enc, two_windows(plan), 100, **kw),
    "refilter": lambda plan, enc, kw: plan.refilter(enc, FIR4, 32, **kw),
    "decode_window": lambda plan, enc, kw: plan.decode_window(enc, None, 100, **kw),  # (every waveform to its end)
    "find_pulses": lambda plan, enc, kw: plan.find_pulses(enc, 20, 1, 1, 3, **kw),
    "transcode": lambda plan, enc, kw: plan.transcode(enc, 32, **kw),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_clean_stream(ctx, O, streams, shape):
    st, x = streams[shape]
    Ns, Ls, taps = SHAPES[shape]
    geom = (st.start, st.length, st.chunk)
    for kw in ({}, dict(wave_words=st.table)):
        assert torch.equal(st.plan.wave_stats(st.enc, head=40, **kw), torch.from_numpy(wave_stats_heads(x, Ns, Ls, [40])[0]).to(ctx.device))
        for width in (8, 24, 100):
            assert torch.equal(st.plan.decode_window(st.enc, None, width, pad=-3, **kw),
                               torch.from_numpy(windows(x, Ns, Ls, None, 0, width, -3, geom)).to(ctx.device)), width
        n, p = find_pulses(x, Ns, Ls, 20, 1, 1, 3, None, geom)
        gn, gp = st.plan.find_pulses(st.enc, 20, 1, 1, 3, **kw)
        assert torch.equal(gn, torch.from_numpy(n).to(ctx.device)) and torch.equal(gp, torch.from_numpy(p).to(ctx.device))
        for bin, n_bins in ((10, 2), (16, 7), (17, 3)):
            assert torch.equal(st.plan.wave_bins(st.enc, bin, n_bins, **kw), torch.from_numpy(wave_bins(x, Ns, Ls, bin, n_bins)).to(ctx.device)), bin
        starts = two_windows(st.plan)
        assert torch.equal(st.plan.decode_windows(st.enc, starts, 100, pad=-3, **kw),
                           torch.from_numpy(windows_multi(x, Ns, Ls, starts.cpu().numpy(), None, 0, 100, -3, geom)).to(ctx.device))
        # (the oracle's stream of the same samples under the new filter, byte for byte: the sources' leads are +-1)
        t = st.plan.refilter(st.enc, FIR4, 32, **kw)
        want, at = [], 0
        for N, L in zip(Ns, Ls):
            want.append(O.encode_chunk(x[at:at + N], (32, L, len(FIR4)) + tuple(v & 0xFFFFFFFF for v in FIR4)))
            at += N
        want = np.concatenate(want)
        assert t.enc.total_words == want.size
        assert np.array_equal(t.enc.words[:want.size].cpu().numpy().view(np.uint32), want)
        if taps is None:  # (the oracle's stream at the new parameter, byte for byte: a filter with lead +-1)
            t = st.plan.transcode(st.enc, 32, **kw)
            want, at = [], 0
            for N, L in zip(Ns, Ls):
                want.append(O.encode_chunk(x[at:at + N], (32, L)))
                at += N
            want = np.concatenate(want)
            assert t.enc.total_words == want.size
            assert np.array_equal(t.enc.words[:want.size].cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("by", [-1, 1], ids=["codes end after the last word", "codes end before the last word"])
@pytest.mark.parametrize("victim", VICTIMS, ids=lambda v: f"chunk{v[0]}-wave{v[1]}")
@pytest.mark.parametrize("shape", list(SHAPES))
def test_payload_a_word_off_is_corrupt(ctx, streams, shape, victim, by):
    import deltarice_amd as dr
    st, x = streams[shape]
    enc, table = damaged(ctx, st, *victim, by)
    for name, call in CALLS.items():
        for kw in ({}, dict(wave_words=table)):
            with pytest.raises(dr.DeltaRiceError) as e:
                call(st.plan, enc, kw)
            assert e.value.status == 4, (name, sorted(kw))


@pytest.mark.parametrize("by", [-1, 1], ids=["shorter", "longer"])
@pytest.mark.parametrize("victim", VICTIMS[:3], ids=lambda v: f"chunk{v[0]}-wave{v[1]}")  # (waveforms longer than the windows)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_head_window_does_not_report_damage_behind_it(ctx, streams, shape, victim, by):
    st, x = streams[shape]
    Ns, Ls, _ = SHAPES[shape]
    enc, table = damaged(ctx, st, *victim, by)
    for width in (8, 24):  # a masked group alone; an unmasked one and a masked one
        want = torch.from_numpy(windows(x, Ns, Ls, None, 0, width, -3, (st.start, st.length, st.chunk))).to(ctx.device)
        for kw in ({}, dict(wave_words=table)):
            got = st.plan.decode_window(enc, None, width, pad=-3, **kw)
            assert st.plan.last_decode_path() == D.PATH_WINDOW and st.plan.finish() == 0, (width, sorted(kw))
            assert torch.equal(got, want), (width, sorted(kw))
