"""k_encode_stream at a waveform's edges: the trailing partial tile on the full tile's arithmetic (code_tail_tile /
put_tail_tile, drx_encode.h), its load as tile n_full of the load pipeline, and the pipeline's unconditional prologue and
refills (for_tiles) -- encoded words, chunk offsets and wave_words byte for byte the oracle's, then the round trip.

Every case runs the persistent encoder twice: with the grid it would get, and with DBG_STREAM_THREE_WGS (two coding
workgroups), where each of eight wavefronts codes hundreds of waveforms and goes around its ring many times.  The samples
are a view with 4 KiB of sentinel (0x7FFF in front, -0x8000 behind) directly around the batch, so the batch's last waveform
ends where the buffer's payload ends: a sample from outside that took part in a code changes the stream, and a write shows
in the sentinels.  (A read whose value is discarded is not visible this way; that no lane addresses anything outside
[x, x + len) is by construction: for_tiles clamps a lane's first sample to len - 8.)"""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from deltarice_amd.codec import EncodedBatch
from test_gpu_placement import window
from test_gpu_routes import make_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STREAM = D.DBG_NO_LONG_PATHS | D.DBG_NO_PIECES | D.DBG_FORCE_STREAM
LENGTHS = (8, 16, 504, 512, 513, 519, 520, 1023, 1024, 1368, 7000, 7001, 7004, 7007)
# for_tiles takes its loop from three full tiles on: exactly three, three and a tail of one lane's part, of one lane,
# four with no tail (a refill beyond the last tile), six and a tail (two rounds of the loop, nothing left behind it)
LOOP_EDGES = (1536, 1537, 1544, 2048, 3080)
WAVES = 700  # waveforms per chunk, three chunks


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.set_option("debug_flags", 0)
    c.set_option("encode_impl", 2)
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def reference(O, x, Ns, Ls, m, taps):
    """-> (words, chunk_word_off, n_i of every waveform), all from the oracle's stream."""
    ftaps = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()
    words, offs, nis, at = [], [0], [], 0
    for N, L in zip(Ns, Ls):
        w = O.encode_chunk(x[at:at + N], ((m, L) if L else (m,)) + ftaps)
        assert int(w[0]) == N
        pos = 1
        for _ in range(-(-N // L) if L else 1):
            nis.append(int(w[pos]))
            pos += 1 + int(w[pos])
        assert pos == w.size
        words.append(w)
        offs.append(offs[-1] + w.size)
        at += N
    return np.concatenate(words), np.array(offs, np.int64), np.array(nis, np.uint32)


def check(ctx, O, x, Ns, Ls, m=8, taps=None, x_offset=0):
    assert x.size == sum(Ns) and x.dtype == np.int16
    ref_w, ref_off, ref_n = reference(O, x, Ns, Ls, m, taps)
    ref_w_d = torch.from_numpy(ref_w.view(np.int32)).to(ctx.device)
    ref_off_d = torch.from_numpy(ref_off).to(ctx.device)
    plan = make_plan(ctx, list(Ns), list(Ls), m, taps)
    xw = window(plan.total_samples, torch.int16, x_offset, guard=(0x7FFF, -0x8000), device=ctx.device)
    xw.t.copy_(torch.from_numpy(x))
    try:
        ctx.set_option("encode_impl", 2)
        for flags in (STREAM, STREAM | D.DBG_STREAM_THREE_WGS):
            cell = (Ls[0], m, taps, x_offset, flags)
            ctx.set_option("debug_flags", flags)
            ww = window(plan.max_encoded_words, torch.int32, 0, fill=-1, device=ctx.device)
            ow = window(len(Ns) + 1, torch.int64, 0, fill=-1, device=ctx.device)
            ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
            plan.encode_async(xw.t, ww.t, ow.t)
            total = plan.finish()
            assert plan.last_encode_path() == D.ENC_STREAM, cell
            n_i = plan.wave_words()
            assert total == ref_w.size, cell
            assert torch.equal(ow.t, ref_off_d), cell
            assert torch.equal(ww.t[:total], ref_w_d), cell
            assert np.array_equal(n_i, ref_n), cell
            assert xw.intact() and ww.intact() and ow.intact(), cell
            y = plan.decode(EncodedBatch(ww.t, ow.t, total))
            assert torch.equal(y, xw.t), cell
    finally:
        ctx.set_option("debug_flags", 0)
        plan.close()


def uniform(L, waves=WAVES, short_last=True):
    """Three chunks of `waves` waveforms of L samples, and (short_last) a shorter waveform of L // 3 behind them."""
    N = waves * L + (L // 3 if short_last else 0)
    return [N] * 3, [L] * 3


def noise(seed, n, sigma=10):
    return np.random.default_rng(seed).normal(0, sigma, n).astype(np.int16)


@pytest.mark.parametrize("L", LENGTHS + LOOP_EDGES)
def test_trailing_tile_content(ctx, O, L):
    """No full tile at all (8, 16, 504), exactly full tiles (512, 1024), one lane with 1..7 samples (513, 519, 1023, 7001,
    7004, 7007), lanes with eight samples or none (520, 1368, 7000: the headline's 344-sample tail)."""
    Ns, Ls = uniform(L)
    check(ctx, O, noise(L, sum(Ns)), Ns, Ls)


@pytest.mark.parametrize("L", (7000, 1368))
def test_escapes_in_the_trailing_tile(ctx, O, L):
    """Full-range samples: every code is an escape, 8 x 25 = 200 bits per lane, so the trailing tile takes emit_tile (at
    L = 1368 into the ring; at L = 7000 the waveform outgrows the ring and is coded again to its place)."""
    Ns, Ls = uniform(L, waves=300)
    x = np.random.default_rng(L + 1).integers(-32768, 32768, sum(Ns), dtype=np.int16)
    check(ctx, O, x, Ns, Ls)


@pytest.mark.parametrize("L", (7000, 1368))
def test_one_spike_in_the_trailing_tile(ctx, O, L):
    """sigma = 10 with one sample of 30000 among the last 344 of every third waveform: two escapes in one lane."""
    Ns, Ls = uniform(L, short_last=False)
    x = noise(L + 2, sum(Ns))
    rng = np.random.default_rng(L + 3)
    for w in range(0, 3 * WAVES, 3):
        x[(w + 1) * L - 1 - int(rng.integers(0, 344))] = 30000
    check(ctx, O, x, Ns, Ls)


@pytest.mark.parametrize("m,L,sigma", [(1, 7000, 1), (1, 1368, 1), (32768, 7000, 3000), (32768, 1368, 3000)])
def test_rice_parameters(ctx, O, m, L, sigma):
    """k = 0 and k = 15 (m = 8 is every other test): at k = 15 a code is 16 bits or more, a lane's eight exactly 128."""
    Ns, Ls = uniform(L)
    check(ctx, O, noise(m + L, sum(Ns), sigma), Ns, Ls, m=m)


@pytest.mark.parametrize("L", (7000, 7001))
def test_general_filter(ctx, O, L):
    """taps (1, -1, 1, -1): the GEN instantiation through the trailing tile."""
    Ns, Ls = uniform(L)
    check(ctx, O, noise(L + 4, sum(Ns), 20), Ns, Ls, taps=(1, -1, 1, -1))


@pytest.mark.parametrize("x_offset", (2, 8))
@pytest.mark.parametrize("L", (7000, 7001))
def test_misaligned_input(ctx, O, L, x_offset):
    Ns, Ls = uniform(L)
    check(ctx, O, noise(L + x_offset, sum(Ns)), Ns, Ls, x_offset=x_offset)


@pytest.mark.parametrize("L", (519, 520, 7000, 7001))
def test_last_waveform_ends_the_buffer(ctx, O, L):
    """The batch's last waveform is a whole one: its trailing tile's load, issued three tiles ahead, is the last read of a
    buffer with sentinels behind it."""
    Ns, Ls = uniform(L, short_last=False)
    check(ctx, O, noise(L + 5, sum(Ns)), Ns, Ls)


def test_ragged_batch(ctx, O):
    """Chunks of different WaveformLengths (locate_uniform's other branch), every length of the list, a shorter last
    waveform in each."""
    Ls = list(LENGTHS)
    Ns = [L * 150 + L // 3 for L in Ls]
    check(ctx, O, noise(99, sum(Ns)), Ns, Ls)
