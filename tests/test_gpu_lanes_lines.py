"""k_decode_lanes with one 128-byte stream piece in flight per lane: the streams whose refills differ.

Every case is a small batch held bit for bit to the oracle, both ways: the decode of the ORACLE's stream and the round trip
through the encoder.  The lanes decoder is forced (decode_impl 7 behind a walk of its own, or decode_impl 8 without the
parallel walks for the fused-walk instantiation; never the long-waveform paths) and last_decode_path() is asserted.  Where the
oracle's stream is decoded the encoded buffer has exactly total_words words, so the last pieces take the guarded loads (the
round trip decodes the encoder's own, larger buffer), and every output lies in a window between sentinels that are checked
afterwards.

  phases        96 x 330 samples, sigma varied per waveform: the waveforms' first payload words cover all 32 residues mod 32,
                i.e. every position of a stream's start inside a 128-byte piece (asserted on the CPU from the oracle's sizes)
  noise         70 x 700 uniform int16 noise under m = 8: 25 bits per sample, 50 words per round -- more than any piece
  zeros         70 x 700 zeros: k + 1 bits per sample exactly, a piece lasts four rounds
  zeros-noise   350 zeros then noise, and noise-zeros: the rule for holding and committing a piece across a jump in rate
  ragged        WaveformLengths 1, 2, 63, 64, 65, 127, 128, 129, 700, each chunk's last waveform shorter than the rest
"""
import numpy as np
import pytest

from deltarice_amd import _lib as D

gpu = pytest.mark.gpu  # (test_phases_cover_a_piece needs neither a GPU nor torch)

try:
    import torch
except ImportError:  # the GPU tests skip on their own then
    torch = None

M = 8
FIR4 = (1, -1, 1, -1)
GUARD = 4096  # bytes of sentinel on each side of a window
S16 = 0x5A5A
RAGGED_L = (1, 2, 63, 64, 65, 127, 128, 129, 700)
PHASES_LEN = 330  # five interior rounds: a piece is requested, held across rounds and committed from every phase
PHASES_SEED = 96  # (a shuffle of the sigmas under which test_phases_cover_a_piece holds, with and without the filter)


def _samples(name):
    """(chunk sample counts, WaveformLengths, int16 samples)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "phases":
        sig = np.geomspace(1.5, 3000.0, 96)
        np.random.default_rng(PHASES_SEED).shuffle(sig)
        x = (rng.normal(0, 1, (96, PHASES_LEN)) * sig[:, None]).clip(-32768, 32767).astype(np.int16)
        return [96 * PHASES_LEN], [PHASES_LEN], x.reshape(-1)
    if name == "ragged":
        Ns = [L * 66 + L // 2 for L in RAGGED_L]
        return Ns, list(RAGGED_L), rng.normal(0, 30, sum(Ns)).astype(np.int16)
    noise = rng.integers(-32768, 32768, (70, 700)).astype(np.int16)
    x = {"noise": noise, "zeros": np.zeros_like(noise)}.get(name)
    if x is None:
        x = noise.copy()
        if name == "zeros-noise":
            x[:, :350] = 0
        else:
            assert name == "noise-zeros"
            x[:, 350:] = 0
    return [70 * 700], [700], x.reshape(-1)


CASES = ("phases", "noise", "zeros", "zeros-noise", "noise-zeros", "ragged")
GEN_CASES = CASES[:5]  # the line phases and every hungry / frugal variant


def _opts(L, taps):
    return (M, L) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())


def first_payload_words(words, offs, Ns, Ls):
    """Index in the batch's word array of every waveform's first payload word (chunk: its sample count, then n_i and n_i
    words per waveform)."""
    at = []
    for c, (N, L) in enumerate(zip(Ns, Ls)):
        w = int(offs[c])
        assert int(words[w]) == N, (c, int(words[w]))
        n_waves = -(-N // L)
        w += 1
        for _ in range(n_waves):
            at.append(w + 1)
            w += 1 + int(words[w])
        assert w == int(offs[c + 1]), c
    return np.array(at)


class Case:
    """One batch, its oracle stream on the device and a plan; shared by the cells of a case."""

    def __init__(self, ctx, name, taps):
        from oracle import oracle as O
        from test_gpu_routes import make_plan
        self.name, self.taps = name, taps
        self.Ns, self.Ls, x = _samples(name)
        words, offs, at = [], [0], 0
        for N, L in zip(self.Ns, self.Ls):
            w = O.encode_chunk(x[at:at + N], _opts(L, taps))
            words.append(w)
            offs.append(offs[-1] + w.size)
            at += N
        self.words, self.offs = np.concatenate(words), np.array(offs, dtype=np.int64)
        self.total = int(offs[-1])
        self.xd = torch.from_numpy(x).to(ctx.device)
        self.plan = make_plan(ctx, self.Ns, self.Ls, M, taps)


def window(device, n, dtype, byte_offset, sentinel):
    """(base, view): n elements at byte_offset past a 16-byte boundary, GUARD bytes of sentinel on each side"""
    es = torch.empty(0, dtype=dtype).element_size()
    lo = (GUARD + byte_offset) // es
    base = torch.full((lo + n + GUARD // es,), sentinel, dtype=dtype, device=device)
    assert base.data_ptr() % 128 == 0
    return base, base[lo:lo + n], lo


def decode_cell(ctx, case, impl, flags, want_path, word_byte_offset=0):
    """Decodes the oracle's stream from a buffer of exactly total_words words into a window between sentinels."""
    plan = case.plan
    wbase, ww, _ = window(ctx.device, case.total, torch.int32, word_byte_offset, -1)  # 0xFFFFFFFF around the stream
    ww.copy_(torch.from_numpy(case.words.view(np.int32)))
    off = torch.from_numpy(case.offs).to(ctx.device)
    ybase, yw, lo = window(ctx.device, plan.total_samples, torch.int16, 0, S16)
    ctx.set_option("decode_impl", impl)
    ctx.set_option("debug_flags", flags)
    try:
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.decode_async(ww, off, yw, in_words=case.total)
        plan.finish()
        cell = (case.name, case.taps, impl, flags, word_byte_offset)
        assert plan.last_decode_path() == want_path, (cell, plan.last_decode_path())
        assert torch.equal(yw, case.xd), cell
        assert bool((ybase[:lo] == S16).all().item()) and bool((ybase[lo + plan.total_samples:] == S16).all().item()), cell
    finally:
        ctx.set_option("decode_impl", 8)
        ctx.set_option("debug_flags", 0)


def round_trip_cell(ctx, case, impl, flags, want_path):
    """The encoder's stream is the oracle's, word for word, and decodes to the samples."""
    plan = case.plan
    enc = plan.encode(case.xd)
    assert enc.total_words == case.total, case.name
    assert np.array_equal(enc.chunk_word_off.cpu().numpy(), case.offs), case.name
    assert np.array_equal(enc.words[:case.total].cpu().numpy().view(np.uint32), case.words), case.name
    ybase, yw, lo = window(ctx.device, plan.total_samples, torch.int16, 0, S16)
    ctx.set_option("decode_impl", impl)
    ctx.set_option("debug_flags", flags)
    try:
        plan.decode(enc, out=yw)
        assert plan.last_decode_path() == want_path, (case.name, plan.last_decode_path())
        assert torch.equal(yw, case.xd), (case.name, case.taps, impl, flags)
        assert bool((ybase[:lo] == S16).all().item()) and bool((ybase[lo + plan.total_samples:] == S16).all().item()), case.name
    finally:
        ctx.set_option("decode_impl", 8)
        ctx.set_option("debug_flags", 0)


LANES = (7, D.DBG_NO_LONG_PATHS, D.PATH_LANES)                                  # k_decode_lanes<false, GEN> behind its walk
FUSED = (8, D.DBG_NO_LONG_PATHS | D.DBG_NO_PARALLEL_WALKS, D.PATH_LANES_FUSED)  # k_decode_lanes<true, GEN>


@pytest.fixture(scope="module")
def ctx():
    if torch is None:
        pytest.skip("torch not found")
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    made = {}

    def get(name, taps=None):
        if (name, taps) not in made:
            made[(name, taps)] = Case(ctx, name, taps)
        return made[(name, taps)]
    yield get
    for c in made.values():
        c.plan.close()


def test_phases_cover_a_piece():
    """CPU part of "phases": a first payload word at every residue mod 32 (the stream starts at word 0 of a 128-byte
    aligned buffer, so the residue is the word's place in its 128-byte line)."""
    from oracle import oracle as O
    Ns, Ls, x = _samples("phases")
    for taps in (None, FIR4):
        w = O.encode_chunk(x, _opts(Ls[0], taps))
        at = first_payload_words(w, [0, w.size], Ns, Ls)
        assert len(at) == 96 and set(at % 32) == set(range(32)), (taps, sorted(set(range(32)) - set(at % 32)))


@gpu
@pytest.mark.parametrize("name", CASES)
def test_lanes_decode_oracle_stream(ctx, cases, name):
    case = cases(name)
    if name == "phases":
        assert set(first_payload_words(case.words, case.offs, case.Ns, case.Ls) % 32) == set(range(32))
    decode_cell(ctx, case, *LANES)
    decode_cell(ctx, case, *LANES, word_byte_offset=4)  # 4 bytes off a 16-byte boundary: every piece by guarded dword loads
    round_trip_cell(ctx, case, *LANES)


@gpu
@pytest.mark.parametrize("name", ("phases", "ragged"))
def test_lanes_fused_walk(ctx, cases, name):
    case = cases(name)
    decode_cell(ctx, case, *FUSED)
    decode_cell(ctx, case, *FUSED, word_byte_offset=4)
    round_trip_cell(ctx, case, *FUSED)


@gpu
@pytest.mark.parametrize("name", GEN_CASES)
def test_lanes_general_filter(ctx, cases, name):
    case = cases(name, FIR4)
    decode_cell(ctx, case, *LANES)
    decode_cell(ctx, case, *LANES, word_byte_offset=4)
    round_trip_cell(ctx, case, *LANES)
    if name == "phases":
        decode_cell(ctx, case, *FUSED)
