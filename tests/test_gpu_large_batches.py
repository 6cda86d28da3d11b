"""Batches of more than 2^32 samples -- and one of more than 2^32 encoded words -- on the routes that
test_gpu_parity.py::test_full_size_headline_batch does not take: 64-bit sample, word and waveform indices, and launches of
more than 2^32 wavefront-threads, held to the oracle and to the samples bit for bit.

Every Gaussian geometry is a prefix x[:T] of ONE seeded tensor of 4.4e9 int16 samples (sigma = 10), seen as its own
(n_chunks, W, L); n_chunks is the smallest count with T >= 2^32 + 2 N (N = W L samples per chunk): the smallest batch in which
an index needs bit 32 and two whole chunks lie behind the boundary.  Per encoder cell: chunk_word_off against the running sum
of 1 + W + sum n_i (uint64), five spot chunks against the oracle's bytes (chunk 0, the chunks holding samples 2^31 and 2^32,
the chunk after that, the last), the whole stream against the first cell's word for word, last_encode_path(); per decoder
cell: torch.equal with x[:T] and last_decode_path().  RiceParameter 8 throughout.

The expected paths are what route_encode() (drx_api_encode.hip), route_decode() (drx_decode_kernels.hip) and route_walk()
(drx_walk.hip) say for these geometries, with 309 chunks (271 of the long waveforms) and k = 3:
  runs-512     L 512 is no packed run (a multiple of 8 BELOW 512) but 14 waveforms make a run of the pieces encoder: PIECES for
               encode_impl 2 and 1.  309 chunks are more than the 224 the block-parallel walk reads: the walk runs inside the
               lanes launch (LDS block walkers, LANES_FUSED) with or without DBG_NO_PARALLEL_WALKS; decode_impl 7 puts the serial
               walk (k_walk_block) in front of k_decode_lanes (LANES).
  packed-64    packed runs of 105 waveforms: PIECES.  6.76e7 waveforms are more than a launch of a wavefront each can carry
               (2^26 - 8): the two-pass encoder goes out in slices, drx_estimate_words gives a wavefront 258 waveforms; FUSED and
               SEGMENTS do not admit the batch, so that encode_impl 1 without the pieces encoder is the two-pass encoder too.
  fused-7000   the headline geometry: STREAM, FUSED under encode_impl 1, PIECES when forced.  Chunk-wide walk by chains in front
               of k_decode_lanes (LANES) -- DBG_WALK_BY_SCAN changes nothing above 224 chunks --, scalar-load walkers inside the
               launch without the parallel walks (LANES_FUSED).
  long-500000  STREAM_SEGS (72 segments a waveform), PIECES over several workgroups under encode_impl 1; 8672 waveforms: the
               block decoder, the inverse of (1, -1, 1, -1) inside it (8672 >= 768 resident workgroups: IIR_FUSED) or behind
               it (DBG_IIR_SEPARATE: k_iir_tiles, IIR).
  fir5         five taps: the two-pass encoder and k_decode_simple behind the serial walk, whatever encode_impl.
  ragged       WaveformLengths above and below 65 536 in one batch: SEGMENTS under encode_impl 2 and 1.  138 short-waveform and
               171 long-waveform chunks (at most 224 each): both parallel walks, a lanes launch behind each, or one behind both
               (DBG_RAGGED_ONE_LANES_LAUNCH): LANES.
k_decode_long has no cell here (a workgroup per waveform; tests/test_gpu_offsets64.py holds it)."""
import numpy as np
import pytest

from deltarice_amd import _lib as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TWO31, TWO32 = 1 << 31, 1 << 32
X_SAMPLES = 4_400_000_000
M = 8
FIR4 = (1, -1, 1, -1)
FIR5 = (1, -1, 1, -1, 1)
GIB = 1 << 30


def n_chunks_for(N):
    """The fewest chunks of N samples with T >= 2^32 + 2 N"""
    return -(-(TWO32 + 2 * N) // N)


# name: (waveforms per chunk, WaveformLength, taps or None, chunks as the rule gives them)
UNIFORM = {
    "runs-512": (27343, 512, None, 309),
    "packed-64": (218750, 64, None, 309),
    "fused-7000": (2000, 7000, None, 309),
    "long-500000": (32, 500000, None, 271),
    "long-500000-fir4": (32, 500000, FIR4, 271),
    "fir5": (14000, 1000, FIR5, 309),
}

# config 5's mix at about 14 M samples a chunk (test_gpu_parity.py::test_ragged_mixed_waveform_lengths, scaled): leftover
# waveforms of 17, 1 and 5 samples, one waveform that is its whole chunk (WaveformLength 0)
RAGGED_NS = [512 * 27343, 2048 * 6835 + 17, 7000 * 2000, 16384 * 854, 7000 * 1999 + 1, 512 * 27300, 16384 * 853 + 5, 2048 * 6836, 14_000_321]
RAGGED_LS = [512, 2048, 7000, 16384, 7000, 512, 16384, 2048, 0]

# (encode_impl, debug flags, DRX_ENC_* expected); the first cell's stream is the one the others are compared with
ENCODE = {
    "runs-512": [(2, 0, D.ENC_PIECES), (1, 0, D.ENC_PIECES), (0, 0, D.ENC_TWO_PASS)],
    "packed-64": [(2, 0, D.ENC_PIECES), (0, 0, D.ENC_TWO_PASS), (1, D.DBG_NO_PIECES | D.DBG_NO_LONG_PATHS, D.ENC_TWO_PASS)],
    "fused-7000": [(2, 0, D.ENC_STREAM), (1, 0, D.ENC_FUSED), (0, 0, D.ENC_TWO_PASS), (2, D.DBG_FORCE_PIECES, D.ENC_PIECES)],
    "long-500000": [(2, 0, D.ENC_STREAM_SEGS), (1, 0, D.ENC_PIECES)],
    "long-500000-fir4": [(2, 0, D.ENC_STREAM_SEGS), (1, 0, D.ENC_PIECES)],
    "fir5": [(2, 0, D.ENC_TWO_PASS), (0, 0, D.ENC_TWO_PASS)],
    "ragged": [(2, 0, D.ENC_SEGMENTS), (1, 0, D.ENC_SEGMENTS), (0, 0, D.ENC_TWO_PASS)],
}
# (decode_impl, debug flags, DRX_PATH_* bits expected)
DECODE = {
    "runs-512": [(8, 0, D.PATH_LANES_FUSED), (8, D.DBG_NO_PARALLEL_WALKS, D.PATH_LANES_FUSED), (7, 0, D.PATH_LANES)],
    "packed-64": [(8, 0, D.PATH_LANES_FUSED)],
    "fused-7000": [(8, 0, D.PATH_LANES), (8, D.DBG_NO_PARALLEL_WALKS, D.PATH_LANES_FUSED), (8, D.DBG_WALK_BY_SCAN, D.PATH_LANES),
                   (8, D.DBG_NO_LONG_PATHS, D.PATH_LANES)],
    "long-500000": [(8, 0, D.PATH_BLOCKS)],
    "long-500000-fir4": [(8, 0, D.PATH_BLOCKS | D.PATH_IIR_FUSED), (8, D.DBG_IIR_SEPARATE, D.PATH_BLOCKS | D.PATH_IIR)],
    "fir5": [(8, 0, D.PATH_SIMPLE)],
    "ragged": [(8, 0, D.PATH_LANES), (8, D.DBG_RAGGED_ONE_LANES_LAUNCH, D.PATH_LANES)],
}


def ragged_geometry():
    """config 5's nine chunks again and again until T >= 2^32 + 2 N for the largest N among them"""
    Ns, Ls = [], []
    while sum(Ns) < TWO32 + 2 * max(RAGGED_NS):
        Ns.append(RAGGED_NS[len(Ns) % len(RAGGED_NS)])
        Ls.append(RAGGED_LS[len(Ls) % len(RAGGED_LS)])
    return Ns, Ls


def test_geometries_follow_the_rule():
    """(no GPU work) the chunk counts written above are the rule's, every prefix fits the tensor and passes 2^32 by two chunks"""
    for name, (W, L, _, n) in UNIFORM.items():
        N = W * L
        assert n == n_chunks_for(N), name
        assert (n - 1) * N < TWO32 + 2 * N <= n * N <= X_SAMPLES, name
    assert UNIFORM["packed-64"][0] * 309 * 64 >= TWO32  # a wavefront per waveform: more threads than a launch carries
    Ns, Ls = ragged_geometry()
    assert len(Ns) == 309 and sum(Ns) <= X_SAMPLES and sum(Ns) - Ns[-1] < TWO32 + 2 * max(RAGGED_NS) <= sum(Ns)
    assert sum(1 for L in Ls if 0 < L <= 2048) == 138  # (short- and long-waveform chunks: 224 at most each for the parallel walks)


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.set_option("debug_flags", 0)
    c.set_option("encode_impl", 2)
    c.set_option("decode_impl", 8)
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def fill(x, make, slab=1 << 28):
    for s0 in range(0, x.numel(), slab):
        n = min(slab, x.numel() - s0)
        x[s0:s0 + n] = make(n)
    torch.cuda.synchronize()
    return x


class Gauss:
    """The module's Gaussian tensor: made when a test first asks for it, dropped by the test that needs its memory."""

    def __init__(self, ctx):
        self.ctx, self.x = ctx, None

    def need(self, gib):
        """Skips unless `gib` GiB are free beside the tensor (8.2 GiB more where it does not exist yet)."""
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(self.ctx.device)
        want = gib * GIB + (0 if self.x is not None else 2 * X_SAMPLES)
        if free < want:
            pytest.skip(f"needs {want / GIB:.0f} GiB of free HBM")

    def get(self):
        if self.x is None:
            dev = self.ctx.device
            g = torch.Generator(device=dev).manual_seed(2 ** 32 + 1)
            self.x = fill(torch.empty(X_SAMPLES, dtype=torch.int16, device=dev),
                          lambda n: torch.randn(n, device=dev, generator=g).mul_(10.0).to(torch.int16))
        return self.x

    def drop(self):
        self.x = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def gauss(ctx):
    g = Gauss(ctx)
    yield g
    g.drop()


def oracle_opts(L, taps):
    return ((M, L) if L else (M,)) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())


def spot_chunks(Ns):
    """chunk 0, the chunks holding samples 2^31 and 2^32, the chunk after that one, the last chunk"""
    ends = np.cumsum(np.asarray(Ns, dtype=np.uint64))
    at31, at32 = (int(np.searchsorted(ends, b, side="right")) for b in (TWO31, TWO32))
    assert at32 + 2 <= len(Ns) - 1  # (two whole chunks behind the boundary)
    return sorted({0, at31, at32, at32 + 1, len(Ns) - 1})


def check_batch(ctx, O, x, plan, Ns, Ls, taps, encode_cells, decode_cells, spots=None, name=""):
    """Every encoder cell against the framing, the oracle's spot chunks and the first cell; every decoder cell against x.
    -> the first cell's encoded batch"""
    n = len(Ns)
    Wc = np.array([-(-N // (L or N)) for N, L in zip(Ns, Ls)], dtype=np.int64)
    wave_base = np.concatenate(([0], np.cumsum(Wc)))
    sample_off = np.concatenate(([0], np.cumsum(np.asarray(Ns, dtype=np.int64))))
    assert plan.total_samples == int(sample_off[-1]) == x.numel() and plan.total_waves == int(wave_base[-1])
    want_bytes = {}
    ref = None
    try:
        for eimpl, flags, want_enc in encode_cells:
            cell = (name, "encode", eimpl, flags)
            ctx.set_option("encode_impl", eimpl)
            ctx.set_option("debug_flags", flags)
            enc = plan.encode(x)
            assert plan.last_encode_path() == want_enc, (cell, plan.last_encode_path())
            # 1. the framing: chunk_word_off is the running sum of 1 + W + sum n_i
            nw = plan.wave_words()
            per_chunk = np.add.reduceat(nw.astype(np.uint64), wave_base[:-1]) + np.uint64(1) + Wc.astype(np.uint64)
            off = enc.chunk_word_off.cpu().numpy().astype(np.uint64)
            assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(per_chunk, dtype=np.uint64)), cell
            assert int(off[-1]) == enc.total_words, cell
            # 2. spot chunks against the oracle
            for c in (spot_chunks(Ns) if spots is None else spots(off)):
                if c not in want_bytes:
                    xc = x[int(sample_off[c]):int(sample_off[c + 1])].cpu().numpy()
                    want_bytes[c] = O.encode_chunk(xc, oracle_opts(Ls[c], taps)).tobytes()
                assert enc.chunk_bytes(c) == want_bytes[c], (cell, c)
            # 3. every encoder the same stream
            if ref is None:
                ref = enc
            else:
                assert torch.equal(enc.chunk_word_off, ref.chunk_word_off), cell
                assert torch.equal(enc.words[:enc.total_words], ref.words[:ref.total_words]), cell
            del enc, nw
        ctx.set_option("encode_impl", 2)
        # 4. every decoder the samples
        for dimpl, flags, want_path in decode_cells:
            cell = (name, "decode", dimpl, flags)
            ctx.set_option("decode_impl", dimpl)
            ctx.set_option("debug_flags", flags)
            y = plan.decode(ref)
            assert plan.last_decode_path() == want_path, (cell, plan.last_decode_path())
            assert torch.equal(y, x), cell
            del y
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("encode_impl", 2)
        ctx.set_option("decode_impl", 8)
    return ref


def uniform_case(ctx, O, gauss, name):
    W, L, taps, n = UNIFORM[name]
    N = W * L
    x = gauss.get()[:n * N]
    plan = ctx.plan_uniform(n, N, oracle_opts(L, taps))
    try:
        enc = check_batch(ctx, O, x, plan, [N] * n, [L] * n, taps, ENCODE[name], DECODE[name], name=name)
        if taps is None:  # drx_estimate_words, 33 / 3 / 1 waveforms to a wavefront: its entry for this RiceParameter is the batch's size
            assert int(plan.estimate_words(x)[3]) == enc.total_words, name
    finally:
        plan.close()


# free HBM asked for beside the Gaussian tensor: two encoded batches at their capacity (25 bits per sample: 12.6 GiB each), a
# decoded batch (8.1 GiB), the plan's tables (16 bytes per waveform and the encoders' look-back state: 3 GiB for packed-64)
@pytest.mark.parametrize("name,gib", [("runs-512", 36), ("fused-7000", 35), ("long-500000", 35), ("long-500000-fir4", 35), ("fir5", 35)])
def test_uniform_batches_past_2_32_samples(ctx, O, gauss, name, gib):
    gauss.need(gib)
    uniform_case(ctx, O, gauss, name)


def reference_sizes(x, n_chunks, W, L):
    """Encoded words of a uniform delta-filter batch for RiceParameter 2^k, k = 0 ... 15, by the format's rules in plain
    tensor arithmetic: a code is q + 1 + k bits (q = z >> k below 8) or 25, a waveform 1 + ceil(bits / 32) words, a chunk one
    more.  uint64 sums."""
    sizes = [n_chunks] * 16
    rows = 16 * W  # waveforms per slab
    xs = x.view(-1, L)
    for r0 in range(0, xs.shape[0], rows):
        v = xs[r0:r0 + rows].to(torch.int32)
        d = v.clone()
        d[:, 1:] -= v[:, :-1]
        d = ((d + 32768) & 0xFFFF) - 32768  # int16 arithmetic
        z = (d << 1) ^ (d >> 31)
        for k in range(16):
            q = z >> k
            bits = torch.where(q < 8, q + (1 + k), torch.full_like(q, 25)).sum(dim=1, dtype=torch.int64)
            sizes[k] += int((1 + ((bits + 31) >> 5)).sum().item())
    return sizes


def test_packed_runs_and_more_waveforms_than_a_launch_carries(ctx, O, gauss):
    """packed-64: 6.76e7 waveforms, 4.33e9 wavefront-threads, of which a launch takes only those modulo 2^32.  The pieces
    encoder, the two-pass encoder (launched in slices; FUSED and SEGMENTS do not admit the batch) and drx_estimate_words (258
    waveforms to a wavefront) against reference_sizes(), which is held to the oracle on a piece of the chunk that holds
    sample 2^32 and to the encoded batch itself at k = 3."""
    gauss.need(38)
    name = "packed-64"
    W, L, taps, n = UNIFORM[name]
    N = W * L
    x = gauss.get()[:n * N]
    plan = ctx.plan_uniform(n, N, (M, L))
    try:
        assert plan.total_waves * 64 >= TWO32
        ref = check_batch(ctx, O, x, plan, [N] * n, [L] * n, taps, ENCODE[name], DECODE[name], name=name)
        total_words = ref.total_words
        del ref
        piece = x[(TWO32 // N) * N:][:4096 * L]
        want_piece = reference_sizes(piece, 1, 4096, L)
        piece_host = piece.cpu().numpy()
        for k in range(1, 16):  # (the oracle's RiceParameter is 2^k, at least 2)
            assert want_piece[k] == O.encode_chunk(piece_host, (1 << k, L)).size, k
        want = reference_sizes(x, n, W, L)
        assert want[3] == total_words
        got = plan.estimate_words(x)
        assert [int(v) for v in got] == want
    finally:
        plan.close()


def test_ragged_batch_past_2_32_samples(ctx, O, gauss):
    gauss.need(36)
    Ns, Ls = ragged_geometry()
    x = gauss.get()[:sum(Ns)]
    plan = ctx.plan(Ns, Ls, M)
    try:
        check_batch(ctx, O, x, plan, Ns, Ls, None, ENCODE["ragged"], DECODE["ragged"], name="ragged")
    finally:
        plan.close()


def test_select_and_gather_past_2_32_samples(ctx, O, gauss):
    """fused-7000's stream: 4096 waveforms -- 1024 at random, the 1024 around the waveform holding sample 2^31 (512 below
    it, itself, 511 above), the same around sample 2^32, the batch's last 1024 -- decoded alone, with and without the
    side-band, and gathered into a batch of chunks of 2000."""
    gauss.need(24)
    W, L, _, n = UNIFORM["fused-7000"]
    N = W * L
    x = gauss.get()[:n * N]
    total_waves = n * W
    rng = np.random.default_rng(7000)
    idx = np.concatenate([rng.integers(0, total_waves, 1024), np.arange(TWO31 // L - 512, TWO31 // L + 512),
                          np.arange(TWO32 // L - 512, TWO32 // L + 512), np.arange(total_waves - 1024, total_waves)]).astype(np.int64)
    rng.shuffle(idx)
    assert idx.size == 4096 and idx.max() * L > TWO32
    plan = ctx.plan_uniform(n, N, (M, L))
    gplan = None
    try:
        enc = plan.encode(x)
        assert plan.last_encode_path() == D.ENC_STREAM
        side = plan.wave_words_device()
        want = x.view(-1, L).index_select(0, torch.from_numpy(idx).to(ctx.device))
        for table in (None, side):
            y = plan.decode_select(enc, idx, wave_words=table)
            assert plan.last_decode_path() == D.PATH_SELECT
            assert torch.equal(y, want), table is not None
            del y
        for table in (None, side):
            g = plan.gather_encoded(enc, idx, 2000, wave_words=table)
            assert plan.last_decode_path() == D.PATH_GATHER
            assert g.chunk_samples.tolist() == [2000 * L, 2000 * L, 96 * L] and g.wave_lens.tolist() == [L] * 3
            assert torch.equal(g.wave_words, side[torch.from_numpy(idx).to(ctx.device)])
            for c in (0, 2):
                rows = want[c * 2000:(c + 1) * 2000].reshape(-1).cpu().numpy()
                assert g.enc.chunk_bytes(c) == O.encode_chunk(rows, (M, L)).tobytes(), (c, table is not None)
            gplan = g.plan(ctx)
            assert torch.equal(gplan.decode(g.enc), want.reshape(-1)), table is not None
            gplan.close()
            gplan = None
            del g
    finally:
        if gplan is not None:
            gplan.close()
        plan.close()


def test_more_than_2_32_encoded_words(ctx, O, gauss):
    """Uniform int16 noise under RiceParameter 8: nearly every code an escape of 25 bits, 0.78 words a sample; 400 chunks of
    2000 x 7000 (the fewest that hold 5.6e9 samples) make 4.38e9 words.  The default encode and decode; the spot chunks are
    chunk 0, the chunk that holds word 2^32, the one after it and the last.  11.2 GB of samples, 17.5 GB of words at the
    plan's capacity, 11.2 GB decoded, the oracle's copies on the host."""
    gauss.drop()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if free < 60 * GIB:
        pytest.skip("needs 60 GiB of free HBM")
    W, L = 2000, 7000
    N = W * L
    n = -(-5_600_000_000 // N)
    assert n == 400
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(2 ** 32 + 2)
    x = fill(torch.empty(n * N, dtype=torch.int16, device=dev),
             lambda m: torch.randint(-32768, 32768, (m,), device=dev, generator=g, dtype=torch.int16))
    plan = ctx.plan_uniform(n, N, (M, L))

    def spots(off):
        at = int(np.searchsorted(off, np.uint64(TWO32), side="right")) - 1  # off[at] <= 2^32 < off[at + 1]
        assert 0 < at and at + 1 < n - 1
        return [0, at, at + 1, n - 1]

    try:
        # (the plan's first encode expects k + 3.5 bits per sample and takes the persistent encoder; the lanes decoder behind
        # the chunk-wide walk by chains)
        enc = check_batch(ctx, O, x, plan, [N] * n, [L] * n, None, [(2, 0, D.ENC_STREAM)], [(8, 0, D.PATH_LANES)], spots=spots,
                          name="words-past-2^32")
        assert enc.total_words > TWO32
        assert 0.78 < enc.total_words / x.numel() < 0.79
    finally:
        plan.close()
