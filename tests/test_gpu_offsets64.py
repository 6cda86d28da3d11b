"""Every decode, walk, select and gather route on streams that lie at word offsets around 2^30, 2^31 and 2^32 of their buffer
(byte offsets around 2^32, 2^33 and 2^34): chunk_word_off[0] is an input, so a small batch's stream -- the ORACLE's, valid
throughout -- is copied to base B of one 17.2 GB buffer that is never filled, chunk_word_off = B + the oracle's offsets and
in_words = B + total (the last pieces take the guarded loads).  1024 words of 0xFFFFFFFF lie on each side of the stream and
every output in a window between sentinels (test_gpu_lanes_lines.py::window), both checked afterwards.

Bases, h = half the stream's words made odd: 2^30 - h (the byte offset straddles 2^32), 2^31 - h, 2^32 - h, 2^32 + 5.

Per batch and base: decode in every cell of CELLS (decode_impl, debug flags -> last_decode_path(), as route_decode() in
drx_decode_kernels.hip and route_walk() in drx_walk.hip say for these geometries; the comments name the walk, which the
path bits do not show), decode_with_wave_words with the oracle's n_i table, decode_select of the first, a middle and the last
waveform (a leftover one where the batch has one) with and without the side-band, gather_encoded of the same entries in
both forms of its copy.  Everything against the samples the oracle was given and its bytes.  The batches are those of
test_gpu_routes.py, shrunk to what their route still takes (about 4e5 words; the inverse filter inside the block decoder
needs 1536 waveforms of 2048 samples: 8.3e5).  The encoders write from word 0 of their output: their rows are here as the
round trip of every batch (ENCODE: every encoder on "stream"), the oracle's stream word for word."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_lanes_lines import S16, window
from test_gpu_routes import BATCHES, make_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BIG_WORDS = 2 ** 32 + 2 ** 20
PAD = 1024
FIR4 = (1, -1, 1, -1)
NLP, NOPAR = D.DBG_NO_LONG_PATHS, D.DBG_NO_PARALLEL_WALKS

# name: (chunk sample counts, WaveformLengths (0: the whole chunk), RiceParameter, taps or None, noise sigma)
SMALL = {
    "stream": ([64 * 7000] * 4, [7000] * 4, 8, None, 10),      # "stream-quiet" at the fewest waveforms the scan walk takes
    "short": BATCHES["short"],
    "runs-512": ([512 * 300] * 3, [512] * 3, 8, None, 10),     # 32 words a waveform at least: the block-parallel walk keeps header lists
    "long": ([16 * 50000] * 2, [50000] * 2, 8, None, 10),      # "long-2", half of it
    "iir": ([768 * 2048] * 2, [2048] * 2, 8, FIR4, 10),        # 1536 waveforms: as many as the block decoder keeps resident at 128 lanes
    "fir5": BATCHES["fir5"],
    "ragged": BATCHES["ragged"],
    "whole-chunk": BATCHES["whole-chunk"],
}

# (decode_impl, debug flags, DRX_PATH_* expected)
CELLS = {
    "stream": [(8, 0, D.PATH_BLOCKS),                              # chunk-wide walk by scan (four chunks), k_decode_blocks
               (8, NLP, D.PATH_LANES),                             # chunk-wide walk by scan, lanes behind its walk
               (8, NLP | D.DBG_WALK_BY_CHAINS, D.PATH_LANES),      # chunk-wide walk by chains
               (8, NLP | NOPAR, D.PATH_LANES_FUSED),               # scalar-load walkers inside the lanes launch
               (7, NLP | NOPAR, D.PATH_LANES)],                    # serial walk by scalar chains
    "short": [(8, 0, D.PATH_LANES),                                # block-parallel walk, second chase
              (8, NOPAR, D.PATH_LANES_FUSED),                      # LDS block walkers inside the lanes launch
              (7, NOPAR, D.PATH_LANES)],                           # serial walk through LDS (k_walk_block)
    "runs-512": [(8, 0, D.PATH_LANES),                             # block-parallel walk with header lists (k_bw_emit)
                 (8, NOPAR, D.PATH_LANES_FUSED)],
    "long": [(8, 0, D.PATH_BLOCKS), (8, D.DBG_LONG_NOT_BLOCKS, D.PATH_LONG), (8, NLP, D.PATH_LANES)],
    "iir": [(8, 0, D.PATH_BLOCKS | D.PATH_IIR_FUSED), (8, D.DBG_IIR_SEPARATE, D.PATH_BLOCKS | D.PATH_IIR),
            (8, NLP, D.PATH_LANES)],                               # block-parallel walk, k_decode_lanes<GEN>
    "fir5": [(8, 0, D.PATH_SIMPLE)],
    "ragged": [(8, 0, D.PATH_LANES_FUSED),                         # a ragged plan too small for the parallel walks
               (7, 0, D.PATH_LANES)],                              # k_walk_block + k_walk_list, lanes in longest-first order
    "whole-chunk": [(8, 0, D.PATH_BLOCKS), (8, D.DBG_LONG_NOT_BLOCKS, D.PATH_LONG), (8, NLP, D.PATH_LANES_FUSED)],
}
# behind the side-band's tables no walk runs and nothing is fused into the lanes launch
SIDE_PATH = {"stream": D.PATH_BLOCKS, "short": D.PATH_LANES, "runs-512": D.PATH_LANES, "long": D.PATH_BLOCKS,
             "iir": D.PATH_BLOCKS | D.PATH_IIR_FUSED, "fir5": D.PATH_SIMPLE, "ragged": D.PATH_LANES, "whole-chunk": D.PATH_BLOCKS}
# (encode_impl, debug flags, DRX_ENC_* expected): route_encode() in drx_api_encode.hip
ENCODE = {
    "stream": [(2, 0, D.ENC_FUSED), (2, D.DBG_FORCE_STREAM, D.ENC_STREAM), (2, D.DBG_FORCE_STREAM_SEGS, D.ENC_STREAM_SEGS),
               (2, D.DBG_FORCE_PIECES, D.ENC_PIECES), (2, D.DBG_FORCE_SEGMENTS, D.ENC_SEGMENTS), (0, 0, D.ENC_TWO_PASS)],
    "short": [(2, 0, D.ENC_PIECES)], "runs-512": [(2, 0, D.ENC_PIECES)], "long": [(2, 0, D.ENC_PIECES)], "iir": [(2, 0, D.ENC_PIECES)],
    "fir5": [(2, 0, D.ENC_TWO_PASS)], "ragged": [(2, 0, D.ENC_PIECES)], "whole-chunk": [(2, 0, D.ENC_PIECES)],
}


def opts_of(L, m, taps):
    return ((m, L) if L else (m,)) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())


class Small:
    """One batch: its samples, the oracle's stream and n_i table, every waveform's place, a plan."""

    def __init__(self, ctx, name):
        from oracle import oracle as O
        self.name = name
        self.Ns, self.Ls, self.m, self.taps, sigma = SMALL[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        self.x = rng.normal(0, sigma, sum(self.Ns)).astype(np.int16)
        words, offs, n_i, rows, at = [], [0], [], [], 0
        for N, L in zip(self.Ns, self.Ls):
            w = O.encode_chunk(self.x[at:at + N], opts_of(L, self.m, self.taps))
            assert int(w[0]) == N
            p = 1
            for s in range(0, N, L or N):
                rows.append((at + s, min(L or N, N - s)))
                n_i.append(int(w[p]))
                p += 1 + int(w[p])
            assert p == w.size
            words.append(w)
            offs.append(offs[-1] + w.size)
            at += N
        self.words, self.offs, self.total = np.concatenate(words), np.array(offs, dtype=np.int64), int(offs[-1])
        self.n_i, self.rows = np.array(n_i, dtype=np.uint32), rows
        self.xd = torch.from_numpy(self.x).to(ctx.device)
        self.side = torch.from_numpy(self.n_i.view(np.int32)).to(ctx.device)
        self.plan = make_plan(ctx, self.Ns, self.Ls, self.m, self.taps)
        assert self.plan.total_waves == len(rows)

    def bases(self):
        h = (self.total // 2) | 1
        return [2 ** 30 - h, 2 ** 31 - h, 2 ** 32 - h, 2 ** 32 + 5]


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big(ctx):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if free < 20 * 2 ** 30:
        pytest.skip("needs 20 GiB of free HBM")
    t = torch.empty(BIG_WORDS, dtype=torch.int32, device=ctx.device)  # (never filled)
    yield t
    del t
    torch.cuda.empty_cache()


def sentinels_intact(base, lo, n):
    return bool((base[:lo] == S16).all().item()) and bool((base[lo + n:] == S16).all().item())


def at_base(ctx, O, big, case, B):
    from deltarice_amd.codec import EncodedBatch
    plan, name, total = case.plan, case.name, case.total
    assert B - PAD >= 0 and B + total + PAD <= BIG_WORDS
    big[B - PAD:B + total + PAD].fill_(-1)
    big[B:B + total].copy_(torch.from_numpy(case.words.view(np.int32)))
    off = torch.from_numpy(case.offs + B).to(ctx.device)
    enc = EncodedBatch(big, off, B + total)
    n = plan.total_samples
    try:
        # 1. decode, every cell
        for impl, flags, want in CELLS[name]:
            cell = (name, B, impl, flags)
            ctx.set_option("decode_impl", impl)
            ctx.set_option("debug_flags", flags)
            ybase, yw, lo = window(ctx.device, n, torch.int16, 0, S16)
            plan.decode(enc, out=yw)
            assert plan.last_decode_path() == want, (cell, plan.last_decode_path())
            assert torch.equal(yw, case.xd), cell
            assert sentinels_intact(ybase, lo, n), cell
        ctx.set_option("decode_impl", 8)
        ctx.set_option("debug_flags", 0)
        # 2. the oracle's n_i table as the side-band
        ybase, yw, lo = window(ctx.device, n, torch.int16, 0, S16)
        ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
        plan.decode_with_wave_words(big, off, case.side, out=yw, in_words=B + total)
        plan.finish()
        assert plan.last_decode_path() == SIDE_PATH[name], (name, B, plan.last_decode_path())
        assert torch.equal(yw, case.xd) and sentinels_intact(ybase, lo, n), (name, B, "side-band")
        # 3. selected waveforms: the first, a middle one, the last
        W = plan.total_waves
        idx = [0, W // 2, W - 1]
        stride = plan.longest_wave()
        for table in (None, case.side):
            cell = (name, B, "select", table is not None)
            obase, ow, lo = window(ctx.device, len(idx) * stride, torch.int16, 0, S16)
            rows = plan.decode_select(enc, idx, out=ow.view(len(idx), stride), wave_words=table)
            assert plan.last_decode_path() == D.PATH_SELECT, cell
            for r, g in enumerate(idx):
                s0, ln = case.rows[g]
                assert torch.equal(rows[r, :ln], case.xd[s0:s0 + ln]), (cell, g)
                assert bool((rows[r, ln:] == S16).all().item()), (cell, g)
            assert sentinels_intact(obase, lo, len(idx) * stride), cell
        # 4. the same entries gathered, one to an output chunk (any lengths), both forms of the copy
        for table in (None, case.side):
            for flags in (0, D.DBG_GATHER_OTHER_COPY):
                cell = (name, B, "gather", table is not None, flags)
                ctx.set_option("debug_flags", flags)
                g = plan.gather_encoded(enc, idx, 1, wave_words=table)
                assert plan.last_decode_path() == D.PATH_GATHER, cell
                assert g.wave_words.cpu().numpy().view(np.uint32).tolist() == [int(case.n_i[i]) for i in idx], cell
                for c, i in enumerate(idx):
                    s0, ln = case.rows[i]
                    assert int(g.chunk_samples[c]) == ln == int(g.wave_lens[c]), cell
                    assert g.enc.chunk_bytes(c) == O.encode_chunk(case.x[s0:s0 + ln], opts_of(ln, case.m, case.taps)).tobytes(), (cell, i)
        ctx.set_option("debug_flags", 0)
        torch.cuda.synchronize()
        assert bool((big[B - PAD:B] == -1).all().item()) and bool((big[B + total:B + total + PAD] == -1).all().item()), (name, B)
        assert np.array_equal(big[B:B + total].cpu().numpy().view(np.uint32), case.words), (name, B)
    finally:
        ctx.set_option("decode_impl", 8)
        ctx.set_option("debug_flags", 0)


@pytest.mark.parametrize("name", list(SMALL))
def test_streams_at_large_word_offsets(ctx, big, name):
    from oracle import oracle as O
    case = Small(ctx, name)
    try:
        assert case.total + 2 * PAD + 5 <= 2 ** 20, case.total  # (the buffer's room behind word 2^32)
        # the encoders' rows: the oracle's stream word for word
        for eimpl, flags, want in ENCODE[name]:
            ctx.set_option("encode_impl", eimpl)
            ctx.set_option("debug_flags", flags)
            enc = case.plan.encode(case.xd)
            assert case.plan.last_encode_path() == want, (name, eimpl, flags, case.plan.last_encode_path())
            assert enc.total_words == case.total and np.array_equal(enc.chunk_word_off.cpu().numpy(), case.offs), (name, eimpl, flags)
            assert np.array_equal(enc.words[:case.total].cpu().numpy().view(np.uint32), case.words), (name, eimpl, flags)
            assert np.array_equal(case.plan.wave_words(), case.n_i), (name, eimpl, flags)
        ctx.set_option("encode_impl", 2)
        ctx.set_option("debug_flags", 0)
        for B in case.bases():
            at_base(ctx, O, big, case, B)
    finally:
        ctx.set_option("encode_impl", 2)
        ctx.set_option("debug_flags", 0)
        case.plan.close()
