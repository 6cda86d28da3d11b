"""Where each encode_impl and debug flag sends a batch: drx_plan_last_encode_path / drx_plan_last_decode_path over a table
of small batches (route_encode() in drx_api_encode.hip, route_decode() in drx_decode_kernels.hip and, for the walk in front of the
decoder, route_walk() in drx_walk.hip), with the round trip of every case."""
import numpy as np
import pytest

from deltarice_amd import _lib as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# name: (chunk sample counts, WaveformLengths (0: the whole chunk), RiceParameter, taps or None, noise sigma)
BATCHES = {
    "stream-quiet": ([2100 * 7000] * 4, [7000] * 4, 8, None, 10),
    "stream-loud": ([2100 * 7000] * 4, [7000] * 4, 8, None, 400),
    "long-2": ([32 * 50000] * 2, [50000] * 2, 8, None, 10),
    "long-40": ([32 * 50000] * 40, [50000] * 40, 8, None, 10),
    "short": ([100 * 3000 + 37] * 3, [100] * 3, 8, None, 10),
    "whole-chunk": ([261001] * 4, [0] * 4, 8, None, 25),
    "ragged": ([512 * 40, 2048 * 9 + 17, 7000 * 30, 16384 * 4, 4321, 3333 * 21 + 1], [512, 2048, 7000, 16384, 0, 3333], 8, None, 10),
    "fir4": ([5000 * 100] * 3, [5000] * 3, 8, (1, -1, 1, -1), 20),
    "fir5": ([5000 * 3] * 3, [1000] * 3, 8, (1, -1, 1, -1, 1), 40),
    "wide-fused": ([200 * 7000] * 4, [7000] * 4, 64, None, 80),
    # as many long waveforms as the block decoder keeps resident: the inverse filter inside it (DRX_PATH_IIR_FUSED)
    "iir-fused": ([800 * 9001 - 9001 // 3] * 2, [9001] * 2, 8, (1, -1, 1, -1), 10),
}

# every flag alone, and the combinations the other tests use
FLAGS = (0, D.DBG_NO_LONG_PATHS, D.DBG_LONG_NOT_BLOCKS, D.DBG_NO_PARALLEL_WALKS, D.DBG_NO_PIECES, D.DBG_FORCE_SEGMENTS,
         D.DBG_FORCE_PIECES, D.DBG_NO_WIDE_FUSED, D.DBG_RAGGED_ONE_LANES_LAUNCH, D.DBG_FORCE_STREAM, D.DBG_IIR_SEPARATE,
         D.DBG_FORCE_STREAM_SEGS, D.DBG_WALK_BY_SCAN, D.DBG_WALK_BY_CHAINS,
         D.DBG_NO_LONG_PATHS | D.DBG_FORCE_STREAM, D.DBG_NO_LONG_PATHS | D.DBG_FORCE_STREAM_SEGS,
         D.DBG_NO_LONG_PATHS | D.DBG_NO_PIECES | D.DBG_FORCE_STREAM, D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_CHAINS,
         D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_SCAN)

# EXPECTED[batch][encode_impl]: "DRX_ENC_* / DRX_PATH_*" for every entry of FLAGS, in order
EXPECTED = {
    "stream-quiet": {
        0: "1/4 1/2 1/2 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/2 1/2 1/2 1/2 1/2",
        1: "3/4 3/2 3/2 3/4 3/4 2/4 4/4 3/4 3/4 3/4 3/4 3/4 3/4 3/4 3/2 3/2 3/2 3/2 3/2",
        2: "5/4 5/2 5/2 5/4 5/4 2/4 4/4 5/4 5/4 5/4 5/4 6/4 5/4 5/4 5/2 6/2 5/2 5/2 5/2",
    },
    "stream-loud": {
        0: "1/4 1/2 1/2 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/2 1/2 1/2 1/2 1/2",
        1: "3/4 3/2 3/2 3/4 3/4 2/4 4/4 3/4 3/4 3/4 3/4 3/4 3/4 3/4 3/2 3/2 3/2 3/2 3/2",
        2: "3/4 3/2 3/2 3/4 3/4 2/4 4/4 3/4 3/4 5/4 3/4 6/4 3/4 3/4 5/2 6/2 5/2 3/2 3/2",
    },
    "long-2": {
        0: "1/4 1/2 1/8 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/2 1/2 1/2 1/2 1/2",
        1: "4/4 4/2 4/8 4/4 2/4 2/4 4/4 4/4 4/4 4/4 4/4 4/4 4/4 4/4 4/2 4/2 3/2 4/2 4/2",
        2: "4/4 4/2 4/8 4/4 2/4 2/4 4/4 4/4 4/4 5/4 4/4 6/4 4/4 4/4 5/2 6/2 5/2 4/2 4/2",
    },
    "long-40": {
        0: "1/4 1/2 1/8 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/2 1/2 1/2 1/2 1/2",
        1: "4/4 4/2 4/8 4/4 2/4 2/4 4/4 4/4 4/4 4/4 4/4 4/4 4/4 4/4 4/2 4/2 3/2 4/2 4/2",
        2: "6/4 4/2 6/8 6/4 2/4 2/4 4/4 6/4 6/4 5/4 6/4 6/4 6/4 6/4 5/2 6/2 5/2 4/2 4/2",
    },
    "short": {
        0: "1/2 1/2 1/2 1/1 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2 1/2",
        1: "4/2 4/2 4/2 4/1 2/2 2/2 4/2 4/2 4/2 4/2 4/2 4/2 4/2 4/2 4/2 4/2 3/2 4/2 4/2",
        2: "4/2 4/2 4/2 4/1 2/2 2/2 4/2 4/2 4/2 5/2 4/2 6/2 4/2 4/2 5/2 6/2 5/2 4/2 4/2",
    },
    "whole-chunk": {
        0: "1/4 1/1 1/8 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/1 1/1 1/1 1/1 1/1",
        1: "4/4 4/1 4/8 4/4 2/4 2/4 4/4 4/4 4/4 4/4 4/4 4/4 4/4 4/4 4/1 4/1 3/1 4/1 4/1",
        2: "4/4 4/1 4/8 4/4 2/4 2/4 4/4 4/4 4/4 5/4 4/4 6/4 4/4 4/4 5/1 6/1 5/1 4/1 4/1",
    },
    "ragged": {
        0: "1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1 1/1",
        1: "4/1 4/1 4/1 4/1 2/1 2/1 4/1 4/1 4/1 4/1 4/1 4/1 4/1 4/1 4/1 4/1 3/1 4/1 4/1",
        2: "4/1 4/1 4/1 4/1 2/1 2/1 4/1 4/1 4/1 5/1 4/1 4/1 4/1 4/1 5/1 4/1 5/1 4/1 4/1",
    },
    "fir4": {
        0: "1/36 1/2 1/2 1/36 1/36 1/36 1/36 1/36 1/36 1/36 1/36 1/36 1/36 1/36 1/2 1/2 1/2 1/2 1/2",
        1: "3/36 3/2 3/2 3/36 3/36 3/36 4/36 3/36 3/36 3/36 3/36 3/36 3/36 3/36 3/2 3/2 3/2 3/2 3/2",
        2: "3/36 3/2 3/2 3/36 3/36 3/36 4/36 3/36 3/36 5/36 3/36 6/36 3/36 3/36 5/2 6/2 5/2 3/2 3/2",
    },
    "fir5": {
        0: "1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16",
        1: "1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16",
        2: "1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16 1/16",
    },
    "wide-fused": {
        0: "1/4 1/2 1/2 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/4 1/2 1/2 1/2 1/2 1/2",
        1: "3/4 3/2 3/2 3/4 3/4 2/4 4/4 4/4 3/4 3/4 3/4 3/4 3/4 3/4 3/2 3/2 3/2 3/2 3/2",
        2: "3/4 3/2 3/2 3/4 3/4 2/4 4/4 4/4 3/4 5/4 3/4 6/4 3/4 3/4 5/2 6/2 5/2 3/2 3/2",
    },
    "iir-fused": {
        0: "1/68 1/2 1/2 1/68 1/68 1/68 1/68 1/68 1/68 1/68 1/36 1/68 1/68 1/68 1/2 1/2 1/2 1/2 1/2",
        1: "3/68 3/2 3/2 3/68 3/68 3/68 4/68 3/68 3/68 3/68 3/36 3/68 3/68 3/68 3/2 3/2 3/2 3/2 3/2",
        2: "3/68 3/2 3/2 3/68 3/68 3/68 4/68 3/68 3/68 5/68 3/36 6/68 3/68 3/68 5/2 6/2 5/2 3/2 3/2",
    },
}


def make_plan(ctx, Ns, Ls, m, taps):
    if len(set(Ns)) == 1 and len(set(Ls)) == 1:
        opts = ((m, Ls[0]) if Ls[0] else (m,)) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())
        return ctx.plan_uniform(len(Ns), Ns[0], opts)
    return ctx.plan(Ns, Ls, m, taps)


def observe(ctx, name):
    """{encode_impl: "enc/dec ..." over FLAGS} of one batch; every case's round trip is checked on the way."""
    Ns, Ls, m, taps, sigma = BATCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
    xd = torch.from_numpy(x).to(ctx.device)
    plan = make_plan(ctx, Ns, Ls, m, taps)
    ref = None
    table = {}
    try:
        for eimpl in (0, 1, 2):
            ctx.set_option("encode_impl", eimpl)
            cells = []
            for flags in FLAGS:
                ctx.set_option("debug_flags", flags)
                plan.encode(xd)  # (twice: the second encode sees the code length the first one measured)
                enc = plan.encode(xd)
                e = plan.last_encode_path()
                words, off = enc.words[:enc.total_words], enc.chunk_word_off
                if ref is None:
                    ref = (words.clone(), off.clone())
                assert torch.equal(off, ref[1]) and torch.equal(words, ref[0]), (name, eimpl, flags)
                y = plan.decode(enc)
                assert torch.equal(y, xd), (name, eimpl, flags)
                cells.append(f"{e}/{plan.last_decode_path()}")
            table[eimpl] = " ".join(cells)
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("encode_impl", 2)
    return table


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(BATCHES))
def test_routes(ctx, name):
    got = observe(ctx, name)
    want = EXPECTED[name]
    for eimpl in (0, 1, 2):
        diff = [(flags, w, g) for flags, w, g in zip(FLAGS, want[eimpl].split(), got[eimpl].split()) if w != g]
        assert not diff, (name, eimpl, diff)
