"""GPU: every site of the decoupled look-back (deltarice_amd/csrc/drx_lookback.h) at a shape where the last walker has more than
two windows of predecessors -- more than 2 x kLookbackWin = 256 entries in front of it, so that the walk's step to the next
window and its `first` bound can both occur -- each result bit for bit against the oracle or the reference the neighbouring
tests of that route use, with the path or form of every call asserted.

On a GPU, whether a walk actually takes a second window depends on timing.  These shapes make it possible; the CPU program
(tests/lookback_rule_host.cpp, tests/test_lookback_rule_host.py) makes the rule certain.

The shapes follow from the constants of the headers (consts() reads them; the piece and block rules are mirrored below and in
tests/block_cells.py).  With the values the headers have today:
  k_encode_fused      3 chunks of 803 waveforms of 200 samples and one of 66: 2412 waveforms, 8 per workgroup: 302 workgroups, a
                      chunk's first waveform inside a workgroup; delta and taps (1, -1, 1, -1) (GEN).  No `wide` case: the wide
                      geometries take WaveformLengths above 3584 only (fused_wide(), drx_internal.h), not this size.
  pieces, packed      3 chunks of 10 504 waveforms of 504 samples: runs of 13, 8 runs per workgroup: 3 x 101 = 303 workgroups
  pieces, runs        3 chunks of 5655 waveforms of 1000 samples and one of 333: runs of 7, 8 per workgroup: 3 x 101 = 303 workgroups
  pieces, segments    2 chunks of 605 waveforms of 12 000 samples and one of 4000: 2 segments each, 4 waveforms per workgroup:
                      2 x 152 = 304 workgroups, 1212 waveforms
  pieces, SUPER       2 chunks of two waveforms of 180 000 and 140 000 samples, 3 parts each (a part's walk ends at its own
                      waveform's part 0: T - part); and one waveform of 19 648 455 samples = 300 parts (39 MB of int16)
  block forms         one chunk: a waveform of 5 400 000 samples (at RiceParameter 8 and sigma 4 it takes 4.6 bits per sample: 256
                      lanes x 9 words per block, 335 blocks, asserted to be at least 300 -- and so at least 300 of the smallest
                      block, 64 lanes x kBlkSegWMin words) and one of 100 000 samples (7 blocks, asserted fewer than 128)
                      directly behind it, whose walk must stop at its own block 0
  k_iir_tiles         one chunk: a waveform of 300 x 32 768 - 777 samples (300 tiles) and one of 40 000 (2 tiles), taps (1, -2, 1)
"""
import os
import re

import numpy as np
import pytest

import block_cells as bc
import filter_reference as fr
from deltarice_amd import _lib as D
from find_pulses_reference import START, find_pulses
from kernel_build import CSRC
from test_gpu_decode_windows import check as windows_check
from test_gpu_encoder_edges import reference
from test_gpu_routes import make_plan
from test_gpu_select import Stream
from test_gpu_transcode import Want, same_stream
from test_gpu_wave_stats_blocks import check as stats_check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BLOCKS = D.STATS_FORM_BLOCKS


def consts():
    """name -> value of the `constexpr` integer constants of the headers the shapes depend on"""
    out = {}
    for name in ("drx_internal.h", "drx_encode.h", "drx_blocks.h", "drx_lookback.h", "drx_encode_kernels.hip"):
        with open(os.path.join(CSRC, name)) as f:
            for line in f:
                m = re.match(r"\s*constexpr (?:uint32_t|uint64_t|int) (.*?);", line)
                if not m:
                    continue
                for item in m.group(1).split(","):
                    if "=" not in item:
                        continue
                    key, expr = (s.strip() for s in item.split("=", 1))
                    expr = re.sub(r"\b(\d+)(?:u|ull)\b", r"\1", expr)
                    if re.fullmatch(r"[\w\s*+\-()]+", expr) and re.fullmatch(r"k\w+", key):
                        try:
                            out[key] = int(eval(expr, {"__builtins__": {}}, dict(out)))
                        except NameError:
                            pass
    return out


K = consts()
WIN = K["kLookbackWin"]
ENOUGH = 300  # entries in front of the last walker: more than two windows
assert WIN == 128 and ENOUGH > 2 * WIN


# the piece rules of drx_internal.h, for RiceParameters up to 8 (k <= 3: the measured geometry)
def piece_run(L, packed):  # piece_shape(): waveforms of a run
    if packed:
        return max(1, min(K["kPcRunSamples"] // L, 2000 // (1 + (9 * L + 31) // 32)))
    return min(K["kPcRunSamples"] // L, K["kPcMaxRun"])


PC_MAX_LEN = K["kPcSegSamples"] * K["kPcWaves"]  # pc_max_len(k <= 3)


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


def noise(seed, n, sigma=10):
    return np.random.default_rng(seed).normal(0, sigma, n).astype(np.int16)


def encode_check(ctx, O, x, Ns, Ls, path, flags, m=8, taps=None):
    """One encode under encode_impl 1 and `flags`: words, chunk offsets and n_i the oracle's, the path as stated, the round trip."""
    ref_w, ref_off, ref_n = reference(O, x, Ns, Ls, m, taps)
    plan = make_plan(ctx, list(Ns), list(Ls), m, taps)
    xd = torch.from_numpy(x).to(ctx.device)
    try:
        ctx.set_option("encode_impl", 1)
        ctx.set_option("debug_flags", flags)
        enc = plan.encode(xd)
        assert plan.last_encode_path() == path, plan.last_encode_path()
        assert enc.total_words == ref_w.size
        assert torch.equal(enc.chunk_word_off.cpu(), torch.from_numpy(ref_off))
        assert torch.equal(enc.words[:enc.total_words].cpu(), torch.from_numpy(ref_w.view(np.int32)))
        assert np.array_equal(plan.wave_words(), ref_n)
        ctx.set_option("debug_flags", 0)
        assert torch.equal(plan.decode(enc), xd)
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("encode_impl", 2)
        plan.close()


# --------------------------------------------------------------------------- k_encode_fused
@pytest.mark.parametrize("taps", [None, (1, -1, 1, -1)], ids=["delta", "gen"])
def test_encode_fused(ctx, O, taps):
    WV, L = K["kEncWaves"], 200
    W = 100 * WV + 3  # full waveforms per chunk: not a multiple of WV, so the next chunk begins inside a workgroup
    Ns, Ls = [W * L + L // 3] * 3, [L] * 3
    waves = 3 * (W + 1)
    assert -(-waves // WV) >= ENOUGH and waves % WV and (W + 1) % WV
    encode_check(ctx, O, noise(1, sum(Ns), 20 if taps else 10), Ns, Ls, D.ENC_FUSED, D.DBG_NO_PIECES | D.DBG_NO_LONG_PATHS, taps=taps)


# --------------------------------------------------------------------------- k_encode_pieces
@pytest.mark.parametrize("L", [504, 1000], ids=["packed", "runs"])
def test_encode_pieces_runs(ctx, O, L):
    packed = L < 512 and L % 8 == 0
    run = piece_run(L, packed)
    assert run > 1 and L <= 3584
    W = (ENOUGH // 3 + 1) * K["kPcWaves"] * run  # waveforms per chunk: whole workgroups of whole runs
    # (a packed chunk's waveforms are all of one length; otherwise the chunk's last waveform is a shorter one)
    Ns, Ls = [W * L if packed else (W - 1) * L + L // 3] * 3, [L] * 3
    assert 3 * (W // (K["kPcWaves"] * run)) >= ENOUGH
    encode_check(ctx, O, noise(L, sum(Ns)), Ns, Ls, D.ENC_PIECES, D.DBG_FORCE_PIECES)


def test_encode_pieces_segments(ctx, O):
    L = 12000
    assert K["kPcWholeLen"] < L <= PC_MAX_LEN
    segs = 1
    while segs < -(-L // K["kPcSegSamples"]):
        segs *= 2
    per_wg = K["kPcWaves"] // segs
    W = (ENOUGH // 2 + 1) * per_wg + 1  # full waveforms per chunk, and a shorter one behind them
    Ns, Ls = [W * L + L // 3] * 2, [L] * 2
    assert 2 * (W + 1) >= ENOUGH and 2 * -(-(W + 1) // per_wg) >= ENOUGH
    encode_check(ctx, O, noise(L, sum(Ns)), Ns, Ls, D.ENC_PIECES, D.DBG_FORCE_PIECES)


def test_encode_pieces_super_two_waveforms_per_chunk(ctx, O):
    """The `T - part` bound: part p of a chunk's second waveform has the first waveform's parts right in front of its own."""
    L, last = 180000, 140000
    assert L > PC_MAX_LEN and -(-L // PC_MAX_LEN) >= 3
    Ns, Ls = [L + last] * 2, [L] * 2
    encode_check(ctx, O, noise(7, sum(Ns)), Ns, Ls, D.ENC_PIECES, D.DBG_FORCE_PIECES)


def test_encode_pieces_super_one_long_waveform(ctx, O):
    """One waveform of ENOUGH parts: the walk over the parts can leave its first window."""
    N = ENOUGH * PC_MAX_LEN - 12345
    assert -(-N // PC_MAX_LEN) == ENOUGH and 2 * N <= 64 << 20
    encode_check(ctx, O, noise(8, N), [N], [0], D.ENC_PIECES, D.DBG_FORCE_PIECES)


# --------------------------------------------------------------------------- the block forms
BLK_K, BLK_L, BLK_LAST = 3, 5400000, 100000


@pytest.fixture(scope="module")
def blk(ctx, O):
    """The stream of the block forms' batch, its samples, and the asserted block counts of its two waveforms."""
    rng = np.random.default_rng(11)
    x = bc.gauss(rng, bc.sigma_of(BLK_K, "matched"), BLK_L + BLK_LAST)
    # pulses far into both waveforms, where a block's first sample is known through the look-back alone
    for at in (BLK_L - 700000, BLK_L - 300000, BLK_L - 5000, BLK_L + BLK_LAST - 2000):
        x[at:at + 6] = 9000
    st = Stream(ctx, O, x, [BLK_L + BLK_LAST], [BLK_L], 1 << BLK_K)
    n_i = st.table.cpu().numpy().view(np.uint32)
    lanes = bc.nt_for_len(BLK_L, BLK_K)
    sw = bc.blk_segw_bits10(bc.blk_bits10(int(st.offs[-1]), x.size))
    blocks = [-(-int(n) // (lanes * sw)) for n in n_i]
    assert len(blocks) == 2 and blocks[0] >= ENOUGH and blocks[1] < WIN, (lanes, sw, blocks)
    assert -(-int(n_i[0]) // (64 * K["kBlkSegWMin"])) >= ENOUGH
    yield st, x
    st.plan.close()


def test_block_decode(ctx, blk):
    st, x = blk
    y = st.plan.decode(st.enc)
    assert st.plan.last_decode_path() == D.PATH_BLOCKS and st.plan.finish() == 0
    assert torch.equal(y, st.xd)


def test_block_wave_stats(ctx, blk):
    st, x = blk
    stats_check(ctx, st, x, (BLK_L,), BLOCKS, what="look-back", sidebands=(False,))


def test_block_find_pulses(ctx, blk):
    st, x = blk
    n, p = find_pulses(x, st.Ns, st.Ls, 5000, 1, 2, 8, None, (st.start, st.length, st.chunk))
    assert n.tolist() == [3, 1]
    gn, gp = st.plan.find_pulses(st.enc, 5000, 1, 2, 8)
    assert st.plan.last_decode_path() == D.PATH_PULSES and st.plan.finish() == 0
    assert st.plan.last_pulses_form() == D.PULSES_FORM_BLOCKS and st.plan.last_pulses_listed() == 0
    assert torch.equal(gn.cpu(), torch.from_numpy(n)) and torch.equal(gp.cpu(), torch.from_numpy(p))
    assert p[0, 2, START] == BLK_L - 5000 and p[1, 0, START] == BLK_LAST - 2000


def test_block_decode_windows(ctx, blk):
    st, x = blk
    starts = np.sort(np.random.default_rng(12).integers(-100, st.length[:, None] + 100, (2, 6)), axis=1)
    starts[:, -1] = st.length - 200  # a window over each waveform's last samples
    windows_check(ctx, st, x, [(starts, None, 0, 256, -1)], D.WINDOWS_FORM_BLOCKS, sidebands=(False,), what="look-back", listed=0)


def test_block_transcode(ctx, O, blk):
    st, x = blk
    want = Want(O, x, st.Ns, st.Ls, 16)
    t = st.plan.transcode(st.enc, rice_m=16)
    assert st.plan.last_decode_path() == D.PATH_TRANSCODE
    assert st.plan.last_transcode_form() == D.TRANSCODE_FORM_BLOCKS and st.plan.last_transcode_listed() == 0
    same_stream(t, want, "look-back")


# --------------------------------------------------------------------------- k_iir_tiles
def test_iir_tiles(ctx, O):
    import deltarice_amd as dr
    tile = K["kIirRun"] * K["kIirThreads"]
    L, last, taps, m = ENOUGH * tile - 777, tile + 7232, (1, -2, 1), 32
    assert -(-L // tile) == ENOUGH and -(-last // tile) == 2
    x = noise(13, L + last)
    opts = fr.opts_of(m, L, taps)
    words, off = O.encode_batch(x, L + last, opts)
    # the stream is the one tests/filter_reference.py states: its residuals' n_i are the stream's headers
    d = fr.chunk_residuals(x, L, taps)
    n_i = fr.chunk_wave_words(d, L, m.bit_length() - 1)
    assert int(words[1]) == n_i[0] and int(words[2 + n_i[0]]) == n_i[1] and words.size == 3 + sum(n_i)
    plan = ctx.plan_uniform(1, L + last, opts)
    try:
        enc = dr.EncodedBatch(torch.from_numpy(words.view(np.int32)).to(ctx.device), torch.from_numpy(off.astype(np.int64)).to(ctx.device), words.size)
        y = plan.decode(enc)
        path = plan.last_decode_path()
        assert path & D.PATH_BLOCKS and path & D.PATH_IIR and not path & D.PATH_IIR_FUSED and plan.finish() == 0, path
        y = y.cpu().numpy()
        assert np.array_equal(y, x), int(np.argmax(y != x))
        assert np.array_equal(fr.chunk_residuals(y, L, taps), d)
    finally:
        plan.close()
