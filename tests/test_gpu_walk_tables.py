"""The header walk's TABLES, walker by walker, at the smallest shapes at which each walker still does all of its work.

Per case and cell: after a decode, plan.wave_words() must be the oracle's own chain walk of the oracle's stream
(call_sequences.walk_chunk), the samples must be the input, and the same stream with one middle header raised by 1 must be
DRX_ERR_CORRUPT.  Cells: flags 0, WALK_BY_CHAINS, WALK_BY_SCAN, NO_PARALLEL_WALKS, each with NO_LONG_PATHS (the lane-per-waveform
decoder behind the walk, whatever the shape), under decode_impl 7 and 8.  Which walker a cell reaches follows from par_walks() /
route_walk() in drx_walk.hip and route_decode() in drx_decode_kernels.hip; the comments at CASES name it.  Under
NO_PARALLEL_WALKS every case takes the serial walkers: decode_impl 7 k_walk_block (WaveformLength <= kWalkShortLen) / k_walk_scalar
/ k_walk_list (ragged), decode_impl 8 the same walkers inside the lanes launch (walk_chunk_block / walk_chunks_scalar)."""
import os
import re

import numpy as np
import pytest

from call_sequences import walk_chunk
from deltarice_amd import _lib as D
from test_gpu_routes import make_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deltarice_amd", "csrc")
NLP = D.DBG_NO_LONG_PATHS
FLAGS = (NLP, NLP | D.DBG_WALK_BY_CHAINS, NLP | D.DBG_WALK_BY_SCAN, NLP | D.DBG_NO_PARALLEL_WALKS)
IMPLS = (7, 8)
THIRD = 2049 // 3

# name: (chunk sample counts, WaveformLengths, RiceParameter, data)
CASES = {
    # chunk-wide (8 <= 64 <= 8192 waveforms longer than kWalkShortLen).  Three chunks of 64 waveforms: the scan form by default and
    # under WALK_BY_SCAN (k_pw_scan + k_walk_parallel; 64 is its minimum), k_walk_sparse with 64 / 8 = 8 chains under WALK_BY_CHAINS
    "scan-64": ([64 * 2049 - THIRD] * 3, [2049] * 3, 8, "gauss"),
    # chunk-wide at kSwMinWaves: fewer than 64 waveforms is outside the scan form's range, so k_walk_sparse under every flag,
    # S = 8 / 8 = one chain per chunk
    "chains-8": ([8 * 2049] * 5, [2049] * 5, 8, "gauss"),
    # block-parallel (1 chunk <= 300 / 35): max_words 50 -> B = 1024; min_words 8 < 32 -> no header lists, the second chase
    # emits; about three blocks
    "blocks-1024-chase": ([300 * 64], [64], 8, "gauss"),
    # block-parallel (2 chunks <= 70 / 35): max_words 400 -> B = 1024; min_words 64 -> header lists and k_bw_emit
    "blocks-1024-lists": ([70 * 512] * 2, [512] * 2, 8, "gauss"),
    # block-parallel (1 <= 40 / 35): max_words 1600 -> B = 2048, with lists
    "blocks-2048-lists": ([40 * 2048], [2048], 8, "gauss"),
    # ragged, rag_par: the long-waveform chunk to the chunk-wide walk over its list (scan form; k_walk_sparse under
    # WALK_BY_CHAINS), the two short-waveform chunks to the block-parallel walk over theirs, B = 2048 (kWalkShortLen's
    # max_words), no lists (rag_bw_min_len = 64)
    "ragged-both": ([300 * 64, 70 * 7000, 80 * 2048], [64, 7000, 2048], 8, "gauss"),
    # block-parallel: more than kSwMaxWaves waveforms, so not chunk-wide; max_words 2110 -> B = 4096, with lists
    "blocks-4096": ([8200 * 2700], [2700], 8, "spikes"),
    # impostor headers (impostor_chunk()).  dense: some block meets more than kBwTries in front of its first header, the chunk is
    # flagged and k_walk_block_only judges it; sparse: every block's chase succeeds after zero to five retries.
    # m = 1: the first pass without lists, m = 8: with lists
    "impostors-dense-m1": ([70 * 512], [512], 1, "dense"),
    "impostors-dense-m8": ([70 * 512], [512], 8, "dense"),
    "impostors-sparse-m1": ([70 * 512], [512], 1, "sparse"),
    "impostors-sparse-m8": ([70 * 512], [512], 8, "sparse"),
}
DENSE_AT = tuple(range(6, 512, 32))
SPARSE_AT = (6, 102, 198, 294, 390)


def impostor_chunk(W, L, m, at):
    """One chunk whose payload holds words that look like headers.  Every residual's zigzag value is 8 << k, an escape of 25
    bits; the residuals at the indices `at` of every waveform have zigzag value 0x8000: the 23 zero bits behind that code's
    leading one, the next escape's marker and eight bits fill one payload word of value 0x100, inside [1, max_words]."""
    k = m.bit_length() - 1
    r = np.full((W, L), (8 << k) // 2, np.int64)
    r[:, list(at)] = 0x8000 // 2
    return (np.cumsum(r, axis=1) & 0xFFFF).astype(np.uint16).view(np.int16).reshape(-1)


def make_data(kind, Ns, Ls, m, seed):
    if kind == "gauss":
        return np.random.default_rng(seed).normal(0, 10, sum(Ns)).astype(np.int16)
    if kind == "spikes":  # zeros, one spike per waveform
        x = np.zeros(sum(Ns), np.int16)
        w = np.arange(Ns[0] // Ls[0])
        x[w * Ls[0] + (w * 37) % Ls[0]] = 1 + w % 100
        return x
    return impostor_chunk(Ns[0] // Ls[0], Ls[0], m, DENSE_AT if kind == "dense" else SPARSE_AT)


def bw_tries():
    m = re.search(r"\bkBwTries\s*=\s*(\d+)", open(os.path.join(CSRC, "drx_walk.hip")).read())
    assert m, "drx_walk.hip: no `kBwTries = ...` any more; the impostor cases are chosen by it"
    return int(m.group(1))


def impostors_in_front(w, n_i, L, B=1024):
    """Per B-word block of one chunk (counted from the chunk's start) that holds a true header: the words in [1, max_words] in
    front of the block's first true header (word 0, the sample count, is no candidate: block 0 starts at word 1)."""
    max_words = (L * 25 + 31) >> 5
    pos = 1 + np.concatenate([[0], np.cumsum(n_i.astype(np.int64) + 1)[:-1]])
    header = np.zeros(w.size, bool)
    header[pos] = True
    small = (w >= 1) & (w <= max_words) & ~header
    small[0] = False
    out = []
    for b0 in range(0, w.size, B):
        h = np.flatnonzero(header[b0:b0 + B])
        if h.size:
            out.append(int(small[b0:b0 + h[0]].sum()))
    return out


class Case:
    def __init__(self, name):
        from oracle import oracle as O
        self.Ns, self.Ls, self.m, self.kind = CASES[name]
        self.x = make_data(self.kind, self.Ns, self.Ls, self.m, sum(map(ord, name)))
        words, offs, n_i, at = [], [0], [], 0
        for N, L in zip(self.Ns, self.Ls):
            w = O.encode_chunk(self.x[at:at + N], (self.m, L))
            t = walk_chunk(w, N, L)
            assert t is not None
            words.append(w), offs.append(offs[-1] + w.size), n_i.append(t)
            at += N
        self.chunks, self.n_i = words, np.concatenate(n_i)
        self.words, self.offs = np.concatenate(words), np.array(offs, np.int64)
        # one middle header raised by 1
        c = len(self.Ns) // 2
        t = n_i[c]
        self.bad = self.words.copy()
        self.bad[offs[c] + 1 + int((t[:t.size // 2].astype(np.int64) + 1).sum())] += 1


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_walk_tables(ctx, name):
    import deltarice_amd as dr
    case = Case(name)
    if case.kind in ("dense", "sparse"):
        # the condition the two recipes are a means to, from the oracle's stream and table
        tries, L = bw_tries(), case.Ls[0]
        assert set(case.n_i.tolist()) == {(L * 25 + 31) >> 5}
        front = impostors_in_front(case.chunks[0], case.n_i, L)
        if case.kind == "dense":
            assert max(front) > tries, front
        else:
            assert max(front) <= tries - 1 and max(front) >= 1, front
    dev = lambda a: torch.from_numpy(a).to(ctx.device)  # noqa: E731
    xd, off = dev(case.x), dev(case.offs)
    good = dr.EncodedBatch(dev(case.words.view(np.int32)), off, case.words.size)
    bad = dr.EncodedBatch(dev(case.bad.view(np.int32)), off, case.bad.size)
    plan = make_plan(ctx, case.Ns, case.Ls, case.m, None)
    try:
        for impl in IMPLS:
            ctx.set_option("decode_impl", impl)
            for flags in FLAGS:
                cell = (name, impl, flags)
                ctx.set_option("debug_flags", flags)
                y = plan.decode(good)
                assert np.array_equal(plan.wave_words(), case.n_i), cell
                assert torch.equal(y, xd), cell
                with pytest.raises(dr.DeltaRiceError) as e:
                    plan.decode(bad)
                assert e.value.status == 4, cell
    finally:
        ctx.set_option("decode_impl", 8)
        ctx.set_option("debug_flags", 0)
        plan.close()
