"""CPU: the shapes of tests/test_gpu_selection_data.py, and the proof -- with the oracle and the launchers' own arithmetic,
no GPU -- that each one reaches the path it is named for.

drx_decode_select and drx_gather_encoded take other paths at exact sizes: payloads of whole 16-word segments and 1024-word
blocks (k_decode_select), copies of exactly kGcPiece words, of fewer than four, of more than `slots` pieces (k_gather_waves),
lists longer than a launch's grid (kSelMaxGrid, the scan's 1024 blocks, the copy's 2^22 wavefronts).  The shapes below are
chosen by those constants, so the constants are READ OUT OF THE SOURCES here: a retune of kSelSeg, kGcPiece, kGsBlock or
kSelMaxGrid fails this file instead of silently moving the GPU tests off their boundaries."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deltarice_amd", "csrc")


# --------------------------------------------------------------------------- the sources' constants
def source(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


# the named constants the shapes are chosen by, per source file, each after the ones its expression uses
NAMED = {
    "drx_select.hip": ("kSelSeg", "kSelSegBits", "kSelBlockWords", "kSelMaxGrid"),
    "drx_gather.hip": ("kGsThreads", "kGsPer", "kGsBlock", "kGcPiece"),
    "drx_api_select.hip": ("kGatherWavesFromWords",),
    "drx_walk.hip": ("kSwSegs", "kSwCap"),
    "drx_walk.h": ("kWalkShortLen",),
}


def constant(txt, fname, name, known):
    """`name = <integer expression of literals and the constants read before it>` of one source file."""
    m = re.search(r"\b%s\s*=\s*([^,;{}]+)[,;]" % name, txt)
    assert m, f"{fname}: no `{name} = ...` any more; the shapes of the selection tests are chosen by it"
    expr = re.sub(r"\b(\d+)(?:ull|ul|u)\b", r"\1", m.group(1), flags=re.I)
    try:
        value = eval(expr, {"__builtins__": {}}, dict(known))  # noqa: S307 (the project's own sources)
    except Exception as e:  # noqa: BLE001
        raise AssertionError(f"{fname}: `{name} = {m.group(1).strip()}` is no integer expression of {sorted(known)}: {e!r}")
    assert isinstance(value, int), f"{fname}: {name} = {value!r}"
    return value


def launch_constants():
    """What the shapes depend on.  Every miss is an assertion that names the file and the constant or the line looked for."""
    K = {}
    for fname, names in NAMED.items():
        txt, known = source(fname), {}
        for n in names:
            known[n] = constant(txt, fname, n, known)
        K.update(known)
    g = source("drx_gather.hip")
    m = re.search(r"__launch_bounds__\((\d+)\)\s*void\s+k_gather_scan\b", g)  # blocks per round of its outer loop
    assert m and re.search(r"b0\s*\+=\s*%s\b" % m.group(1), g), "drx_gather.hip: k_gather_scan's workgroup size and the stride of its outer loop"
    K["scan_round"] = int(m.group(1))
    m = re.search(r"k_gather_waves<<<\(unsigned\)std::min<uint64_t>\(wgs,\s*1u\s*<<\s*(\d+)\),\s*(\d+),", g)  # grid cap, threads
    assert m and re.search(r"wgs\s*=\s*\(n_sel \* slots \+ 3\)\s*/\s*4;", g), "drx_gather.hip: k_gather_waves' grid"
    K["waves_max_wavefronts"] = (1 << int(m.group(1))) * (int(m.group(2)) // 64)
    m = re.search(r"slots\s*=\s*\(mean_words \+ kGcPiece - 1\)\s*/\s*kGcPiece;\s*slots\s*=\s*std::max<uint64_t>\(1,\s*std::min<uint64_t>\(slots,\s*(\d+)\)\);", g)
    assert m, "drx_gather.hip: how launch_gather() gets `slots` from mean_words"
    K["slots_max"] = int(m.group(1))
    api = source("drx_api_select.hip")
    assert re.search(r"mean_words\s*=\s*in_words\s*/\s*G\.total_waves;", api), "drx_api_select.hip: mean_words"
    assert re.search(r"tiles\s*=\s*\(mean_words < kGatherWavesFromWords\)\s*!=", api), "drx_api_select.hip: the choice of the copy form"
    w = source("drx_walk.hip")  # k_walk_sparse: the number of chains, their cuts, what flags a chunk
    assert re.search(r"uint32_t S = W / 8u;\s*S = S > kSwSegs \? kSwSegs : \(S < 1u \? 1u : S\);\s*if \(len_w / W > 8192u\) S = 1u;", w), "drx_walk.hip: chains per chunk"
    assert re.search(r"from = 1u \+ \(uint32_t\)\(\(\(uint64_t\)\(len_w - 1u\) \* sg\) / S\);", w), "drx_walk.hip: a chain's cut"
    assert re.search(r"if \(n < lo_any \|\| n > hi_any \|\| cnt >= kSwCap\) \{ bad = true; break; \}", w), "drx_walk.hip: a chain's capacity"
    assert re.search(r"return chunk_wide_walk_takes\(n_waves, wave_len\) \? 0 : 2;", w) and \
        re.search(r"return wave_len > kWalkShortLen && n_waves >= kSwMinWaves && n_waves <= kSwMaxWaves;", w), "drx_walk.hip: select_walk_class()"
    m = re.search(r"kSwMinWaves = (\d+), kSwMaxWaves = (\d+);", w)
    assert m, "drx_walk.hip: kSwMinWaves, kSwMaxWaves"
    K["kSwMinWaves"], K["kSwMaxWaves"] = int(m.group(1)), int(m.group(2))
    return K


def chain_headers(K, n_i, n_waves):
    """k_walk_sparse's chains over one chunk, replayed on its true header chain (n_i of its waveforms): headers each chain
    meets between its start -- the first header at or behind its cut -- and the next chain's.  A chain that meets more than
    kSwCap of them stops there, and the chunk goes to the scalar walker.  (Chain 0 starts at the chunk's first header, a true
    one, so its count up to the next CUT holds whatever word the kernel takes for the next start.)"""
    pos = 1 + np.cumsum(n_i.astype(np.int64) + 1) - (n_i.astype(np.int64) + 1)  # every header, in words of the chunk
    len_w = int(pos[-1] + n_i[-1] + 1)
    S = max(1, min(K["kSwSegs"], n_waves // 8))
    if len_w // n_waves > 8192:
        S = 1
    cuts = [1 + (len_w - 1) * sg // S for sg in range(S)]
    first = np.searchsorted(pos, cuts)  # the first header at or behind each cut
    return np.diff(np.append(first, n_waves)), int(np.searchsorted(pos, cuts[1])) if S > 1 else n_waves


def slots_of(K, in_words, total_waves):
    """launch_gather's pieces side by side, from the in_words the caller states."""
    mean = in_words // total_waves
    return max(1, min(-(-mean // K["kGcPiece"]), K["slots_max"])), mean


# --------------------------------------------------------------------------- generators
def all_escape(rng, n_waves, L):
    """Per waveform the running sum mod 2^16 of deltas with 64 <= |d| <= 32767: at m = 8 every code is an escape, 25 bits of
    random content, so n_i = ceil(25 L / 32) whatever the draw."""
    d = rng.integers(64, 32768, (n_waves, L)) * rng.choice([-1, 1], (n_waves, L))
    return (np.cumsum(d, axis=1) & 0xFFFF).astype(np.uint16).view(np.int16).reshape(-1)


# (b) exact payload sizes.  L -> n_i; five waveforms of each length, one chunk per length, one ragged plan, m = 8
EXACT_M, EXACT_WAVES = 8, 5
ESCAPE_LEN = {1: 1, 2: 2, 20: 16, 21: 17, 40: 32, 1309: 1023, 1310: 1024, 1311: 1025, 2618: 2046, 2620: 2047, 2621: 2048,
              5241: 4095, 5242: 4096, 5243: 4097}
# zeros at k = 3: four bits a sample and no code that differs from its neighbours, so a parse started anywhere but on a code
# boundary never falls into step
CONSTANT_LEN = {8184: 1023, 8192: 1024, 8200: 1025, 16376: 2047, 16384: 2048}


def exact_batch():
    """-> x, Ns, Ls, the n_i each waveform must have."""
    rng = np.random.default_rng(20)
    xs, Ns, Ls, want = [], [], [], []
    for L, n in ESCAPE_LEN.items():
        xs.append(all_escape(rng, EXACT_WAVES, L))
        Ns.append(EXACT_WAVES * L), Ls.append(L), want.extend([n] * EXACT_WAVES)
    for L, n in CONSTANT_LEN.items():
        xs.append(np.zeros(EXACT_WAVES * L, np.int16))
        Ns.append(EXACT_WAVES * L), Ls.append(L), want.extend([n] * EXACT_WAVES)
    return np.concatenate(xs), Ns, Ls, np.array(want, np.uint32)


# (c) code lengths that differ inside a chunk
LEVELS = dict(L=7000, W=16, n_chunks=3, m=8)


def levels_batch():
    """Waveforms alternately silent and full-range uniform: the batch's mean code length is half a loud waveform's."""
    g = LEVELS
    rng = np.random.default_rng(21)
    x = rng.integers(-32768, 32768, (g["n_chunks"] * g["W"], g["L"])).astype(np.int16)
    x[0::2] = 0
    return x.reshape(-1), [g["W"] * g["L"]] * g["n_chunks"], [g["L"]] * g["n_chunks"]


SILENT_LOUD = dict(L=7000, W=512, n_chunks=3, m=1)


def silent_loud_batch():
    """The "mixed" data of test_chunk_wide_walk_by_chains: the first three quarters of every chunk silent (one bit per sample
    at k = 0), the rest loud; a shorter last waveform.  (k_walk_sparse's chains are unequal there, 56 headers at most: it
    still walks such a chunk itself -- CHAIN_OVERFLOW is the shape it gives up on.)"""
    g = SILENT_LOUD
    N = g["W"] * g["L"] - g["L"] // 3
    rng = np.random.default_rng(22)
    x = rng.normal(0, 2000, g["n_chunks"] * N).astype(np.int16)
    for c in range(g["n_chunks"]):
        x[c * N:c * N + (3 * N) // 4] = 0
    return x, [N] * g["n_chunks"], [g["L"]] * g["n_chunks"]


# 400 silent waveforms of 66 words each in front of 560 loud ones of ~1600: a sixty-fourth of the chunk's words, one chain, lies
# wholly in the silent part and holds more than kSwCap headers
CHAIN_OVERFLOW = dict(L=2049, W=960, quiet=400, n_chunks=3, m=1)


def chain_overflow_batch():
    g = CHAIN_OVERFLOW
    N = g["W"] * g["L"] - g["L"] // 3
    rng = np.random.default_rng(26)
    x = rng.normal(0, 2000, g["n_chunks"] * N).astype(np.int16)
    for c in range(g["n_chunks"]):
        x[c * N:c * N + g["quiet"] * g["L"]] = 0
    return x, [N] * g["n_chunks"], [g["L"]] * g["n_chunks"]


# (e) lists beyond the launch caps
CAPS = dict(L=24, W=5000, n_chunks=2, m=8, n_select=(1 << 20) + 77, n_gather=(1 << 22) + 4099, cw=65536)


def caps_batch():
    g = CAPS
    x = np.random.default_rng(23).normal(0, 10, g["n_chunks"] * g["W"] * g["L"]).astype(np.int16)
    return x, [g["W"] * g["L"]] * g["n_chunks"], [g["L"]] * g["n_chunks"]


CAPACITY_FACTOR = 64  # (f) in_words = a buffer 64 times the stream


# --------------------------------------------------------------------------- the checks
@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def K():
    return launch_constants()


def chain(O, x, Ns, Ls, m):
    """n_i of every waveform from the header chains of the oracle's stream, and the stream's size."""
    out, total, at = [], 0, 0
    for N, L in zip(Ns, Ls):
        w = O.encode_chunk(x[at:at + N], (m, L))
        assert int(w[0]) == N
        p = 1
        for _ in range(-(-N // L)):
            out.append(int(w[p]))
            p += int(w[p]) + 1
        assert p == w.size
        total += w.size
        at += N
    return np.array(out, np.uint32), total


def test_constants_are_found_and_related_as_the_shapes_assume(K):
    assert K["kSelSegBits"] == 32 * K["kSelSeg"] and K["kSelBlockWords"] == 64 * K["kSelSeg"]
    assert K["kGcPiece"] % 4 == 0 and K["kGsBlock"] > 0 and K["kSelMaxGrid"] > 0 and K["waves_max_wavefronts"] > 0


def test_exact_sizes_sit_on_the_segment_block_and_piece_boundaries(O, K):
    x, Ns, Ls, want = exact_batch()
    n_i, total = chain(O, x, Ns, Ls, EXACT_M)
    assert np.array_equal(n_i, want)  # every draw, not only the formula
    have = set(want.tolist())
    seg, blk, piece = K["kSelSeg"], K["kSelBlockWords"], K["kGcPiece"]
    # k_decode_select: payloads of whole segments, of whole blocks, one word either side of a block, an entry of one word
    assert {seg, seg + 1, 2 * seg, 1} <= have
    assert {blk - 1, blk, blk + 1, 2 * blk - 1, 2 * blk, 4 * blk - 1, 4 * blk, 4 * blk + 1} <= have
    # ... a block whose last code ends with the block while the waveform goes on (carry_in == 0 against end_last ==
    # kSelSegBits), in codes that never re-synchronise: 4 bits a sample, 16384 samples, two blocks
    assert CONSTANT_LEN[16384] == 2 * blk and (blk * 32) % 4 == 0
    # wave_copy_words: cnt = n_i + 1 words at and around a piece and two pieces, and below four (no vector part)
    cnt = {n + 1 for n in have}
    assert {piece - 1, piece, piece + 1, 2 * piece, 2 * piece + 1} <= cnt and {2, 3} <= cnt
    # the piece loop more than once in ONE wavefront: slots == 1, entries of more than a piece; a wavefront per entry by default
    slots, mean = slots_of(K, total, want.size)
    assert slots == 1 and mean >= K["kGatherWavesFromWords"] and max(cnt) > 2 * piece


def test_levels_need_a_second_pass_of_the_piece_loop(O, K):
    x, Ns, Ls = levels_batch()
    n_i, total = chain(O, x, Ns, Ls, LEVELS["m"])
    assert set(n_i[0::2].tolist()) == {LEVELS["L"] * 4 // 32} and int(n_i[1::2].min()) > 5400
    slots, mean = slots_of(K, total, n_i.size)
    assert slots == 2 and mean >= K["kGatherWavesFromWords"]
    assert int(n_i.max()) + 1 > slots * K["kGcPiece"]  # a loud entry: its wavefronts come round again (p += slots * kGcPiece)
    # (f) the same stream stated by a capacity: other slots, the same bytes wanted
    big, _ = slots_of(K, total * CAPACITY_FACTOR, n_i.size)
    assert big not in (slots, K["slots_max"]) and big > 2


def defined_at_m1(x, N, L, n_chunks):
    """M = 1 is defined only while z < 32768: |delta| < 16384 in every waveform, the first sample's delta from zero."""
    for c in range(n_chunks):
        w = x[c * N:c * N + (N // L) * L].reshape(-1, L).astype(np.int64)
        if int(np.abs(np.diff(w, axis=1, prepend=0)).max()) >= 16384:
            return False
    return True


def test_silent_and_loud_waveforms_share_a_chunk(O, K):
    """The issue's "mixed" shape: very different code lengths in one chunk, chains of very different counts -- but none over
    kSwCap, so k_walk_sparse walks these chunks itself and the cell is one of data, not of the fallback."""
    x, Ns, Ls = silent_loud_batch()
    g = SILENT_LOUD
    assert defined_at_m1(x, Ns[0], g["L"], g["n_chunks"])
    for c in range(g["n_chunks"]):
        n_i, total = chain(O, x[c * Ns[0]:(c + 1) * Ns[0]], Ns[:1], Ls[:1], g["m"])
        quiet = n_i[:(3 * g["W"]) // 4 - 1]
        assert set(quiet.tolist()) == {-(-g["L"] // 32)}  # one bit per sample
        assert int(n_i[(3 * g["W"]) // 4 + 1:-1].min()) > 20 * int(quiet[0])
        per_chain, _ = chain_headers(K, n_i, g["W"])
        assert per_chain.sum() == g["W"] and per_chain.min() <= 3 and 40 < per_chain.max() < K["kSwCap"]


def test_a_chain_overflows_and_the_scalar_walker_takes_the_chunk(O, K):
    """CHAIN_OVERFLOW: the selection walks such a chunk by chains (select_walk_class() == 0), chain 0 meets more than kSwCap
    headers before its cut, k_walk_sparse flags the chunk and k_walk_scalar_only walks it -- in every chunk of the batch, so
    also in the two a selection of chunks 0 and 2 names."""
    x, Ns, Ls = chain_overflow_batch()
    g = CHAIN_OVERFLOW
    assert g["L"] > K["kWalkShortLen"] and K["kSwMinWaves"] <= g["W"] <= K["kSwMaxWaves"]  # the chain walk's chunk
    assert g["W"] // 8 >= K["kSwSegs"]  # all its chains
    assert defined_at_m1(x, Ns[0], g["L"], g["n_chunks"])
    for c in range(g["n_chunks"]):
        n_i, total = chain(O, x[c * Ns[0]:(c + 1) * Ns[0]], Ns[:1], Ls[:1], g["m"])
        assert total // g["W"] <= 8192  # (not the one-chain form)
        per_chain, before_cut_1 = chain_headers(K, n_i, g["W"])
        assert before_cut_1 > K["kSwCap"] and per_chain[0] > K["kSwCap"], (c, before_cut_1)
        assert set(n_i[:before_cut_1].tolist()) == {-(-g["L"] // 32)}  # silent waveforms all the way to the cut


def test_lists_exceed_every_launch_cap(O, K):
    x, Ns, Ls = caps_batch()
    g = CAPS
    n_i, total = chain(O, x, Ns, Ls, g["m"])
    assert g["n_select"] > K["kSelMaxGrid"]  # k_decode_select strides over the list
    assert -(-g["n_gather"] // K["kGsBlock"]) > K["scan_round"]  # k_gather_scan's outer loop, with its carry
    slots, mean = slots_of(K, total, n_i.size)
    assert slots == 1 and mean < K["kGatherWavesFromWords"]  # a workgroup per run by default: the other form by its flag
    assert g["n_gather"] * slots > K["waves_max_wavefronts"]  # k_gather_waves strides over its items
    assert (g["n_gather"] + 3) // 4 > K["waves_max_wavefronts"] // 4
    assert g["n_gather"] % g["cw"] != 0 and g["n_gather"] // g["cw"] >= 64  # the chunks of entries 2^20 j, a short last chunk
    assert g["n_gather"] < 1 << 32 and g["cw"] * g["L"] < 1 << 31


def test_a_capacity_changes_the_copy_form_of_a_short_batch(O, K):
    from test_gpu_routes import BATCHES
    Ns, Ls, m, taps, sigma = BATCHES["short"]
    x = np.random.default_rng(sum(map(ord, "short"))).normal(0, sigma, sum(Ns)).astype(np.int16)
    n_i, total = chain(O, x, Ns, Ls, m)
    assert total // n_i.size < K["kGatherWavesFromWords"] <= total * CAPACITY_FACTOR // n_i.size
