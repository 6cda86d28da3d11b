"""CPU: the surface of drx_transcode_filter / drx_estimate_words_encoded_filter -- exports and signatures against the header,
the form bits and the debug flag in the header, the binding and the package, what a NULL and a closed plan answer -- and the
filter search that optimise() and optimise_encoded() share, driven by a fake measure of size.  No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("drx_transcode_filter", "drx_transcode_filter_with_wave_words", "drx_estimate_words_encoded_filter")


def header():
    return open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()


def test_exports_and_signatures():
    from deltarice_amd import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), n
        m = re.search(r"\bdrx_status\s+" + n + r"\s*\(([^)]*)\)", code)
        assert m, n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), n
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [11, 12, 8]


def test_form_bits_and_debug_flag():
    import deltarice_amd as dr
    from deltarice_amd import _lib
    h = header()
    assert re.search(r"^#define DRX_TRANSCODE_FORM_REFILTER 8u\b", h, flags=re.M)
    assert re.search(r"^#define DRX_TRANSCODE_FORM_REFILTER_SERIAL 16u\b", h, flags=re.M)
    assert (_lib.TRANSCODE_FORM_REFILTER, _lib.TRANSCODE_FORM_REFILTER_SERIAL) == (8, 16)
    assert (dr.TRANSCODE_FORM_REFILTER, dr.TRANSCODE_FORM_REFILTER_SERIAL) == (8, 16)
    forms = [_lib.TRANSCODE_FORM_LANES, _lib.TRANSCODE_FORM_BLOCKS, _lib.TRANSCODE_FORM_FALLBACK_ALL, _lib.TRANSCODE_FORM_REFILTER,
             _lib.TRANSCODE_FORM_REFILTER_SERIAL]
    assert forms == [1, 2, 4, 8, 16]  # bits of their own
    m = re.search(r"^#define DRX_DBG_REFILTER_SERIAL (\d+)u\b", h, flags=re.M)
    assert m and int(m.group(1)) == _lib.DBG_REFILTER_SERIAL == dr.DBG_REFILTER_SERIAL
    flags = [int(v) for v in re.findall(r"^#define DRX_DBG_\w+ (\d+)u\b", h, flags=re.M)]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)  # one free bit each


def test_null_plan_is_refused():
    from deltarice_amd import _lib
    lib = _lib.load()
    out = (C.c_uint64 * 16)()
    taps = (C.c_int32 * 2)(1, -1)
    assert lib.drx_transcode_filter(None, None, 0, None, 3, 2, taps, None, 0, None, None) == 1
    assert lib.drx_transcode_filter_with_wave_words(None, None, 0, None, None, 3, 2, taps, None, 0, None, None) == 1
    assert lib.drx_estimate_words_encoded_filter(None, None, 0, None, None, 2, taps, out) == 1


def test_closed_plan_raises():
    import deltarice_amd as dr
    from deltarice_amd.codec import Plan
    plan = Plan.__new__(Plan)
    plan._h = None
    for call in (lambda: plan.refilter(None, (1, -1, 1, -1)), lambda: plan.refilter(None, (1, -1), rice_m=16),
                 lambda: plan.refilter_async(None, None, (1, -2, 1), 16), lambda: plan.estimate_words_refiltered(None, (1, -2, 1))):
        with pytest.raises(dr.DeltaRiceError) as e:
            call()
        assert e.value.status == 1 and "closed" in str(e.value)


def test_target_taps_of_the_python_surface():
    import deltarice_amd as dr
    from deltarice_amd.codec import Plan
    arr, n, carried = Plan._target_taps((1, -1))
    assert (list(arr), n, carried) == ([1, -1], 2, None)  # the delta filter: Transcoded carries None
    assert Plan._target_taps(None)[2] is None
    arr, n, carried = Plan._target_taps([-1, 2147483647, -2147483648, 65537])
    assert (list(arr), n, carried) == ([-1, 2147483647, -2147483648, 65537], 4, (-1, 2147483647, -2147483648, 65537))
    for bad in ((), (1,) * 65, (1, 1 << 31)):
        with pytest.raises(dr.DeltaRiceError):
            Plan._target_taps(bad)


# --------------------------------------------------------------------------- the search, with a fake measure of size
def reference_search(size_of, taps, search, lossless, max_steps, ks):
    """optimise()'s loop as it stood before the search was factored out of it, over size_of(taps) -> sixteen sizes"""
    from deltarice_amd.optimise import _valid
    ks = list(range(16)) if ks is None else list(ks)
    cur = tuple(taps)
    seen, order = {}, []

    def score(f):
        if f not in seen:
            seen[f] = size_of(f)
            order.append(f)
        w = seen[f]
        k = min(ks, key=lambda kk: (int(w[kk]), kk))
        return int(w[k]), k

    steps = 0
    best, best_k = score(cur)
    while steps < max_steps:
        steps += 1
        cand, cand_words, cand_k = cur, best, best_k
        for delta in itertools.product(range(-search, search + 1), repeat=len(cur)):
            f = tuple(t + d for t, d in zip(cur, delta))
            if f == cur or not _valid(f, lossless):
                continue
            w, k = score(f)
            if w < cand_words:
                cand, cand_words, cand_k = f, w, k
        if cand == cur:
            break
        cur, best, best_k = cand, cand_words, cand_k
    return cur, best_k, best, steps, seen, order


def bowl(centre):
    """a measure with one minimum: sizes[k] = 1000 + 50 |f - centre|_1 + 10 |k - 5|"""
    def size_of(f):
        d = sum(abs(a - b) for a, b in zip(f, centre))
        return np.array([1000 + 50 * d + 10 * abs(k - 5) for k in range(16)], np.uint64)
    return size_of


@pytest.mark.parametrize("start,centre,search,lossless,max_steps,ks", [
    ((1, -1, 1), (1, -3, 2), 1, True, 64, None),     # walks two steps and stops at the centre
    ((1, -1, 1), (1, -3, 2), 1, True, 1, None),      # stopped by max_steps
    ((1, -1), (3, -2), 2, False, 64, (0, 1, 2)),     # leads other than +-1 allowed, a restricted set of k
    ((1, -1), (3, -2), 1, True, 64, None),           # lossless: the lead stays +-1
    ((-1, 2, -1, 1), (-1, 2, -1, 1), 1, True, 64, None),  # already the best of its neighbourhood
])
def test_search_helper_is_optimises_loop(start, centre, search, lossless, max_steps, ks):
    from deltarice_amd.optimise import _valid, search_filters
    calls = []

    def counted(f):
        calls.append(f)
        return bowl(centre)(f)

    taps, k, words, steps, seen = search_filters(counted, start, search, lossless, max_steps, ks)
    w_taps, w_k, w_words, w_steps, w_seen, w_order = reference_search(bowl(centre), start, search, lossless, max_steps, ks)
    assert (taps, k, words, steps) == (w_taps, w_k, w_words, w_steps)
    assert calls == w_order and len(set(calls)) == len(calls)  # the same filters in the same order, each measured once
    assert list(seen) == w_order and all(np.array_equal(seen[f], w_seen[f]) for f in seen)
    assert all(_valid(f, lossless) for f in seen)
    if max_steps == 64:  # it stopped because the neighbourhood holds nothing smaller: every valid neighbour was visited
        for delta in itertools.product(range(-search, search + 1), repeat=len(taps)):
            f = tuple(t + d for t, d in zip(taps, delta))
            assert not _valid(f, lossless) or (f in seen and int(seen[f].min() if ks is None else min(seen[f][list(ks)])) >= words)


def test_search_helper_refuses_an_invalid_start():
    from deltarice_amd.optimise import search_filters
    for taps, lossless in (((0, 1), True), ((1, 0), False), ((2, -1), True)):
        with pytest.raises(ValueError):
            search_filters(lambda f: 1 / 0, taps, 1, lossless, 4, None)  # (refused before anything is measured)


def test_optimise_encoded_is_exported():
    import deltarice_amd as dr
    from deltarice_amd import optimise as mod
    assert dr.optimise_encoded is mod.optimise_encoded and callable(mod.optimise)
