"""RiceParameter and encoding-filter optimiser (the routine the reference's docs describe but do not ship:
/root/reference/docs/Optimization.md:5-19, "capable of minimizing both in tandem"; docs/Algorithm.md:20).

The search is the one the docs spell out (Optimization.md:17-19): start from the caller's filter; test every filter of the
same length whose taps lie within +-search of the current one (filters with a zero at either end are invalid: the zero changes
nothing but the stored length); if the current filter is the best of its neighbourhood stop, otherwise move to the best and
repeat; sizes already computed are kept.  What is minimised is the EXACT size of the encoded batch -- ``drx_estimate_words``
counts, on the GPU and in one pass per filter, the words the encoder would write for every RiceParameter 2^0 .. 2^15
(``k_estimate_words``, csrc/drx_encode_kernels.hip) -- so M is optimised in tandem: a filter's score is its best k's size.

Nothing here runs on the CPU but the loop over candidate filters; the samples stay in HBM.  optimise_encoded() runs the same
search over a batch that exists only ENCODED: a filter's sizes come from the stream (``drx_estimate_words_encoded_filter``).
"""
from __future__ import annotations

import itertools
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .codec import Context, EncodedBatch, Plan


def _valid(taps: Tuple[int, ...], lossless: bool) -> bool:
    if taps[0] == 0 or taps[-1] == 0:  # Optimization.md:15 ("should not have zeros on either end"); taps[0] divides
        return False
    if lossless and abs(taps[0]) != 1:  # decodeWaveform divides by filter[0] in integers (src/deltaRice.c:91-102): exact
        return False                    # for every input only when it is +-1
    return True


def search_filters(size_of, taps: Sequence[int], search: int, lossless: bool, max_steps: int, ks: Optional[Sequence[int]]):
    """The neighbourhood search of Optimization.md:17-19 over any measure of size: size_of(taps) -> the sixteen sizes in words
    of the batch under that filter, called once per filter.  -> (taps, k, words, steps, evaluated)."""
    ks = list(range(16)) if ks is None else [int(k) for k in ks]
    cur = tuple(int(t) for t in taps)
    if not _valid(cur, lossless):
        raise ValueError(f"initial filter {cur} is not valid (zero at an end" + (", or taps[0] != +-1)" if lossless else ")"))
    seen: Dict[Tuple[int, ...], np.ndarray] = {}

    def score(f: Tuple[int, ...]) -> Tuple[int, int]:
        if f not in seen:
            seen[f] = size_of(f)
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
    return cur, best_k, best, steps, seen


def _result(found, n_samples: int):
    cur, best_k, best, steps, seen = found
    return {"taps": cur, "k": best_k, "m": 1 << best_k, "words": best, "bits_per_sample": 32.0 * best / n_samples,
            "steps": steps, "evaluated": seen}


def optimise(ctx: Context, x: torch.Tensor, chunk_samples: int, wave_len: int, taps: Sequence[int] = (1, -1), search: int = 1,
             lossless: bool = True, max_steps: int = 64, ks: Optional[Sequence[int]] = None):
    """-> dict(taps, k, m, words, bits_per_sample, steps, evaluated).

    x: int16 samples on the context's device, a whole number of chunks of chunk_samples; wave_len as in compression_opts
    (<= 0: the whole chunk); taps: the initial filter, its length is kept; search: s of Optimization.md:19 ((2s+1)^n
    neighbours per step); lossless: only filters the reference decodes exactly (taps[0] = +-1); ks: RiceParameters 2^k to
    consider (default all sixteen).  `evaluated` maps every filter tried to its sixteen sizes in words."""
    n = x.numel()
    if n == 0 or n % chunk_samples:
        raise ValueError("x must hold a whole number of chunks")
    n_chunks = n // chunk_samples
    L = wave_len if wave_len and wave_len > 0 else chunk_samples
    plan = ctx.plan_uniform(n_chunks, chunk_samples, (8, L))  # (the plan's own k does not enter the estimate)

    def size_of(f: Tuple[int, ...]) -> np.ndarray:
        plan.set_filter(f)  # ([1, -1] selects the delta kernels again)
        return plan.estimate_words(x)

    try:
        return _result(search_filters(size_of, taps, search, lossless, max_steps, ks), n)
    finally:
        plan.close()


def optimise_encoded(ctx: Context, plan: Plan, enc: EncodedBatch, taps: Optional[Sequence[int]] = None, search: int = 1,
                     lossless: bool = True, max_steps: int = 64, ks: Optional[Sequence[int]] = None,
                     wave_words: Optional[torch.Tensor] = None):
    """optimise() over an ENCODED batch: the same search, a filter's sixteen sizes taken from the stream by
    ``plan.estimate_words_refiltered`` (the words ``plan.refilter(enc, taps, 2^k)`` would give) -- no decoded sample in memory.
    plan describes the source as it does for decode(); taps None: the search starts from the plan's own filter.  -> the same
    dict; ``plan.refilter(enc, r["taps"], r["m"])`` then re-codes the batch.  ctx: the plan's context."""
    if taps is None:
        taps = plan._taps if plan._taps is not None else (1, -1)
    found = search_filters(lambda f: plan.estimate_words_refiltered(enc, f, wave_words), taps, search, lossless, max_steps, ks)
    return _result(found, plan.total_samples)
