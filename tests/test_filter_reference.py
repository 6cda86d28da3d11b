"""CPU: the oracle's prediction filter, 1 to 64 taps, against an independent statement of the reference's source lines
(tests/filter_reference.py), and both against the compiled reference where that is defined (tests/golden/ref_filters.json,
written by tests/golden/make_golden.py).  Every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_reference as F
from conftest import GOLDEN_DIR, ROOT
from oracle import oracle as O

CHILD_TIME_LIMIT = 120  # seconds for the whole table in the compiled reference (it takes about one)


def test_array_forms_are_the_source_lines():
    """forward / inverse (arrays, one wrap per sample in the inverse) against the literal transcriptions, every filter."""
    rng = np.random.default_rng(5)
    for name, taps in F.FILTERS.items():
        n = len(taps) + 7
        for x in (rng.integers(-32768, 32768, n), np.full(n, -32768), rng.integers(-40, 40, n)):
            d = F.forward(x, taps)
            assert np.array_equal(d, F.forward_literal(x, taps)), name
            assert np.array_equal(F.inverse(d, taps), F.inverse_literal(d, taps)), name
            assert np.array_equal(F.inverse(x, taps), F.inverse_literal(x, taps)), name  # (any residuals, not only a filter's)
        two = rng.integers(-32768, 32768, (2, n))
        assert np.array_equal(F.forward(two, taps)[1], F.forward_literal(two[1], taps)), name
        assert np.array_equal(F.inverse(two, taps)[1], F.inverse_literal(two[1], taps)), name


def test_division_is_towards_zero():
    # src/deltaRice.c:99 with a negative divisor that is no unit, and the one quotient that does not fit a short
    assert F.inverse_literal([7, -7, 1, -1], (-2,)).tolist() == [-3, 3, 0, 0]
    assert F.inverse([7, -7, 1, -1], (-2,)).tolist() == [-3, 3, 0, 0]
    assert F.inverse([-32768], (-1,)).tolist() == [-32768]
    assert O.decode_chunk(O.encode_chunk(np.array([7, -7, 1, -1], np.int16), (8, 4, 1, 1)), (8, 4, 1, 0xFFFFFFFE)).tolist() == [-3, 3, 0, 0]


def test_words_of_the_docs_example():
    assert F.forward([-2, 23], (1, -1)).tolist() == [-2, 25] and F.words([-2, 25], 3) == 1
    assert F.words(np.zeros(7000, np.int16), 3) == 875


@pytest.mark.parametrize("name", list(F.FILTERS))
def test_oracle_against_the_statement(name):
    taps = F.FILTERS[name]
    for kind, L, n, m, x in F.cases(name):
        what = (name, kind, L, n, m)
        k = m.bit_length() - 1
        opts = F.opts_of(m, L, taps)
        d = F.chunk_residuals(x, L, taps)
        w = O.encode_chunk(x, opts)
        assert int(w[0]) == n, what                                      # the chunk header
        at = 1
        for s, length in F.waveforms(n, L):                              # every n_i along the chain, and what it heads
            n_i = int(w[at])
            assert n_i == F.words(d[s:s + length], k), what
            got, bits = O.rice_unpack(w[at + 1:at + 1 + n_i], length, k)
            assert np.array_equal(got, d[s:s + length]) and (bits + 31) // 32 == n_i, what
            at += 1 + n_i
        assert at == w.size, what
        want = F.chunk_decoded(d, L, taps)
        y = O.decode_chunk(w, opts)
        assert np.array_equal(y, want), what                             # every decoded sample, the lossy leads included
        assert np.array_equal(O.decode_chunk(w, opts, fast=True), want), what
        if F.lossless(taps):
            assert np.array_equal(y, x), what


@pytest.mark.parametrize("name", ["delta0", "delta00"])
def test_delta_with_zero_taps_gives_the_delta_bytes(name):
    for kind, L, n, m, x in F.cases(name):
        assert np.array_equal(O.encode_chunk(x, F.opts_of(m, L, F.FILTERS[name])), O.encode_chunk(x, (m, L))), (kind, L, n)


def test_identity_modulo_2_16():
    for kind, L, n, m, x in F.cases("identity_mod"):
        assert np.array_equal(F.chunk_residuals(x, L, F.FILTERS["identity_mod"]), x)
        assert np.array_equal(O.encode_chunk(x, F.opts_of(m, L, (1, 65536))), O.encode_chunk(x, (m, L, 1, 1)))


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN_DIR, "ref_filters.json")) as f:
        return json.load(f)["filters"]


def test_oracle_against_the_pinned_reference(pinned):
    """The compiled reference's bytes and decoded samples for every case of the table it is defined at, 5 to 64 taps included."""
    assert max(len(p["taps"]) for p in pinned) == 64
    mine = [d for d in (F.digests(name, O.encode_chunk, O.decode_chunk) for name in F.FILTERS) if d]
    assert [d["filter"] for d in mine] == [p["filter"] for p in pinned]
    for d, p in zip(mine, pinned):
        assert d == p, d["filter"]


def test_compiled_reference_against_its_pins(pinned):
    """Where oracle/_ref is built: the reference itself, in a child process under a time limit (outside its domain it can fail
    to return)."""
    if not O.have_ref("omp"):
        pytest.skip("oracle/_ref is not built here; the pins stand in for it")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_filters_child.py"), "omp"], capture_output=True,
                       text=True, timeout=CHILD_TIME_LIMIT)
    assert r.returncode == 0, r.stderr[-2000:]
    live = [json.loads(line) for line in r.stdout.splitlines()]
    assert [d["filter"] for d in live] == [p["filter"] for p in pinned]
    for d, p in zip(live, pinned):
        assert d == p, d["filter"]
