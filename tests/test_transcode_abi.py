"""CPU: the surface of drx_transcode / drx_estimate_words_encoded -- exports, signatures, DRX_PATH_TRANSCODE in the header,
the binding and the package, what a closed plan answers, and the arguments Transcoded.plan() hands on.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("drx_transcode", "drx_transcode_with_wave_words", "drx_estimate_words_encoded")


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
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [9, 10, 6]


def test_path_constant():
    import deltarice_amd as dr
    from deltarice_amd import _lib
    assert re.search(r"^#define DRX_PATH_TRANSCODE 1024u\b", header(), flags=re.M)
    assert _lib.PATH_TRANSCODE == 1024 and dr.PATH_TRANSCODE == 1024
    paths = [getattr(_lib, n) for n in dir(_lib) if n.startswith("PATH_")]
    assert len(set(paths)) == len(paths)  # a bit of its own


def test_null_plan_is_refused():
    from deltarice_amd import _lib
    lib = _lib.load()
    out = (C.c_uint64 * 16)()
    assert lib.drx_transcode(None, None, 0, None, 3, None, 0, None, None) == 1
    assert lib.drx_transcode_with_wave_words(None, None, 0, None, None, 3, None, 0, None, None) == 1
    assert lib.drx_estimate_words_encoded(None, None, 0, None, None, out) == 1


def test_closed_plan_raises():
    import deltarice_amd as dr
    from deltarice_amd.codec import Plan
    plan = Plan.__new__(Plan)
    plan._h = None
    for call in (lambda: plan.transcode(None), lambda: plan.transcode(None, rice_m=16),
                 lambda: plan.transcode_async(None, None, 16), lambda: plan.estimate_words_encoded(None)):
        with pytest.raises(dr.DeltaRiceError) as e:
            call()
        assert e.value.status == 1 and "closed" in str(e.value)


class FakeCtx:
    def __init__(self):
        self.calls = []

    def plan_uniform(self, *a):
        self.calls.append(("uniform",) + a)
        return "U"

    def plan(self, *a):
        self.calls.append(("ragged",) + a)
        return "R"


def test_transcoded_plan_arguments():
    import dataclasses
    import deltarice_amd as dr
    T = dr.Transcoded
    assert [f.name for f in dataclasses.fields(T)] == ["enc", "wave_words", "rice_m", "taps", "chunk_samples", "wave_lens"]
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    c = FakeCtx()
    assert T(None, None, 32, None, i64(14000, 14000), i64(7000, 7000)).plan(c) == "U"
    assert c.calls[-1] == ("uniform", 2, 14000, (32, 7000))
    assert T(None, None, 4, (1, -1, 1, -1), i64(600, 600, 600), i64(200, 200, 200)).plan(c) == "U"
    assert c.calls[-1] == ("uniform", 3, 600, (4, 200, 4, 1, 0xFFFFFFFF, 1, 0xFFFFFFFF))
    assert T(None, None, 1, None, i64(999), i64(0)).plan(c) == "U"  # the whole chunk: WaveformLength -1
    assert c.calls[-1] == ("uniform", 1, 999, (1, 0xFFFFFFFF))
    assert T(None, None, 16, (3, -1), i64(1000, 2000), i64(100, 0)).plan(c) == "R"
    assert c.calls[-1] == ("ragged", [1000, 2000], [100, 0], 16, (3, -1))
    with pytest.raises(dr.DeltaRiceError):
        T(None, None, 8, None, i64(), i64()).plan(c)
