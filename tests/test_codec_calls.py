"""CPU: what every launching entry of deltarice_amd.codec.Plan hands to the library -- which drx_* symbol, which pointers, strides,
NULLs and scalars, in the order of the prototypes of include/deltarice_hip.h -- recorded by the stand-in of tests/plan_standin.py
(one chunk, three waveforms, device ``cpu``) and held to expectations written by hand; and a closed plan in every entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from deltarice_amd import DeltaRiceError, _lib
from plan_standin import NULL_PLAN, plan as standin

H = 1      # the stand-in's plan handle
ANY = object()  # an argument that is not looked at (a pointer to no entries)
BOTH = pytest.mark.parametrize("sideband", [False, True], ids=["walk", "sideband"])


def _plain(a):
    if isinstance(a, C.Array):
        assert type(a)._type_ is C.c_int32
        return ("int32",) + tuple(a)
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value
    return a


def calls(plan):
    """The record so far, ctypes pointers as addresses and ctypes arrays as (type, values...); the record starts again."""
    got = [(name, tuple(_plain(a) for a in args)) for name, args in plan.ctx.lib.calls]
    plan.ctx.lib.calls.clear()
    return got


def expect(plan, name, sideband, ww, *args):
    """The one recorded call is drx_<name>(plan, words, in_words, chunk_word_off, *args), or its _with_wave_words form with the
    table in front of args; args[:3] are (words pointer, in_words, chunk_word_off pointer)."""
    want = (H,) + args[:3] + ((ww.data_ptr(),) if sideband else ()) + args[3:]
    got = calls(plan)
    assert len(got) == 1, got
    assert got[0][0] == "drx_" + name + ("_with_wave_words" if sideband else "")
    assert len(got[0][1]) == len(want), (got, want)
    for i, (g, w) in enumerate(zip(got[0][1], want)):
        assert w is ANY or (g == w and type(g) is type(w)), (name, i, g, w)


def batch(total_waves=3):
    return (torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(total_waves, dtype=torch.int32))


def columns(W):
    """name -> (the int64 column handed in, the stride the library is to see)"""
    table = torch.arange(W * 8, dtype=torch.int64).view(W, 8)
    return {"contiguous": (torch.arange(W, dtype=torch.int64), 1), "column 3 of [W, 8]": (table[:, 3], 8 if W > 1 else 1)}


def test_the_real_library_on_a_null_plan():
    # the five entries that left a closed plan to the library: what the stand-in's library answers for a None handle
    lib = _lib.load()
    assert lib.drx_encode(None, None, None, 0, None) == NULL_PLAN
    assert lib.drx_decode(None, None, 0, None, None) == NULL_PLAN
    assert lib.drx_decode_with_wave_words(None, None, 0, None, None, None) == NULL_PLAN
    assert lib.drx_decode_select(None, None, 0, None, None, 1, None, 0) == NULL_PLAN
    assert lib.drx_decode_select_with_wave_words(None, None, 0, None, None, None, 1, None, 0) == NULL_PLAN
    assert lib.drx_gather_encoded(None, None, 0, None, None, 1, 1, None, 0, None, None) == NULL_PLAN
    assert lib.drx_gather_encoded_with_wave_words(None, None, 0, None, None, None, 1, 1, None, 0, None, None) == NULL_PLAN
    assert NULL_PLAN == 1  # DRX_ERR_ARG


def test_encode():
    plan = standin()
    x = torch.zeros(250, dtype=torch.int16)
    out, off = torch.zeros(40, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    assert [t.data_ptr() for t in plan.encode_async(x, out, off)] == [out.data_ptr(), off.data_ptr()]
    assert calls(plan) == [("drx_encode", (H, x.data_ptr(), out.data_ptr(), 40, off.data_ptr()))]
    out, off = plan.encode_async(x)  # the plan's bound
    assert out.dtype == torch.int32 and out.numel() == plan.max_encoded_words and off.dtype == torch.int64 and off.numel() == 2
    assert calls(plan) == [("drx_encode", (H, x.data_ptr(), out.data_ptr(), 300, off.data_ptr()))]
    out, off = plan.encode_async(x, capacity_words=7)
    assert calls(plan) == [("drx_encode", (H, x.data_ptr(), out.data_ptr(), 7, off.data_ptr()))]


@BOTH
def test_decode(sideband):
    plan = standin()
    words, off, ww = batch()
    out = torch.zeros(250, dtype=torch.int16)
    launch = (lambda *a, **k: plan.decode_with_wave_words(words, off, ww, *a, **k)) if sideband else \
        (lambda *a, **k: plan.decode_async(words, off, *a, **k))
    assert launch(out).data_ptr() == out.data_ptr()
    expect(plan, "decode", sideband, ww, words.data_ptr(), 8, off.data_ptr(), out.data_ptr())
    got = launch(in_words=5)
    assert got.dtype == torch.int16 and got.shape == (250,)
    expect(plan, "decode", sideband, ww, words.data_ptr(), 5, off.data_ptr(), got.data_ptr())


@BOTH
def test_decode_select(sideband):
    plan = standin()
    words, off, ww = batch()
    kw = dict(wave_words=ww) if sideband else {}
    idx = np.array([2, 0, 2], dtype=np.uint64)
    out = torch.zeros((3, 100), dtype=torch.int16)
    assert plan.decode_select_async(words, off, idx, out, **kw) is out
    expect(plan, "decode_select", sideband, ww, words.data_ptr(), 8, off.data_ptr(), idx.ctypes.data, 3, out.data_ptr(), 100)
    rows = torch.zeros((3, 128), dtype=torch.int16)[:, :100]  # rows further apart than they are long
    plan.decode_select_async(words, off, idx, rows, in_words=5, **kw)
    expect(plan, "decode_select", sideband, ww, words.data_ptr(), 5, off.data_ptr(), idx.ctypes.data, 3, rows.data_ptr(), 128)
    one = torch.zeros((1, 120), dtype=torch.int16)  # one row: its length is the stride
    plan.decode_select_async(words, off, idx[:1], one, **kw)
    expect(plan, "decode_select", sideband, ww, words.data_ptr(), 8, off.data_ptr(), idx.ctypes.data, 1, one.data_ptr(), 120)


@BOTH
def test_gather_encoded(sideband):
    plan = standin()
    words, off, ww = batch()
    kw = dict(wave_words=ww) if sideband else {}
    idx = np.array([2, 0, 2], dtype=np.uint64)
    # out_words None and an empty out_words: the sizing call, NULL and capacity 0; two output chunks of two and one entries
    for out_words in (None, torch.zeros(0, dtype=torch.int32)):
        ow, ooff, otab = plan.gather_encoded_async(words, off, idx, 2, out_words, **kw)
        assert ow is out_words and (ooff.dtype, ooff.shape) == (torch.int64, (3,)) and (otab.dtype, otab.shape) == (torch.int32, (3,))
        expect(plan, "gather_encoded", sideband, ww, words.data_ptr(), 8, off.data_ptr(), idx.ctypes.data, 3, 2, None, 0,
               ooff.data_ptr(), otab.data_ptr())
    out_words = torch.zeros(16, dtype=torch.int32)
    got = plan.gather_encoded_async(words, off, idx, 2, out_words, 5, out_chunk_word_off=ooff, out_wave_words=otab, **kw)
    assert got[0] is out_words and got[1] is ooff and got[2] is otab
    expect(plan, "gather_encoded", sideband, ww, words.data_ptr(), 5, off.data_ptr(), idx.ctypes.data, 3, 2, out_words.data_ptr(), 16,
           ooff.data_ptr(), otab.data_ptr())
    # an empty selection: one table entry, no output chunk, NULL out_wave_words
    ow, ooff, otab = plan.gather_encoded_async(words, off, [], 2, out_words, **kw)
    assert ooff.shape == (1,) and otab.shape == (0,)
    expect(plan, "gather_encoded", sideband, ww, words.data_ptr(), 8, off.data_ptr(), ANY, 0, 2, out_words.data_ptr(), 16,
           ooff.data_ptr(), None)


@BOTH
def test_wave_stats(sideband):
    plan = standin()
    words, off, ww = batch()
    kw = dict(wave_words=ww) if sideband else {}
    out = plan.wave_stats_async(words, off, **kw)
    assert out.dtype == torch.int64 and out.shape == (3, _lib.STAT_COLS)
    expect(plan, "wave_stats", sideband, ww, words.data_ptr(), 8, off.data_ptr(), 0, out.data_ptr())
    assert plan.wave_stats_async(words, off, 500, out, in_words=5, **kw) is out
    expect(plan, "wave_stats", sideband, ww, words.data_ptr(), 5, off.data_ptr(), 500, out.data_ptr())


@BOTH
@pytest.mark.parametrize("W", [3, 1])
def test_wave_bins(W, sideband):
    plan = standin(W)
    words, off, ww = batch(W)
    kw = dict(wave_words=ww) if sideband else {}
    # no start: NULL and stride 0; the default n_bins covers the longest waveform (100 samples) from the offset
    out = plan.wave_bins_async(words, off, 10, offset=-5, **kw)
    assert out.dtype == torch.int64 and out.shape == (W, 11, _lib.BIN_COLS)
    expect(plan, "wave_bins", sideband, ww, words.data_ptr(), 8, off.data_ptr(), None, 0, -5, 10, 11, out.data_ptr(), 11 * _lib.BIN_COLS)
    for what, (start, stride) in columns(W).items():
        out = torch.zeros(W * 2 * _lib.BIN_COLS, dtype=torch.int64)
        assert plan.wave_bins_async(words, off, 25, 2, start, 7, out, in_words=5, **kw) is out
        expect(plan, "wave_bins", sideband, ww, words.data_ptr(), 5, off.data_ptr(), start.data_ptr(), stride, 7, 25, 2, out.data_ptr(),
               2 * _lib.BIN_COLS)
    # no bin: nothing to do, and the library is not called
    assert plan.wave_bins_async(words, off, 10, 0, **kw).shape == (W, 0, _lib.BIN_COLS)
    assert plan.wave_bins_async(words, off, 10, offset=100, **kw).shape == (W, 0, _lib.BIN_COLS)
    assert calls(plan) == []


@BOTH
@pytest.mark.parametrize("W", [3, 1])
def test_decode_window(W, sideband):
    plan = standin(W)
    words, off, ww = batch(W)
    kw = dict(wave_words=ww) if sideband else {}
    # no start, and an int, which is folded into the offset: NULL and stride 0
    for start, offset in ((None, -2), (7, 5)):
        out = plan.decode_window_async(words, off, start, 16, -2, -1, **kw)
        assert out.dtype == torch.int16 and out.shape == (W, 16)
        expect(plan, "decode_window", sideband, ww, words.data_ptr(), 8, off.data_ptr(), None, 0, offset, 16, -1, out.data_ptr(), 16)
    for what, (start, stride) in columns(W).items():
        out = torch.zeros((W - 1) * 20 + 16, dtype=torch.int16)
        assert plan.decode_window_async(words, off, start, 16, 3, 0, out, 20, in_words=5, **kw) is out
        expect(plan, "decode_window", sideband, ww, words.data_ptr(), 5, off.data_ptr(), start.data_ptr(), stride, 3, 16, 0, out.data_ptr(), 20)
    # rows further apart than they are long and no tensor given: a flat one that holds them
    out = plan.decode_window_async(words, off, None, 16, out_stride=20, **kw)
    assert out.shape == ((W - 1) * 20 + 16,)
    expect(plan, "decode_window", sideband, ww, words.data_ptr(), 8, off.data_ptr(), None, 0, 0, 16, 0, out.data_ptr(), 20)
    # no width: nothing to do, and the library is not called
    assert plan.decode_window_async(words, off, None, 0, **kw).shape == (W, 0)
    assert calls(plan) == []


@BOTH
@pytest.mark.parametrize("W", [3, 1])
def test_decode_windows(W, sideband):
    plan = standin(W)
    words, off, ww = batch(W)
    kw = dict(wave_words=ww) if sideband else {}
    count = torch.zeros(W, dtype=torch.int32)
    # a contiguous [W, 2]; a dimension of one entry passes its own stride
    start = torch.zeros((W, 2), dtype=torch.int64)
    rows = plan.decode_windows_async(words, off, start, 16, **kw)
    assert rows.dtype == torch.int16 and rows.shape == (W, 2, 16) and rows.stride() == (32, 16, 1)
    expect(plan, "decode_windows", sideband, ww, words.data_ptr(), 8, off.data_ptr(), start.data_ptr(), 2, 1, None, 2, 0, 16, 0,
           rows.data_ptr(), 32, 16)
    # the records of find_pulses as they are: [W, 4, PULSE_COLS][:, :, PULSE_START], with their count
    start = torch.zeros((W, 4, 5), dtype=torch.int64)[:, :, 0]
    rows = plan.decode_windows_async(words, off, start, 16, count, -64, -1, in_words=5, **kw)
    assert rows.shape == (W, 4, 16)
    expect(plan, "decode_windows", sideband, ww, words.data_ptr(), 5, off.data_ptr(), start.data_ptr(), 20, 5, count.data_ptr(), 4, -64, 16, -1,
           rows.data_ptr(), 64, 16)
    # K = 1: the one window's stride is its own, 5, not 1
    start = torch.zeros((W, 1, 5), dtype=torch.int64)[:, :, 0]
    assert start.stride() == (5, 5)
    rows = plan.decode_windows_async(words, off, start, 16, **kw)
    assert rows.shape == (W, 1, 16)
    expect(plan, "decode_windows", sideband, ww, words.data_ptr(), 8, off.data_ptr(), start.data_ptr(), 5, 5, None, 1, 0, 16, 0,
           rows.data_ptr(), 16, 16)
    # out_strides given: the strided view of the caller's tensor comes back
    start = torch.zeros((W, 2), dtype=torch.int64)
    out = torch.zeros((W - 1) * 40 + 20 + 16, dtype=torch.int16)
    rows = plan.decode_windows_async(words, off, start, 16, out=out, out_strides=(40, 20), **kw)
    assert rows.data_ptr() == out.data_ptr() and rows.shape == (W, 2, 16) and rows.stride() == (40, 20, 1)
    expect(plan, "decode_windows", sideband, ww, words.data_ptr(), 8, off.data_ptr(), start.data_ptr(), 2, 1, None, 2, 0, 16, 0,
           out.data_ptr(), 40, 20)
    # no width and no window slot: nothing to do, and the library is not called
    assert plan.decode_windows_async(words, off, start, 0, **kw).shape == (W, 2, 0)
    assert plan.decode_windows_async(words, off, torch.zeros((W, 0), dtype=torch.int64), 16, **kw).shape == (W, 0, 16)
    assert calls(plan) == []


@BOTH
@pytest.mark.parametrize("W", [3, 1])
def test_find_pulses(W, sideband):
    plan = standin(W)
    words, off, ww = batch(W)
    kw = dict(wave_words=ww) if sideband else {}
    # an int is folded into the offset: NULL and stride 0
    n, pulses = plan.find_pulses_async(words, off, 7, offset=2, **kw)
    assert (n.dtype, n.shape) == (torch.int32, (W,)) and (pulses.dtype, pulses.shape) == (torch.int64, (W, 4, _lib.PULSE_COLS))
    expect(plan, "find_pulses", sideband, ww, words.data_ptr(), 8, off.data_ptr(), None, 0, 9, 1, 1, 4, n.data_ptr(), pulses.data_ptr())
    for what, (thr, stride) in columns(W).items():
        count, out = torch.zeros(W, dtype=torch.int32), torch.zeros(W * 2 * _lib.PULSE_COLS, dtype=torch.int64)
        n, pulses = plan.find_pulses_async(words, off, thr, -5, 3, 2, 40, count, out, in_words=5, **kw)  # polarity -5 is -1
        assert n.data_ptr() == count.data_ptr() and pulses.data_ptr() == out.data_ptr() and pulses.shape == (W, 2, _lib.PULSE_COLS)
        expect(plan, "find_pulses", sideband, ww, words.data_ptr(), 5, off.data_ptr(), thr.data_ptr(), stride, 40, -1, 3, 2, count.data_ptr(),
               out.data_ptr())
    # the counting form: no records, NULL
    n, pulses = plan.find_pulses_async(words, off, 0, 9, max_pulses=0, **kw)
    assert pulses.shape == (W, 0, _lib.PULSE_COLS)
    expect(plan, "find_pulses", sideband, ww, words.data_ptr(), 8, off.data_ptr(), None, 0, 0, 1, 1, 0, n.data_ptr(), None)


@BOTH
def test_transcode_and_refilter(sideband):
    plan = standin()
    words, off, ww = batch()
    kw = dict(wave_words=ww) if sideband else {}
    forms = (("transcode", lambda *a, **k: plan.transcode_async(words, off, 16, *a, **k), (4,)),
             ("transcode_filter", lambda *a, **k: plan.refilter_async(words, off, (1, -2, 1), 4, *a, **k), (2, 3, ("int32", 1, -2, 1))),
             ("transcode_filter", lambda *a, **k: plan.refilter_async(words, off, None, 2, *a, **k), (1, 2, ("int32", 1, -1))))
    for name, launch, own in forms:
        # out_words None and an empty out_words: the sizing call, NULL and capacity 0
        for out_words in (None, torch.zeros(0, dtype=torch.int32)):
            ow, ooff, otab = launch(out_words, **kw)
            assert ow is out_words and (ooff.dtype, ooff.shape) == (torch.int64, (2,)) and (otab.dtype, otab.shape) == (torch.int32, (3,))
            expect(plan, name, sideband, ww, words.data_ptr(), 8, off.data_ptr(), *own, None, 0, ooff.data_ptr(), otab.data_ptr())
        out_words = torch.zeros(16, dtype=torch.int32)
        got = launch(out_words, 5, out_chunk_word_off=ooff, out_wave_words=otab, **kw)
        assert got[0] is out_words and got[1] is ooff and got[2] is otab
        expect(plan, name, sideband, ww, words.data_ptr(), 5, off.data_ptr(), *own, out_words.data_ptr(), 16, ooff.data_ptr(), otab.data_ptr())


def test_a_closed_plan_in_every_launching_entry():
    plan = standin()
    words, off, ww = batch()
    col, idx = torch.zeros(3, dtype=torch.int64), np.array([1], dtype=np.uint64)
    plan._h = None
    entries = {
        "encode_async": lambda: plan.encode_async(torch.zeros(250, dtype=torch.int16)),
        "decode_async": lambda: plan.decode_async(words, off),
        "decode_with_wave_words": lambda: plan.decode_with_wave_words(words, off, ww),
        "decode_select_async": lambda: plan.decode_select_async(words, off, idx, torch.zeros((1, 100), dtype=torch.int16)),
        "decode_select_async, side-band": lambda: plan.decode_select_async(words, off, idx, torch.zeros((1, 100), dtype=torch.int16), wave_words=ww),
        "gather_encoded_async": lambda: plan.gather_encoded_async(words, off, idx, 1),
        "gather_encoded_async, side-band": lambda: plan.gather_encoded_async(words, off, idx, 1, wave_words=ww),
        "wave_stats_async": lambda: plan.wave_stats_async(words, off),
        "wave_bins_async": lambda: plan.wave_bins_async(words, off, 10),
        "decode_window_async": lambda: plan.decode_window_async(words, off, col, 16),
        "decode_windows_async": lambda: plan.decode_windows_async(words, off, torch.zeros((3, 2), dtype=torch.int64), 16),
        "find_pulses_async": lambda: plan.find_pulses_async(words, off, col),
        "transcode_async": lambda: plan.transcode_async(words, off, 8),
        "refilter_async": lambda: plan.refilter_async(words, off, (1, -2, 1), 8),
    }
    for what, call in entries.items():
        with pytest.raises(DeltaRiceError) as e:
            call()
        assert e.value.status == 1, what
