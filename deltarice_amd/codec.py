"""Host side of the MI355X Delta-Rice codec: batches of HDF5 chunks resident in HBM.

PyTorch is used only as plumbing (device memory, streams); all arithmetic happens in
the HIP kernels behind the C ABI (include/deltarice_hip.h).  The option tuple has the
meaning of the reference's ``compression_opts`` (README.md:71-80 of the reference,
parsed at src/deltaRice.c:248-291): ``(RiceParameter[, WaveformLength[, nTaps, taps...]])``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import DeltaRiceError, DrxOpts

H5FILTER = 32025  # H5Z_FILTER_DELTARICE (reference src/deltaRice.h:7)


def _cd_values(opts: Sequence[int]):
    """compression_opts as the cd_values array the library takes beside len(opts)"""
    return (C.c_uint * max(len(opts), 1))(*[int(v) & 0xFFFFFFFF for v in opts])


def parse_opts(opts: Sequence[int] = ()) -> DrxOpts:
    """compression_opts -> parsed options; raises DeltaRiceError like the reference rejects
    (stderr + failure, src/deltaRice.c:114-136)."""
    lib = _lib.load()
    o = DrxOpts()
    st = lib.drx_parse_cd_values(len(opts), _cd_values(opts), C.byref(o))
    if st != _lib.DRX_OK:
        raise DeltaRiceError(st, f"compression_opts={tuple(opts)}")
    return o


# The scalar arguments of the stream calls, by the type the library takes them as: int(v), or DRX_ERR_ARG naming it.
def _uint32(v, name: str, least: int = 0) -> int:
    v = int(v)
    if not least <= v < 1 << 32:
        raise DeltaRiceError(1, f"{name}: {v} is not a uint32" + (f" of at least {least}" if least else ""))
    return v


def _int16(v, name: str) -> int:
    v = int(v)
    if not -32768 <= v <= 32767:
        raise DeltaRiceError(1, f"{name}: {v} is not an int16")
    return v


def _int64(v, name: str) -> int:
    v = int(v)
    if not -(1 << 63) <= v < 1 << 63:
        raise DeltaRiceError(1, f"{name}: {v} is not an int64")
    return v


def _stride(t: torch.Tensor, d: int) -> Optional[int]:
    """The element stride of dimension d as the library takes one: positive, or None; where the dimension has no second entry
    to step to, any stride will do, and one below 1 is passed as 1."""
    s = int(t.stride(d))
    return s if s >= 1 else (1 if t.shape[d] <= 1 else None)


def _is_delta(o: DrxOpts) -> bool:
    return o.n_taps == 2 and o.taps[0] == 1 and o.taps[1] == -1


def wave_lengths(chunk_samples: Sequence[int], wave_lens: Sequence[int], wave_idx) -> np.ndarray:
    """Samples of each waveform of ``wave_idx`` (global waveform indices) in a batch whose chunk c holds
    ``chunk_samples[c]`` samples in waveforms of ``wave_lens[c]`` (0 or less: the whole chunk): WaveformLength, or what is
    left for the last waveform of a chunk (src/deltaRice.c:399-403 of the reference).  Host arithmetic; no GPU."""
    N = np.asarray(chunk_samples, dtype=np.int64).reshape(-1)
    L = np.asarray(wave_lens, dtype=np.int64).reshape(-1)
    if N.size == 0 or N.size != L.size or (N <= 0).any():
        raise DeltaRiceError(1, "chunk_samples / wave_lens mismatch")
    L = np.where(L <= 0, N, L)
    W = (N + L - 1) // L
    base = np.concatenate(([0], np.cumsum(W)))
    idx = _as_index_array(wave_idx)
    if idx.size and int(idx.max()) >= int(base[-1]):
        raise DeltaRiceError(1, f"waveform index {int(idx.max())} out of range (the batch has {int(base[-1])})")
    g = idx.astype(np.int64)
    if (W == W[0]).all():  # (every chunk the same number of waveforms: no search)
        c = g // W[0]
    else:
        c = np.searchsorted(base, g, side="right") - 1
    i = g - base[c]
    return np.where(i + 1 == W[c], N[c] - i * L[c], L[c]).astype(np.int64)


def gather_geometry(chunk_samples: Sequence[int], wave_lens: Sequence[int], wave_idx, chunk_waves: int):
    """Geometry of the batch Plan.gather_encoded makes of the waveforms ``wave_idx`` names, ``chunk_waves`` to an output chunk:
    -> (chunk_samples, wave_lens) of the result, int64 each, as Context.plan() takes them.  Output chunk c holds entries
    [c * chunk_waves, (c + 1) * chunk_waves) of the list; its WaveformLength is its first entry's length, which every entry but
    its last must share (the last may be shorter): a list that breaks this raises DRX_ERR_ARG.  Host arithmetic; no GPU."""
    cw = int(chunk_waves)
    if cw < 1:
        raise DeltaRiceError(1, "chunk_waves must be at least 1")
    Ns = np.asarray(chunk_samples, dtype=np.int64).reshape(-1)
    Ls = np.asarray(wave_lens, dtype=np.int64).reshape(-1)
    if Ns.size and Ns.size == Ls.size and Ls[0] > 0 and Ns[0] % Ls[0] == 0 and (Ns == Ns[0]).all() and (Ls == Ls[0]).all():
        # every waveform of the batch has one length: any list at any chunking is valid, and its geometry is counting
        idx = _as_index_array(wave_idx)
        W = int(Ns.size * (Ns[0] // Ls[0]))
        if idx.size and int(idx.max()) >= W:
            raise DeltaRiceError(1, f"waveform index {int(idx.max())} out of range (the batch has {W})")
        n_out = -(-idx.size // cw)
        N = np.full(n_out, cw * int(Ls[0]), dtype=np.int64)
        if n_out:
            N[-1] = (idx.size - (n_out - 1) * cw) * int(Ls[0])
            if int(N.max()) >= 1 << 31:
                raise DeltaRiceError(1, f"output chunk 0 has {int(N.max())} samples (2^31 - 1 at most)")
        return N, np.full(n_out, int(Ls[0]), dtype=np.int64)
    lens = wave_lengths(chunk_samples, wave_lens, wave_idx)
    n = lens.size
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    first = np.arange(0, n, cw)
    last = np.minimum(first + cw, n) - 1
    L = lens[first]
    want = np.repeat(L, last - first + 1)
    is_last = np.zeros(n, dtype=bool)
    is_last[last] = True
    bad = np.nonzero((lens > want) | ((lens < want) & ~is_last))[0]
    if bad.size:
        e = int(bad[0])
        raise DeltaRiceError(1, f"entry {e} has {int(lens[e])} samples, output chunk {e // cw}'s first has {int(want[e])}"
                                + ("" if lens[e] > want[e] else " and it is not the chunk's last"))
    N = np.add.reduceat(lens, first)
    if int(N.max()) >= 1 << 31:
        raise DeltaRiceError(1, f"output chunk {int(N.argmax())} has {int(N.max())} samples (2^31 - 1 at most)")
    return N.astype(np.int64), L.astype(np.int64)


def _as_index_array(wave_idx) -> np.ndarray:
    """Any integer sequence, numpy array or CPU tensor -> contiguous uint64 [n]."""
    if isinstance(wave_idx, torch.Tensor):
        if wave_idx.device.type != "cpu":
            raise DeltaRiceError(1, "wave_idx: a selection lives on the host (a CPU tensor, an array or a sequence)")
        wave_idx = wave_idx.numpy()
    a = np.asarray(wave_idx).reshape(-1)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint64)
    if a.dtype.kind not in "iu":
        raise DeltaRiceError(1, f"wave_idx: integers wanted, got {a.dtype}")
    if a.dtype.kind == "i" and int(a.min()) < 0:
        raise DeltaRiceError(1, f"wave_idx: negative index {int(a.min())}")
    return np.ascontiguousarray(a, dtype=np.uint64)


@dataclass
class EncodedBatch:
    """Encoded chunks back to back in HBM + the table saying where each one starts."""
    words: torch.Tensor           # int32 storage of the uint32 stream, length = capacity
    chunk_word_off: torch.Tensor  # int64 [n_chunks + 1]
    total_words: int

    def chunk_bytes(self, c: int) -> bytes:
        off = self.chunk_word_off[c:c + 2].cpu().tolist()
        return self.words[off[0]:off[1]].cpu().numpy().view(np.uint32).tobytes()

    def to_numpy(self):
        w = self.words[:self.total_words].cpu().numpy().view(np.uint32)
        return w, self.chunk_word_off.cpu().numpy().astype(np.uint64)


@dataclass
class Gathered:
    """What Plan.gather_encoded returns: a new encoded batch made of selected waveforms, and all that is needed to use it."""
    enc: EncodedBatch             # the chunks, back to back, with their offset table
    chunk_samples: np.ndarray     # int64 [n_out_chunks]: N_c of every output chunk ...
    wave_lens: np.ndarray         # ... and its WaveformLength (what Context.plan() takes)
    wave_words: torch.Tensor      # int32 [n_sel] on the device: n_i of every entry, the result's side-band
    rice_m: int                   # the source plan's RiceParameter ...
    taps: Optional[tuple]         # ... and prediction filter (None: delta)

    def plan(self, ctx: "Context") -> "Plan":
        """The plan of the result: its own geometry, the source's RiceParameter and filter."""
        return _result_plan(ctx, self.chunk_samples, self.wave_lens, self.rice_m, self.taps, "an empty selection has no plan")


@dataclass
class Transcoded:
    """What Plan.transcode and Plan.refilter return: the source batch re-coded at another RiceParameter (refilter: and under
    another prediction filter), and all that is needed to use it."""
    enc: EncodedBatch             # the chunks, back to back, with their offset table
    wave_words: torch.Tensor      # int32 [total_waves] on the device: n_i of every waveform, the result's side-band
    rice_m: int                   # the RiceParameter of the result ...
    taps: Optional[tuple]         # ... and its prediction filter: the source plan's, or refilter's target (None: delta)
    chunk_samples: np.ndarray     # int64 [n_chunks]: the source plan's geometry (what Context.plan() takes)
    wave_lens: np.ndarray

    def plan(self, ctx: "Context") -> "Plan":
        """The plan of the result: the source's geometry, the result's filter and RiceParameter."""
        return _result_plan(ctx, self.chunk_samples, self.wave_lens, self.rice_m, self.taps, "an empty batch has no plan")


def _result_plan(ctx: "Context", chunk_samples, wave_lens, rice_m: int, taps: Optional[tuple], empty: str) -> "Plan":
    """The plan of a Gathered or a Transcoded: a uniform plan where every chunk is alike, a ragged one otherwise; a WaveformLength
    of 0 or less is the whole chunk (a gathered batch has none); ``empty``: what to say of a batch without a chunk."""
    N, L = np.asarray(chunk_samples, dtype=np.int64), np.asarray(wave_lens, dtype=np.int64)
    if N.size == 0:
        raise DeltaRiceError(1, empty)
    if (N == N[0]).all() and (L == L[0]).all():
        ftaps = (len(taps),) + tuple(int(t) & 0xFFFFFFFF for t in taps) if taps else ()
        return ctx.plan_uniform(int(N.size), int(N[0]), (rice_m, int(L[0]) if L[0] > 0 else 0xFFFFFFFF) + ftaps)
    return ctx.plan(N.tolist(), L.tolist(), rice_m, taps)


class Context:
    """One GPU, one HIP stream (a torch stream, so torch events/ordering apply to it)."""

    def __init__(self, device: int | torch.device = 0):
        if not torch.cuda.is_available():
            raise DeltaRiceError(2, "no GPU visible: deltarice_amd has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        self.stream = torch.cuda.Stream(device=self.device)
        h = C.c_void_p()
        st = self.lib.drx_ctx_create(self.device.index or 0, C.c_void_p(self.stream.cuda_stream), C.byref(h))
        if st != _lib.DRX_OK:
            raise DeltaRiceError(st, "drx_ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.drx_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, st: int):
        if st != _lib.DRX_OK:
            raise DeltaRiceError(st, (self.lib.drx_ctx_last_error(self._h) or b"").decode())

    def set_option(self, key: str, value: int):
        self._check(self.lib.drx_ctx_set_option(self._h, key.encode(), int(value)))

    def synchronize(self):
        self._check(self.lib.drx_ctx_synchronize(self._h))

    def plan_uniform(self, n_chunks: int, chunk_samples: int, opts: Sequence[int] = ()) -> "Plan":
        o = parse_opts(opts)
        h = C.c_void_p()
        L = 0 if o.wave_len < 0 else int(o.wave_len)
        self._check(self.lib.drx_plan_create_uniform(self._h, n_chunks, chunk_samples, L, o.rice_k, C.byref(h)))
        plan = Plan(self, h, np.full(n_chunks, chunk_samples, dtype=np.int64), np.full(n_chunks, L, dtype=np.int64))
        plan._rice_m = 1 << o.rice_k
        if not _is_delta(o):  # general prediction filter: GPU FIR/IIR kernels (correct, not tuned)
            plan._taps = plan._apply_filter(o.taps[:o.n_taps])
        return plan

    def plan(self, chunk_samples: Sequence[int], wave_lens: Sequence[int], rice_m: int = 8,
             taps: Optional[Sequence[int]] = None) -> "Plan":
        """Ragged batch: per-chunk sample counts and WaveformLengths (0 or -1: whole chunk); taps: a general
        prediction filter for every chunk (compression_opts[3:] of the reference), None: the delta filter."""
        o = parse_opts((rice_m,))
        n = len(chunk_samples)
        if n == 0 or len(wave_lens) != n:
            raise DeltaRiceError(1, "chunk_samples / wave_lens mismatch")
        cs = (C.c_uint32 * n)(*[int(v) for v in chunk_samples])
        wl = (C.c_uint32 * n)(*[0 if int(v) <= 0 else int(v) for v in wave_lens])
        h = C.c_void_p()
        self._check(self.lib.drx_plan_create(self._h, n, cs, wl, o.rice_k, C.byref(h)))
        plan = Plan(self, h, list(cs), list(wl))
        plan._rice_m = 1 << o.rice_k
        if taps is not None:
            plan._taps = plan._apply_filter(taps)
        return plan

    def filter_chunk(self, data: bytes | np.ndarray, opts: Sequence[int] = (), reverse: bool = False) -> bytes:
        """One chunk through host memory with the H5Z callback's semantics
        (reference src/deltaRice.c:468-490): bytes in, bytes out."""
        raw = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
        out = C.c_void_p()
        nout = C.c_size_t()
        buf = C.create_string_buffer(raw, len(raw))
        self._check(self.lib.drx_filter_chunk_host(self._h, 1 if reverse else 0, len(opts), _cd_values(opts), buf, len(raw),
                                                   C.byref(out), C.byref(nout)))
        res = C.string_at(out.value, nout.value)
        C.CDLL(None).free(C.c_void_p(out.value))
        return res


class Plan:
    """Geometry of one batch (chunks x waveforms), device resident; reusable."""

    def __init__(self, ctx: Context, handle, chunk_samples: Sequence[int] = (), wave_lens: Sequence[int] = ()):
        self.ctx, self._h = ctx, handle
        # the batch's geometry as the plan was made from it (wave_lengths(), decode_select's row stride)
        self._chunk_samples = np.asarray(chunk_samples, dtype=np.int64)
        self._wave_lens = np.asarray(wave_lens, dtype=np.int64)
        self._rice_m, self._taps = 8, None  # (Context.plan / plan_uniform set them: what Gathered.plan() carries over)
        lib = ctx.lib
        self.n_chunks = int(lib.drx_plan_n_chunks(handle))
        self.total_samples = int(lib.drx_plan_total_samples(handle))
        self.total_waves = int(lib.drx_plan_total_waves(handle))
        self.max_encoded_words = int(lib.drx_plan_max_encoded_words(handle))

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx.lib.drx_plan_destroy(self._h)
        self._h = None

    __del__ = close

    def set_filter(self, taps: Optional[Sequence[int]] = None):
        """Another prediction filter for this plan, which may have been used (waits for the context's stream); None or
        (1, -1): the delta filter again.  Gathered.plan() carries over the filter set here."""
        t = self._apply_filter((1, -1) if taps is None else tuple(taps))
        self._taps = None if t == (1, -1) else t

    def _apply_filter(self, taps: Sequence[int]) -> tuple:
        """Sets the plan's prediction filter -> the taps as the library took them (int32), for the plan to remember"""
        arr = (C.c_int32 * max(len(taps), 1))(*[int(v) for v in taps])
        self.ctx._check(self.ctx.lib.drx_plan_set_filter(self._h, len(taps), arr))
        return tuple(int(v) for v in arr[:len(taps)])

    def _dev_check(self, t: torch.Tensor, dtype, n: int, name: str):
        if t.device != self.ctx.device or t.dtype != dtype or not t.is_contiguous() or t.numel() < n:
            raise DeltaRiceError(1, f"{name}: need contiguous {dtype} tensor of >= {n} elements on {self.ctx.device}")

    def _out(self, t: Optional[torch.Tensor], dtype, shape, name: str) -> torch.Tensor:
        """The caller's tensor, or a new one of ``shape`` (a tuple, or a count): contiguous, of ``dtype``, on the plan's device,
        and holding what ``shape`` holds at least"""
        shape = (shape,) if isinstance(shape, int) else shape
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.ctx.device)
        self._dev_check(t, dtype, math.prod(shape), name)
        return t

    def _column(self, t: Optional[torch.Tensor], name: str):
        """(pointer, element stride) of one int64 per waveform: a 1-D tensor of total_waves entries on the plan's device with any
        positive stride (a column of wave_stats() as it is), the stride 1 where there is one waveform at most; None: (NULL, 0)"""
        if t is None:
            return None, 0
        W = self.total_waves
        if (not isinstance(t, torch.Tensor) or t.dim() != 1 or t.device != self.ctx.device or t.dtype != torch.int64 or
                t.shape[0] != W or _stride(t, 0) is None):
            raise DeltaRiceError(1, f"{name}: need a 1-D int64 tensor of {W} entries on {self.ctx.device}")
        return t.data_ptr(), (_stride(t, 0) if W > 1 else 1)

    # What the calls on an encoded batch share: the closed-plan check, the checks of the batch's tensors, the choice between
    # drx_X and drx_X_with_wave_words (the side-band table goes in front of the call's own arguments), and the blocking form.
    def _open(self, who: str):
        if not getattr(self, "_h", None):
            raise DeltaRiceError(1, f"{who}: the plan is closed")

    def _check_encoded(self, words: torch.Tensor, chunk_word_off: torch.Tensor, wave_words: Optional[torch.Tensor]):
        self._dev_check(words, torch.int32, 1, "words")
        self._dev_check(chunk_word_off, torch.int64, self.n_chunks + 1, "chunk_word_off")
        if wave_words is not None:
            self._dev_check(wave_words, torch.int32, self.total_waves, "wave_words")

    def _call_encoded(self, name: str, words, chunk_word_off, wave_words, in_words, *args):
        n = words.numel() if in_words is None else int(in_words)
        if wave_words is None:
            st = getattr(self.ctx.lib, "drx_" + name)(self._h, words.data_ptr(), n, chunk_word_off.data_ptr(), *args)
        else:
            st = getattr(self.ctx.lib, f"drx_{name}_with_wave_words")(self._h, words.data_ptr(), n, chunk_word_off.data_ptr(),
                                                                      wave_words.data_ptr(), *args)
        self.ctx._check(st)

    def _blocking(self, launch, enc: "EncodedBatch", *args, **kw):
        """launch -- an *_async entry -- on the batch ``enc`` behind the caller's stream, and finish()"""
        self._open(launch.__name__.removesuffix("_async"))
        self.ctx.stream.wait_stream(torch.cuda.current_stream(self.ctx.device))
        r = launch(enc.words, enc.chunk_word_off, *args, in_words=enc.total_words, **kw)
        self.finish()
        return r

    def _batch_call(self, name: str, words, chunk_word_off, wave_words, in_words, own: tuple, out_words, out_chunk_word_off,
                    n_out_chunks: int, out_wave_words, n_out_waves: int):
        """The calls that write a new encoded batch, drx_<name>(the batch, *own, d_out, out_cap_words, d_out_chunk_word_off,
        d_out_wave_words): out_words None or empty is the sizing call (NULL, 0); the two tables are the caller's or new ones."""
        self._check_encoded(words, chunk_word_off, wave_words)
        if out_words is not None:
            self._dev_check(out_words, torch.int32, 0, "out_words")
        off = self._out(out_chunk_word_off, torch.int64, n_out_chunks + 1, "out_chunk_word_off")
        tab = self._out(out_wave_words, torch.int32, n_out_waves, "out_wave_words")
        op, cap = (out_words.data_ptr(), out_words.numel()) if out_words is not None and out_words.numel() else (None, 0)
        self._call_encoded(name, words, chunk_word_off, wave_words, in_words, *own, op, cap, off.data_ptr(),
                           tab.data_ptr() if n_out_waves else None)
        return out_words, off, tab

    def _sized(self, launch, enc: "EncodedBatch", own: tuple, wave_words, out_words):
        """launch -- gather_encoded_async, transcode_async or refilter_async, ``own`` its arguments in front of out_words -- into
        the caller's out_words, or into an exact one: a sizing call, finish() for the words needed, and the call again, which
        resumes from the first one's tables, all behind the caller's stream -> (EncodedBatch, out_wave_words)"""
        self.ctx.stream.wait_stream(torch.cuda.current_stream(self.ctx.device))
        off = tab = None
        if out_words is None:
            _, off, tab = launch(enc.words, enc.chunk_word_off, *own, None, enc.total_words, wave_words)
            out_words = torch.empty(self.finish(), dtype=torch.int32, device=self.ctx.device)
        _, off, tab = launch(enc.words, enc.chunk_word_off, *own, out_words, enc.total_words, wave_words, off, tab)
        return EncodedBatch(out_words, off, self.finish()), tab

    def encode_async(self, x: torch.Tensor, out_words: Optional[torch.Tensor] = None,
                     chunk_word_off: Optional[torch.Tensor] = None, capacity_words: Optional[int] = None):
        """Launches the encode on the context's stream; no host sync."""
        self._open("encode")
        self._dev_check(x, torch.int16, self.total_samples, "x")
        if out_words is None:
            cap = self.max_encoded_words if capacity_words is None else int(capacity_words)
            out_words = torch.empty(cap, dtype=torch.int32, device=self.ctx.device)
        chunk_word_off = self._out(chunk_word_off, torch.int64, self.n_chunks + 1, "chunk_word_off")
        self.ctx._check(self.ctx.lib.drx_encode(self._h, x.data_ptr(), out_words.data_ptr(), out_words.numel(),
                                                chunk_word_off.data_ptr()))
        return out_words, chunk_word_off

    def finish(self) -> int:
        """Waits for the last call on this plan and raises on device-side errors
        (capacity, corrupt input); returns the encoded word count of the last encode."""
        n = C.c_uint64()
        self.ctx._check(self.ctx.lib.drx_plan_finish(self._h, C.byref(n)))
        return int(n.value)

    def encode(self, x: torch.Tensor, capacity_words: Optional[int] = None) -> EncodedBatch:
        cur = torch.cuda.current_stream(self.ctx.device)
        self.ctx.stream.wait_stream(cur)
        words, off = self.encode_async(x, capacity_words=capacity_words)
        total = self.finish()
        return EncodedBatch(words, off, total)

    def decode_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, out: Optional[torch.Tensor] = None,
                     in_words: Optional[int] = None):
        self._open("decode")
        return self._decode(words, chunk_word_off, None, out, in_words)

    def _decode(self, words, chunk_word_off, wave_words, out, in_words):
        self._check_encoded(words, chunk_word_off, wave_words)
        out = self._out(out, torch.int16, self.total_samples, "out")
        self._call_encoded("decode", words, chunk_word_off, wave_words, in_words, out.data_ptr())
        return out

    def decode_with_wave_words(self, words: torch.Tensor, chunk_word_off: torch.Tensor, wave_words: torch.Tensor,
                               out: Optional[torch.Tensor] = None, in_words: Optional[int] = None) -> torch.Tensor:
        """Decode with the encoder's n_i table as a side-band (int32 tensor [total_waves] on the device): no header walk.
        Launch only; finish() raises DRX_ERR_CORRUPT if the table does not belong to the stream."""
        self._open("decode_with_wave_words")
        self._dev_check(wave_words, torch.int32, self.total_waves, "wave_words")  # (this form has no walk to fall back to)
        return self._decode(words, chunk_word_off, wave_words, out, in_words)

    def wave_words_device(self) -> torch.Tensor:
        """A device copy of n_i of every waveform from the last encode/decode (the side-band of decode_with_wave_words)."""
        return torch.from_numpy(self.wave_words().view(np.int32)).to(self.ctx.device)

    def decode(self, enc: EncodedBatch, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._blocking(self.decode_async, enc, out)

    def wave_lengths(self, wave_idx) -> np.ndarray:
        """len_i of the waveforms ``wave_idx`` names: WaveformLength, or less for the last waveform of a chunk."""
        return wave_lengths(self._chunk_samples, self._wave_lens, wave_idx)

    def longest_wave(self) -> int:
        """The longest waveform of the plan (the row stride decode_select allocates)."""
        L = np.where(self._wave_lens <= 0, self._chunk_samples, self._wave_lens)
        return int(np.minimum(L, self._chunk_samples).max())

    def decode_select_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, wave_idx,
                            out: Optional[torch.Tensor] = None, in_words: Optional[int] = None,
                            wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decodes the waveforms ``wave_idx`` names (global indices; any order, duplicates allowed; any integer sequence,
        numpy array or CPU tensor) and no others: row i of the result holds waveform wave_idx[i].  Only the chunks those
        waveforms lie in are read and validated.  out: int16 [n_sel, stride] with contiguous rows, of which exactly len_i
        samples per row are written; None: a new tensor whose stride is the plan's longest waveform, zero behind a shorter
        one.  wave_words: the encoder's n_i table as decode_with_wave_words takes it (no header walk).
        Launch only; finish() raises on device-side errors."""
        self._open("decode_select")
        idx = _as_index_array(wave_idx)
        n_sel = int(idx.size)
        self._check_encoded(words, chunk_word_off, wave_words)
        if out is None:
            out = torch.zeros((n_sel, self.longest_wave()), dtype=torch.int16, device=self.ctx.device)
            self.ctx.stream.wait_stream(torch.cuda.current_stream(self.ctx.device))  # (the zero fill)
        if (out.dim() != 2 or out.device != self.ctx.device or out.dtype != torch.int16 or out.shape[0] < n_sel or
                (out.shape[1] > 1 and out.stride(1) != 1) or (out.shape[0] > 1 and out.stride(0) < out.shape[1])):
            raise DeltaRiceError(1, f"out: need an int16 [>= {n_sel}, stride] tensor with contiguous rows on {self.ctx.device}")
        stride = int(out.stride(0)) if out.shape[0] > 1 else int(out.shape[1])
        # (rows of the plan's longest waveform hold any selection; shorter ones are checked against this one)
        if n_sel and out.shape[1] < self.longest_wave() and int(self.wave_lengths(idx).max()) > out.shape[1]:
            raise DeltaRiceError(1, f"out: rows of {out.shape[1]} samples are shorter than the longest selected waveform")
        self._call_encoded("decode_select", words, chunk_word_off, wave_words, in_words,
                           idx.ctypes.data_as(C.POINTER(C.c_uint64)), n_sel, out.data_ptr(), stride)
        return out

    def decode_select(self, enc: EncodedBatch, wave_idx, out: Optional[torch.Tensor] = None,
                      wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """decode_select_async on an EncodedBatch; waits, and raises like decode()."""
        return self._blocking(self.decode_select_async, enc, wave_idx, out, wave_words=wave_words)

    def gather_encoded_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, wave_idx, chunk_waves: int,
                             out_words: Optional[torch.Tensor] = None, in_words: Optional[int] = None,
                             wave_words: Optional[torch.Tensor] = None, out_chunk_word_off: Optional[torch.Tensor] = None,
                             out_wave_words: Optional[torch.Tensor] = None):
        """Launches drx_gather_encoded on the context's stream: the waveforms ``wave_idx`` names (as decode_select takes
        them), ``chunk_waves`` to an output chunk, copied -- not decoded -- into ``out_words`` (int32, its numel the capacity).
        out_words None: the SIZING call, which writes the two tables only; finish() then returns the words needed.
        -> (out_words, out_chunk_word_off int64 [n_out_chunks + 1], out_wave_words int32 [n_sel]).  finish() raises on
        device-side errors (DRX_ERR_CAPACITY: nothing was written; DRX_ERR_CORRUPT: a touched chunk failed validation)."""
        self._open("gather_encoded")
        idx = _as_index_array(wave_idx)
        n_sel, cw = int(idx.size), int(chunk_waves)
        n_out = -(-n_sel // cw) if cw > 0 else 0
        return self._batch_call("gather_encoded", words, chunk_word_off, wave_words, in_words,
                                (idx.ctypes.data_as(C.POINTER(C.c_uint64)), n_sel, cw), out_words, out_chunk_word_off, n_out,
                                out_wave_words, n_sel)

    def gather_encoded(self, enc: EncodedBatch, wave_idx, chunk_waves: int, wave_words: Optional[torch.Tensor] = None,
                       out_words: Optional[torch.Tensor] = None) -> Gathered:
        """A new encoded batch of the waveforms ``wave_idx`` names (any order, duplicates allowed), ``chunk_waves`` to a chunk,
        without decoding them: byte for byte what encode() gives for the gathered samples under this plan's RiceParameter and
        filter.  Every output chunk needs one WaveformLength (gather_geometry()).  out_words None: sized by a first call and
        allocated exactly (the second call resumes from the first one's tables: one walk, one scan); otherwise
        DRX_ERR_CAPACITY if the result does not fit it.  Waits, and raises like decode()."""
        idx = _as_index_array(wave_idx)
        N, L = gather_geometry(self._chunk_samples, self._wave_lens, idx, chunk_waves)
        if idx.size == 0:
            off = torch.zeros(1, dtype=torch.int64, device=self.ctx.device)
            tab = torch.empty(0, dtype=torch.int32, device=self.ctx.device)
            out_words = torch.empty(0, dtype=torch.int32, device=self.ctx.device) if out_words is None else out_words
            return Gathered(EncodedBatch(out_words, off, 0), N, L, tab, self._rice_m, self._taps)
        res, tab = self._sized(self.gather_encoded_async, enc, (idx, chunk_waves), wave_words, out_words)
        return Gathered(res, N, L, tab, self._rice_m, self._taps)

    def wave_stats_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, head: int = 0,
                         out: Optional[torch.Tensor] = None, wave_words: Optional[torch.Tensor] = None,
                         in_words: Optional[int] = None) -> torch.Tensor:
        """Launches drx_wave_stats on the context's stream: int64 [total_waves, STAT_COLS], row g = (min, argmin, max, argmax,
        sum, sum of squares, head sum, head sum of squares) of waveform g over the int16 samples decode() would give, exact;
        first occurrences; ``head``: the window of the last two columns, the first min(head, len) samples.  Nothing is decoded
        to memory.  wave_words: the encoder's n_i table as decode_with_wave_words takes it (no header walk).
        Launch only; finish() raises on device-side errors."""
        self._open("wave_stats")
        head = _uint32(head, "head")
        self._check_encoded(words, chunk_word_off, wave_words)
        out = self._out(out, torch.int64, (self.total_waves, _lib.STAT_COLS), "out")
        self._call_encoded("wave_stats", words, chunk_word_off, wave_words, in_words, head, out.data_ptr())
        return out

    def wave_stats(self, enc: EncodedBatch, head: int = 0, out: Optional[torch.Tensor] = None,
                   wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wave_stats_async on an EncodedBatch; waits, and raises like decode().  The cuts of an analysis come from its
        columns: ``plan.gather_encoded(enc, torch.nonzero(cut(stats)).flatten().cpu(), 2000)``."""
        return self._blocking(self.wave_stats_async, enc, head, out, wave_words)

    def wave_bins_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, bin: int, n_bins: Optional[int] = None,
                        start: Optional[torch.Tensor] = None, offset: int = 0, out: Optional[torch.Tensor] = None,
                        wave_words: Optional[torch.Tensor] = None, in_words: Optional[int] = None) -> torch.Tensor:
        """Launches drx_wave_bins on the context's stream: int64 [total_waves, n_bins, BIN_COLS], row (g, b) = (sum, sum of
        squares, min, max) of the samples of waveform g with index in [a + b * bin, a + (b + 1) * bin), a = start[g] + offset,
        over the int16 samples decode() would give, exact.  A bin that holds no sample is (0, 0, 32767, -32768), so neighbouring
        bins merge by add, add, min, max.  Nothing is decoded to memory.  n_bins None: enough bins to cover the plan's longest
        waveform from ``offset``.  start: None, or a 1-D int64 tensor of total_waves entries on the plan's device with any
        element stride -- ``stats[:, STAT_ARGMAX]`` is passed as it is, as decode_window takes it.  out: a contiguous int64
        tensor of total_waves * n_bins * BIN_COLS elements.  wave_words: the encoder's n_i table as decode_with_wave_words
        takes it (no header walk).  Launch only; finish() raises on device-side errors."""
        self._open("wave_bins")
        bin, offset = _uint32(bin, "bin", 1), _int64(offset, "offset")
        n_bins = _uint32(max(0, -(-(self.longest_wave() - offset) // bin)) if n_bins is None else n_bins, "n_bins")
        sp, ss = self._column(start, "start")
        self._check_encoded(words, chunk_word_off, wave_words)
        out = self._out(out, torch.int64, (self.total_waves, n_bins, _lib.BIN_COLS), "out")
        if n_bins == 0 or self.total_waves == 0:
            return out
        self._call_encoded("wave_bins", words, chunk_word_off, wave_words, in_words, sp, ss, offset, bin, n_bins, out.data_ptr(),
                           n_bins * _lib.BIN_COLS)
        return out

    def wave_bins(self, enc: EncodedBatch, bin: int, n_bins: Optional[int] = None, start: Optional[torch.Tensor] = None,
                  offset: int = 0, out: Optional[torch.Tensor] = None, wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wave_bins_async on an EncodedBatch -> int64 [total_waves, n_bins, BIN_COLS]; waits, and raises like wave_stats().  The
        charge in eight gates of 250 samples around every waveform's peak:
        ``plan.wave_bins(enc, 250, 8, start=stats[:, STAT_ARGMAX], offset=-500)[:, :, BIN_SUM]``.  Few long waveforms (the
        reference's default of one waveform per chunk) are much faster by the block form, which the context option takes:
        ``ctx.set_option("bins_impl", 1)``; the rows are the same, last_bins_form() says which form ran."""
        return self._blocking(self.wave_bins_async, enc, bin, n_bins, start, offset, out, wave_words)

    def wave_stack_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, width: Optional[int] = None,
                         start: Optional[torch.Tensor] = None, offset: int = 0, select: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None, wave_words: Optional[torch.Tensor] = None,
                         in_words: Optional[int] = None) -> torch.Tensor:
        """Launches drx_wave_stack on the context's stream: int64 [width, STACK_COLS], row j = (how many, their sum, the sum of
        their squares) over the samples ``start[g] + offset + j`` of the selected waveforms g that have one, over the int16
        samples decode() would give, exact; a position nobody reaches is (0, 0, 0), and results of several batches add.
        Nothing is decoded to memory and a waveform is read no further than its window's end.  width None: the positions that
        some waveform of the plan reaches from ``offset`` with origins 0 (wave_bins' default n_bins at bin 1).  start: as
        wave_bins takes it -- ``stats[:, STAT_ARGMAX]`` is passed as it is.  select: None (every waveform), or a bool or uint8
        tensor of total_waves entries on the plan's device (nonzero: selected); a waveform that is not selected is not read.
        out: a contiguous int64 tensor of width * STACK_COLS elements.  wave_words: the encoder's n_i table as
        decode_with_wave_words takes it (no header walk).  Launch only; finish() raises on device-side errors."""
        self._open("wave_stack")
        offset = _int64(offset, "offset")
        width = _uint32(max(0, self.longest_wave() - offset) if width is None else width, "width")
        sp, ss = self._column(start, "start")
        if select is not None:
            if not isinstance(select, torch.Tensor) or select.dim() != 1 or select.dtype not in (torch.bool, torch.uint8):
                raise DeltaRiceError(1, f"select: need a 1-D bool or uint8 tensor of {self.total_waves} entries on {self.ctx.device}")
            self._dev_check(select, select.dtype, self.total_waves, "select")
        self._check_encoded(words, chunk_word_off, wave_words)
        out = self._out(out, torch.int64, (width, _lib.STACK_COLS), "out")
        if width == 0:
            return out
        if self.total_waves == 0:
            with torch.cuda.stream(self.ctx.stream):
                out.view(-1)[:width * _lib.STACK_COLS].zero_()  # (no waveform: the rows nobody reaches)
            return out
        self._call_encoded("wave_stack", words, chunk_word_off, wave_words, in_words, sp, ss, offset, width,
                           select.data_ptr() if select is not None else None, out.data_ptr(), _lib.STACK_COLS)
        return out

    def wave_stack(self, enc: EncodedBatch, width: Optional[int] = None, start: Optional[torch.Tensor] = None, offset: int = 0,
                   select: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wave_stack_async on an EncodedBatch -> int64 [width, STACK_COLS]; waits, and raises like wave_stats().  The average
        pulse of the waveforms that passed a cut, aligned on the maximum, and its variance:
        ``r = plan.wave_stack(enc, 512, start=stats[:, STAT_ARGMAX], offset=-64, select=cut(stats))``, then
        ``mean = r[:, STACK_SUM] / r[:, STACK_COUNT]``.  General prediction filters and few long waveforms are correct and slow."""
        return self._blocking(self.wave_stack_async, enc, width, start, offset, select, out, wave_words)

    def decode_window_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, start, width: int, offset: int = 0,
                            pad: int = 0, out: Optional[torch.Tensor] = None, out_stride: Optional[int] = None,
                            wave_words: Optional[torch.Tensor] = None, in_words: Optional[int] = None) -> torch.Tensor:
        """Launches drx_decode_window on the context's stream: int16 [total_waves, width], row g = the ``width`` samples of
        waveform g from sample ``start[g] + offset`` on, ``pad`` where that leaves the waveform.  A payload is read no further
        than its window's end and the batch is not decoded to memory.  start: None, an int (folded into offset), or a 1-D
        int64 tensor of total_waves entries on the plan's device with any element stride -- ``stats[:, STAT_ARGMAX]`` is
        passed as it is.  out: an int16 tensor that holds (total_waves - 1) * out_stride + width samples (out_stride: samples
        between rows, default width); the samples between rows keep what they held.  wave_words: the encoder's n_i table as
        decode_with_wave_words takes it (no header walk).  Launch only; finish() raises on device-side errors."""
        self._open("decode_window")
        width, pad = _uint32(width, "width"), _int16(pad, "pad")
        if start is not None and not isinstance(start, torch.Tensor):
            start, offset = None, int(offset) + int(start)
        sp, ss = self._column(start, "start")
        offset = _int64(offset, "offset")
        self._check_encoded(words, chunk_word_off, wave_words)
        stride = width if out_stride is None else int(out_stride)
        if stride < width:
            raise DeltaRiceError(1, f"out_stride: rows {stride} samples apart do not hold {width}")
        need = (self.total_waves - 1) * stride + width if self.total_waves else 0
        out = self._out(out, torch.int16, (self.total_waves, width) if stride == width else need, "out")
        if width == 0 or self.total_waves == 0:
            return out
        self._call_encoded("decode_window", words, chunk_word_off, wave_words, in_words, sp, ss, offset, width, pad, out.data_ptr(),
                           stride)
        return out

    def decode_window(self, enc: EncodedBatch, start, width: int, offset: int = 0, pad: int = 0,
                      out: Optional[torch.Tensor] = None, wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """decode_window_async on an EncodedBatch -> int16 [total_waves, width]; waits, and raises like decode().  The samples
        around every pulse: ``plan.decode_window(enc, stats[:, STAT_ARGMAX], 256, offset=-64)``."""
        return self._blocking(self.decode_window_async, enc, start, width, offset, pad, out, None, wave_words)

    def decode_windows_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, start: torch.Tensor, width: int,
                             count: Optional[torch.Tensor] = None, offset: int = 0, pad: int = 0,
                             out: Optional[torch.Tensor] = None, out_strides: Optional[tuple] = None,
                             wave_words: Optional[torch.Tensor] = None, in_words: Optional[int] = None) -> torch.Tensor:
        """Launches drx_decode_windows on the context's stream: int16 [total_waves, n_win, width], row (g, p) = the ``width``
        samples of waveform g from sample ``start[g, p] + offset`` on, ``pad`` where that leaves the waveform -- and all over
        the row where p >= min(count[g], n_win).  A payload is read no further than its last window's end and the batch is not
        decoded to memory.  start: a 2-D int64 tensor [total_waves, n_win] on the plan's device with any positive element
        strides -- ``pulses[:, :, PULSE_START]`` of find_pulses() is passed as it is, with its ``count``.  count: an int32
        tensor of total_waves entries, or None (every slot is live).  Windows may come in any order and overlap; non-decreasing
        starts are the fast case.  out: an int16 tensor that holds the rows at out_strides = (samples between waveforms, samples
        between a waveform's rows), default (n_win * width, width); the samples between rows keep what they held.  wave_words:
        the encoder's n_i table as decode_with_wave_words takes it (no header walk).  Launch only; finish() raises on
        device-side errors."""
        self._open("decode_windows")
        width, offset, pad = _uint32(width, "width"), _int64(offset, "offset"), _int16(pad, "pad")
        W = self.total_waves
        if (not isinstance(start, torch.Tensor) or start.dim() != 2 or start.device != self.ctx.device or
                start.dtype != torch.int64 or start.shape[0] != W or not start.shape[1] < 1 << 32 or
                _stride(start, 0) is None or _stride(start, 1) is None):
            raise DeltaRiceError(1, f"start: need a 2-D int64 tensor [{W}, n_win] with positive strides on {self.ctx.device}")
        K, s_wave, s_win = int(start.shape[1]), _stride(start, 0), _stride(start, 1)
        if count is not None:
            self._dev_check(count, torch.int32, W, "count")
        self._check_encoded(words, chunk_word_off, wave_words)
        o_wave, o_win = (K * width, width) if out_strides is None else (int(out_strides[0]), int(out_strides[1]))
        if o_win < width:
            raise DeltaRiceError(1, f"out_strides: rows {o_win} samples apart do not hold {width}")
        if K and o_wave < (K - 1) * o_win + width:
            raise DeltaRiceError(1, f"out_strides: waveforms {o_wave} samples apart do not hold {K} rows {o_win} apart")
        need = (W - 1) * o_wave + (K - 1) * o_win + width if W and K and width else 0
        out = self._out(out, torch.int16, need, "out")
        rows =out.view(-1).as_strided((W, K, width), (o_wave, o_win, 1)) if need else out.view(-1)[:0].view(W, K, width)
        if need == 0:
            return rows
        self._call_encoded("decode_windows", words, chunk_word_off, wave_words, in_words, start.data_ptr(), s_wave, s_win,
                           count.data_ptr() if count is not None else None, K, offset, width, pad, out.data_ptr(), o_wave, o_win)
        return rows

    def decode_windows(self, enc: EncodedBatch, start: torch.Tensor, width: int, count: Optional[torch.Tensor] = None,
                       offset: int = 0, pad: int = 0, out: Optional[torch.Tensor] = None,
                       wave_words: Optional[torch.Tensor] = None) -> torch.Tensor:
        """decode_windows_async on an EncodedBatch -> int16 [total_waves, n_win, width]; waits, and raises like decode().  The
        samples around every pulse: ``n, pulses = plan.find_pulses(enc, thr, max_pulses=8)``, then
        ``plan.decode_windows(enc, pulses[:, :, PULSE_START], 256, count=n, offset=-64)``."""
        return self._blocking(self.decode_windows_async, enc, start, width, count, offset, pad, out, None, wave_words)

    def find_pulses_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, threshold, polarity: int = 1,
                          min_width: int = 1, max_pulses: int = 4, offset: int = 0, count: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None, wave_words: Optional[torch.Tensor] = None,
                          in_words: Optional[int] = None):
        """Launches drx_find_pulses on the context's stream -> (count, pulses): int32 [total_waves], the number of pulses of
        every waveform (all of them, those beyond max_pulses included), and int64 [total_waves, max_pulses, PULSE_COLS], row g
        slot p = (start, width, peak, argpeak, sum) of pulse p of waveform g, zero beyond its last pulse.  A pulse is a maximal
        run of at least ``min_width`` consecutive samples above (polarity > 0) or below (polarity < 0) ``threshold[g] + offset``,
        strictly, over the int16 samples decode() would give; exact; nothing is decoded to memory.  threshold: an int (folded
        into offset), or a 1-D int64 tensor of total_waves entries on the plan's device with any positive element stride -- a
        column of wave_stats() or an expression over it is passed as it is.  max_pulses 0: the counting form, pulses is empty.
        count / out: an int32 tensor of total_waves and an int64 tensor of total_waves * max_pulses * PULSE_COLS elements to
        write to.  wave_words: the encoder's n_i table as decode_with_wave_words takes it (no header walk).  Launch only;
        finish() raises on device-side errors."""
        self._open("find_pulses")
        polarity = int(polarity)
        if polarity == 0:
            raise DeltaRiceError(1, "polarity: 0 is neither above nor below")
        min_width, max_pulses = _uint32(min_width, "min_width", 1), _uint32(max_pulses, "max_pulses")
        if not isinstance(threshold, torch.Tensor):
            threshold, offset = None, int(offset) + int(threshold)
        tp, ts = self._column(threshold, "threshold")
        offset = _int64(offset, "offset")
        self._check_encoded(words, chunk_word_off, wave_words)
        W, need = self.total_waves, self.total_waves * max_pulses * _lib.PULSE_COLS
        count = self._out(count, torch.int32, W, "count")
        out = self._out(out, torch.int64, need, "out")
        self._call_encoded("find_pulses", words, chunk_word_off, wave_words, in_words, tp, ts, offset, 1 if polarity > 0 else -1,
                           min_width, max_pulses, count.data_ptr(), out.data_ptr() if need else None)
        return count.view(-1)[:W], out.view(-1)[:need].view(W, max_pulses, _lib.PULSE_COLS)

    def find_pulses(self, enc: EncodedBatch, threshold, polarity: int = 1, min_width: int = 1, max_pulses: int = 4,
                    offset: int = 0, count: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    wave_words: Optional[torch.Tensor] = None):
        """find_pulses_async on an EncodedBatch -> (count, pulses); waits, and raises like decode().  Forty counts above every
        waveform's own baseline: ``plan.find_pulses(enc, stats[:, STAT_HEAD_SUM] // 500, offset=40)``."""
        return self._blocking(self.find_pulses_async, enc, threshold, polarity, min_width, max_pulses, offset, count, out, wave_words)

    def estimate_words_encoded(self, enc: EncodedBatch, wave_words: Optional[torch.Tensor] = None) -> np.ndarray:
        """estimate_words from the encoded stream: entry k is the total words transcode() gives at RiceParameter 2^k, k = 0..15;
        nothing is decoded to memory.  wave_words: the source's n_i table (no header walk).  Waits; raises DRX_ERR_CORRUPT for a
        stream that fails validation."""
        self._open("estimate_words_encoded")
        return self._estimate("drx_estimate_words_encoded", enc, wave_words)

    def _estimate(self, symbol: str, enc: EncodedBatch, wave_words, *target):
        """The sixteen totals of drx_estimate_words_encoded, or of its _filter form with the ``target`` taps (n, array)"""
        self._check_encoded(enc.words, enc.chunk_word_off, wave_words)
        self.ctx.stream.wait_stream(torch.cuda.current_stream(self.ctx.device))
        out = (C.c_uint64 * 16)()
        self.ctx._check(getattr(self.ctx.lib, symbol)(self._h, enc.words.data_ptr(), int(enc.total_words), enc.chunk_word_off.data_ptr(),
                                                      wave_words.data_ptr() if wave_words is not None else None, *target, out))
        return np.array(list(out), dtype=np.uint64)

    def transcode_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, rice_m: int,
                        out_words: Optional[torch.Tensor] = None, in_words: Optional[int] = None,
                        wave_words: Optional[torch.Tensor] = None, out_chunk_word_off: Optional[torch.Tensor] = None,
                        out_wave_words: Optional[torch.Tensor] = None):
        """Launches drx_transcode on the context's stream: the batch re-coded -- not decoded -- at RiceParameter ``rice_m`` into
        ``out_words`` (int32, its numel the capacity).  out_words None: the SIZING call, which writes the two tables only;
        finish() then returns the words needed.  -> (out_words, out_chunk_word_off int64 [n_chunks + 1], out_wave_words int32
        [total_waves]).  finish() raises on device-side errors (DRX_ERR_CAPACITY, DRX_ERR_CORRUPT: nothing was written)."""
        self._open("transcode")
        k = parse_opts((int(rice_m),)).rice_k
        return self._batch_call("transcode", words, chunk_word_off, wave_words, in_words, (k,), out_words, out_chunk_word_off,
                                self.n_chunks, out_wave_words, self.total_waves)

    def transcode(self, enc: EncodedBatch, rice_m: Optional[int] = None, wave_words: Optional[torch.Tensor] = None,
                  out_words: Optional[torch.Tensor] = None) -> "Transcoded":
        """The batch re-coded at RiceParameter ``rice_m`` without decoding it: for a filter with lead +-1 byte for byte what
        encode() gives for the decoded samples at that parameter, for every filter a stream that decodes to the same samples.
        rice_m None: the parameter of the smallest total of estimate_words_encoded() (on a tie the smaller).  out_words None:
        sized by a first call and allocated exactly -- that costs a second sizes pass, so a caller that has a bound (the
        plan's max_encoded_words bounds any result) should pass out_words; otherwise DRX_ERR_CAPACITY if the result does not
        fit it.  Waits, and raises like decode()."""
        self._open("transcode")
        if rice_m is None:
            rice_m = 1 << int(np.argmin(self.estimate_words_encoded(enc, wave_words)))  # (argmin: the first of equals)
        res, tab = self._sized(self.transcode_async, enc, (rice_m,), wave_words, out_words)
        return Transcoded(res, tab, int(rice_m), self._taps, self._chunk_samples.copy(), self._wave_lens.copy())

    @staticmethod
    def _target_taps(taps: Optional[Sequence[int]]):
        """(ctypes int32 array, its length, the taps as Transcoded carries them: None for (1, -1)) of a target filter"""
        t = (1, -1) if taps is None else tuple(int(v) for v in taps)
        if not 1 <= len(t) <= _lib.DRX_MAX_TAPS:
            raise DeltaRiceError(1, f"taps: {len(t)} values (1 .. {_lib.DRX_MAX_TAPS})")
        if any(not -(1 << 31) <= v < 1 << 31 for v in t):
            raise DeltaRiceError(1, "taps: a value is not an int32")
        return (C.c_int32 * len(t))(*t), len(t), (None if t == (1, -1) else t)

    def estimate_words_refiltered(self, enc: EncodedBatch, taps: Optional[Sequence[int]],
                                  wave_words: Optional[torch.Tensor] = None) -> np.ndarray:
        """estimate_words_encoded under ANOTHER prediction filter: entry k is the total words refilter() gives with ``taps`` at
        RiceParameter 2^k, k = 0..15 -- what estimate_words(x) of a plan with that filter gives for the decoded samples x, with
        nothing decoded to memory.  Waits; raises DRX_ERR_CORRUPT for a stream that fails validation."""
        self._open("estimate_words_refiltered")
        arr, n, _ = self._target_taps(taps)
        return self._estimate("drx_estimate_words_encoded_filter", enc, wave_words, n, arr)

    def refilter_async(self, words: torch.Tensor, chunk_word_off: torch.Tensor, taps: Optional[Sequence[int]], rice_m: int,
                       out_words: Optional[torch.Tensor] = None, in_words: Optional[int] = None,
                       wave_words: Optional[torch.Tensor] = None, out_chunk_word_off: Optional[torch.Tensor] = None,
                       out_wave_words: Optional[torch.Tensor] = None):
        """Launches drx_transcode_filter on the context's stream: transcode_async with a change of prediction filter -- the
        batch re-coded under ``taps`` (None or (1, -1): the delta filter) at RiceParameter ``rice_m``, not decoded to memory.
        The plan's own filter and RiceParameter describe the source and stay.  Arguments, the sizing call, the result and
        finish() as transcode_async."""
        self._open("refilter")
        k = parse_opts((int(rice_m),)).rice_k
        arr, n, _ = self._target_taps(taps)
        return self._batch_call("transcode_filter", words, chunk_word_off, wave_words, in_words, (k, n, arr), out_words,
                                out_chunk_word_off, self.n_chunks, out_wave_words, self.total_waves)

    def refilter(self, enc: EncodedBatch, taps: Optional[Sequence[int]], rice_m: Optional[int] = None,
                 wave_words: Optional[torch.Tensor] = None, out_words: Optional[torch.Tensor] = None) -> "Transcoded":
        """The batch re-coded under the prediction filter ``taps`` at RiceParameter ``rice_m`` without decoding it to memory:
        byte for byte what a plan with that filter and parameter encodes from decode(enc).  rice_m None: the parameter of the
        smallest total of estimate_words_refiltered() (on a tie the smaller).  out_words as in transcode().  The result's
        ``taps`` are the target's (None for (1, -1)), so ``result.plan(ctx)`` decodes it.  Waits, and raises like decode().
        Always a lane per waveform, also for the few long waveforms transcode() gives to its block form.  It is SLOWER than
        decode(), set_filter(), encode(), set_filter() back -- 21.2 against 13.4 ms on 1 M waveforms of 7000 samples
        (profiles/refilter_notes.md) -- and saves the decoded intermediate: 7.4 instead of 21.4 GB of peak device memory there."""
        self._open("refilter")
        _, _, carried = self._target_taps(taps)
        if rice_m is None:
            rice_m = 1 << int(np.argmin(self.estimate_words_refiltered(enc, taps, wave_words)))  # (argmin: the first of equals)
        res, tab = self._sized(self.refilter_async, enc, (taps, rice_m), wave_words, out_words)
        return Transcoded(res, tab, int(rice_m), carried, self._chunk_samples.copy(), self._wave_lens.copy())

    def estimate_words(self, x: torch.Tensor) -> np.ndarray:
        """Exact encoded size (uint32 words) of this batch for RiceParameter 2^k, k = 0..15 -- the
        optimisation the reference's docs/Optimization.md describes; argmin gives the best m."""
        self._dev_check(x, torch.int16, self.total_samples, "x")
        cur = torch.cuda.current_stream(self.ctx.device)
        self.ctx.stream.wait_stream(cur)
        out = (C.c_uint64 * 16)()
        self.ctx._check(self.ctx.lib.drx_estimate_words(self._h, x.data_ptr(), out))
        return np.array(list(out), dtype=np.uint64)

    def last_timings(self):
        """Kernel times (ms) of the last call, HIP events on the context's stream; needs
        ctx.set_option("profile", 1).  encode: (sizes, scan, pack, total); decode, wave_stats, decode_window and find_pulses: (walk, kernel, 0, total);
        transcode and refilter: (walk, sizes + scan + offsets, pack, total)."""
        ms = (C.c_float * 4)()
        self.ctx._check(self.ctx.lib.drx_plan_last_timings(self._h, ms))
        return tuple(float(v) for v in ms)

    def last_decode_path(self) -> int:
        """DRX_PATH_* bits (include/deltarice_hip.h) of the decoders the last decode used."""
        return int(self.ctx.lib.drx_plan_last_decode_path(self._h))

    def last_stats_form(self) -> int:
        """DRX_STATS_FORM_* (include/deltarice_hip.h): which form the last wave_stats took -- a lane per waveform, or a workgroup
        per block of a waveform's stream (few long waveforms); 0 before the plan's first statistics call."""
        return int(self.ctx.lib.drx_plan_last_stats_form(self._h))

    def last_pulses_form(self) -> int:
        """DRX_PULSES_FORM_* (include/deltarice_hip.h): which form the last find_pulses took -- a lane per waveform, or a
        workgroup per block of a waveform's stream with the runs stitched behind it (few long waveforms); 0 before the plan's
        first pulse call."""
        return int(self.ctx.lib.drx_plan_last_pulses_form(self._h))

    def last_windows_form(self) -> int:
        """DRX_WINDOWS_FORM_* (include/deltarice_hip.h): which form the last decode_windows took -- a lane per waveform, or a
        workgroup per block of a waveform's stream (few long waveforms); 0 before the plan's first such call."""
        return int(self.ctx.lib.drx_plan_last_windows_form(self._h))

    def last_windows_listed(self) -> int:
        """After finish(): how many waveforms the last decode_windows' block form handed to the lane kernel behind it (flagged or
        judged suspect by the block parse; their rows are written again and judged there); 0 for the lane form."""
        return int(self.ctx.lib.drx_plan_last_windows_listed(self._h))

    def last_bins_form(self) -> int:
        """DRX_BINS_FORM_* (include/deltarice_hip.h): which form the last wave_bins took -- a lane per waveform (every batch under
        the context's default ``bins_impl`` 0), or under ``ctx.set_option("bins_impl", 1)`` a workgroup per block of a waveform's
        stream (few long waveforms); 0 before the plan's first such call."""
        self._open("last_bins_form")
        return int(self.ctx.lib.drx_plan_last_bins_form(self._h))

    def last_bins_listed(self) -> int:
        """After finish(): how many waveforms the last wave_bins' block form handed to the lane kernel behind it (flagged or
        judged suspect by the block parse; all their rows are written again and judged there); 0 for the lane form."""
        self._open("last_bins_listed")
        return int(self.ctx.lib.drx_plan_last_bins_listed(self._h))

    def last_transcode_form(self) -> int:
        """DRX_TRANSCODE_FORM_* (include/deltarice_hip.h): which form the last transcode (the sizing call included) or
        estimate_words_encoded took -- a lane per waveform, or a workgroup per block of a waveform's stream (few long waveforms,
        any prediction filter); refilter and estimate_words_refiltered report LANES | REFILTER, and REFILTER_SERIAL where their
        serial kernels ran; 0 before the plan's first such call."""
        return int(self.ctx.lib.drx_plan_last_transcode_form(self._h))

    def last_transcode_listed(self) -> int:
        """After finish(): how many waveforms the last transcode's block form handed to the lane kernels behind it (flagged or
        judged suspect by the block parse, or with samples and no payload word); 0 for the lane form."""
        return int(self.ctx.lib.drx_plan_last_transcode_listed(self._h))

    def last_pulses_listed(self) -> int:
        """After finish(): how many waveforms the last find_pulses' block form handed to the lane kernel behind it (flagged by the
        block parse, or short of staged records); 0 for the lane form."""
        return int(self.ctx.lib.drx_plan_last_pulses_listed(self._h))

    def last_pulses_redone(self) -> int:
        """After finish(): how many waveforms the last find_pulses' block form finished by its second launch of the blocks (a block
        of theirs had staged fewer records than the waveform needs: max_pulses above PULSES_STAGE_CAP only); 0 for the lane form."""
        return int(self.ctx.lib.drx_plan_last_pulses_redone(self._h))

    def last_encode_path(self) -> int:
        """DRX_ENC_* (include/deltarice_hip.h): the encoder the last encode used."""
        return int(self.ctx.lib.drx_plan_last_encode_path(self._h))

    def wave_words(self) -> np.ndarray:
        """n_i (payload words) of every waveform from the last encode/decode, on the host."""
        buf = np.empty(self.total_waves, dtype=np.uint32)
        self.ctx._check(self.ctx.lib.drx_plan_read_wave_words(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint32))))
        return buf
