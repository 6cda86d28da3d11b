"""Direct-chunk HDF5 file <-> VRAM path (include/deltarice_h5io.h, csrc/h5_direct.c): whole datasets move
between a file and HBM with H5Dread_chunk / H5Dwrite_chunk, one PCIe copy and one batched codec call,
instead of one filter callback (two PCIe crossings, one launch) per chunk."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from .codec import Context

H5IO_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdeltarice_h5io.so")


class Stats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("chunk_rows", C.c_uint64), ("n_chunks", C.c_uint64),
                ("raw_bytes", C.c_uint64), ("stored_bytes", C.c_uint64),
                ("t_file", C.c_double), ("t_pcie", C.c_double), ("t_gpu", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_io = None
_s, _u64, _u32, _vp, _st = C.c_char_p, C.c_uint64, C.c_uint, C.c_void_p, C.POINTER(Stats)
# name -> argument types behind the context; every call returns a drx_status and takes the stats last
SIGNATURES = {
    "drx_h5_read": [_s, _s, _vp, _u64],
    "drx_h5_read_rows": [_s, _s, C.POINTER(_u64), _u64, _vp, _u64],
    "drx_h5_copy_rows": [_s, _s, C.POINTER(_u64), _u64, _s, _s, _u64],
    "drx_h5_recompress": [_s, _s, _s, _s, _u32],
    "drx_h5_recompress_filtered": [_s, _s, _s, _s, _u32, _u32, C.POINTER(C.c_int32)],
    "drx_h5_write": [_s, _s, _vp, _u64, _u64, _u64, _u32, _u32],
    "drx_h5_write_filtered": [_s, _s, _vp, _u64, _u64, _u64, _u32, _u32, _u32, C.POINTER(C.c_int32)],
}


def _load():
    global _io
    if _io is None:
        if not os.path.exists(H5IO_PATH):
            raise ImportError(f"{H5IO_PATH} is missing: build it with `make h5io` (needs the HDF5 C library)")
        _lib.load()
        L = C.CDLL(H5IO_PATH)
        for name, args in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the ABI lost a symbol
            f.restype = C.c_int
            f.argtypes = [_vp] + args + [_st]
        _io = L
    return _io


def _call(ctx: Context, name: str, what: str, *args) -> Stats:
    """One call of the library on ctx behind the current stream's work; what: the call as an error names it."""
    st = Stats()
    ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
    rc = getattr(_load(), name)(ctx._h, *args, C.byref(st))
    if rc != _lib.DRX_OK:
        raise _lib.DeltaRiceError(rc, what)
    return st


def read(ctx: Context, path: str, name: str, out: torch.Tensor) -> dict:
    """File -> VRAM.  out: contiguous int16 tensor on ctx.device, large enough for the dataset."""
    return _call(ctx, "drx_h5_read", f"drx_h5_read({path!r}, {name!r})", os.fsencode(path), name.encode(), out.data_ptr(), out.numel()).as_dict()


def read_rows(ctx: Context, path: str, name: str, rows, out: torch.Tensor | None = None):
    """File -> VRAM, the dataset rows ``rows`` names (any integer sequence, array or CPU tensor; any order, duplicates
    allowed): only the chunks those rows lie in are fetched and decoded.  Returns (int16 tensor [n_rows, cols] on
    ctx.device, stats); out: a contiguous int16 tensor on ctx.device with room for n_rows * cols samples."""
    from .codec import _as_index_array
    idx = _as_index_array(rows)
    ip = idx.ctypes.data_as(C.POINTER(C.c_uint64))
    call = ("drx_h5_read_rows", f"drx_h5_read_rows({path!r}, {name!r})", os.fsencode(path), name.encode(), ip)
    if out is None:
        # the dataset's width is in the file: ask with an empty selection (opens the dataset, fetches nothing)
        st = _call(ctx, *call, 0, None, 0)
        out = torch.empty((idx.size, int(st.cols)), dtype=torch.int16, device=ctx.device)
    if out.device != ctx.device or out.dtype != torch.int16 or not out.is_contiguous():
        raise _lib.DeltaRiceError(1, f"out: need a contiguous int16 tensor on {ctx.device}")
    st = _call(ctx, *call, idx.size, out.data_ptr(), out.numel())
    cols = int(st.cols)
    return out.view(-1)[:idx.size * cols].view(idx.size, cols), st.as_dict()


def copy_rows(ctx: Context, src: str, name: str, rows, dst: str, dst_name: str | None = None,
              chunk_rows: int | None = None) -> dict:
    """File -> file: the dataset rows ``rows`` names (as read_rows takes them) become dataset ``dst_name`` (None: ``name``) of
    the new file ``dst`` in chunks of ``chunk_rows`` rows (None: the source's, or all rows where there are fewer), with the
    source's element type and compression_opts.  Only the chunks those rows lie in are fetched; their waveforms are regrouped
    on the GPU as encoded words (drx_gather_encoded), not decoded.  Returns the stats: n_chunks / stored_bytes = fetched."""
    from .codec import _as_index_array
    idx = _as_index_array(rows)
    return _call(ctx, "drx_h5_copy_rows", f"drx_h5_copy_rows({src!r}, {name!r} -> {dst!r})", os.fsencode(src), name.encode(),
                 idx.ctypes.data_as(C.POINTER(C.c_uint64)), idx.size, os.fsencode(dst), (name if dst_name is None else dst_name).encode(),
                 0 if chunk_rows is None else int(chunk_rows)).as_dict()


def recompress(ctx: Context, src: str, name: str, dst: str, dst_name: str | None = None, rice_m: int | None = None,
               taps=None) -> dict:
    """File -> file: dataset ``name`` of ``src`` becomes dataset ``dst_name`` (None: ``name``) of the new file ``dst`` with
    every stored chunk re-coded at RiceParameter ``rice_m`` (None: the one that makes the dataset smallest) on the GPU as
    encoded words (drx_transcode), not decoded; shape, element type, chunking and the rest of the compression_opts are the
    source's.  taps: ANOTHER prediction filter for the new dataset ((1, -1): the delta filter; drx_transcode_filter, still no
    decoded sample in memory) -- its compression_opts then carry the new taps, a delta target the two-value form; None: the
    source's filter.  Returns the stats: n_chunks / stored_bytes = fetched."""
    t = None if taps is None else [int(v) for v in taps]
    if t is not None and not 1 <= len(t) <= _lib.DRX_MAX_TAPS:
        raise _lib.DeltaRiceError(1, f"taps: {len(t)} values (1 .. {_lib.DRX_MAX_TAPS})")
    tarr = (C.c_int32 * len(t))(*t) if t else None
    what = f"drx_h5_recompress({src!r}, {name!r} -> {dst!r}" + (f", taps={tuple(t)})" if t else ")")
    return _call(ctx, "drx_h5_recompress_filtered", what, os.fsencode(src), name.encode(), os.fsencode(dst),
                 (name if dst_name is None else dst_name).encode(), 0 if rice_m is None else int(rice_m), len(t) if t else 0, tarr).as_dict()


def write(ctx: Context, path: str, name: str, x: torch.Tensor, rows: int, cols: int, chunk_rows: int,
          rice_m: int = 8, wave_len: int | None = None, taps=None) -> dict:
    """VRAM -> file.  x: contiguous int16 tensor [rows*cols] on ctx.device.  taps: a general prediction filter
    (compression_opts[3:], src/deltaRice.c:277-289 of the reference); None: the delta filter."""
    taps = [int(t) for t in (taps or ())]
    tarr = (C.c_int32 * max(len(taps), 1))(*taps)
    return _call(ctx, "drx_h5_write_filtered", f"drx_h5_write({path!r}, {name!r})", os.fsencode(path), name.encode(), x.data_ptr(),
                 rows, cols, chunk_rows, rice_m, cols if wave_len is None else wave_len, len(taps), tarr).as_dict()
