"""Loads the C-ABI library (include/deltarice_hip.h).  No fallback: if the HIP
library is missing or cannot be loaded, importing the codec raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRX_LIB_PATH: load another build of the same ABI (A/B timing of kernel variants on one GPU box)
LIB_PATH = os.environ.get("DRX_LIB_PATH") or os.path.join(_HERE, "libdeltarice_hip.so")
PLUGIN_PATH = os.path.join(_HERE, "plugin", "libh5deltarice.so")

DRX_OK = 0
STATUS_NAMES = {0: "DRX_OK", 1: "DRX_ERR_ARG", 2: "DRX_ERR_DEVICE", 3: "DRX_ERR_CAPACITY",
                4: "DRX_ERR_CORRUPT", 5: "DRX_ERR_UNSUPPORTED", 6: "DRX_ERR_NOMEM"}
DRX_MAX_TAPS = 64

# DRX_PATH_*, DRX_ENC_* and DRX_DBG_* of include/deltarice_hip.h (tests/test_abi_surface.py holds them equal)
PATH_LANES_FUSED, PATH_LANES, PATH_BLOCKS, PATH_LONG, PATH_SIMPLE, PATH_IIR, PATH_IIR_FUSED = 1, 2, 4, 8, 16, 32, 64
PATH_SELECT = 128
PATH_GATHER = 256
PATH_STATS = 512
PATH_TRANSCODE = 1024
PATH_WINDOW = 2048
PATH_PULSES = 4096
PATH_WINDOWS = 8192
PATH_BINS = 16384
PATH_STACK = 32768
# DRX_STACK_*: the columns of a drx_wave_stack row (tests/test_wave_stack_abi.py holds them equal)
STACK_COUNT, STACK_SUM, STACK_SUMSQ = range(3)
STACK_COLS = 3
# DRX_BIN_*: the columns of a drx_wave_bins row (tests/test_wave_bins_abi.py holds them equal)
BIN_SUM, BIN_SUMSQ, BIN_MIN, BIN_MAX = range(4)
BIN_COLS = 4
# DRX_STAT_*: the columns of a drx_wave_stats row (tests/test_wave_stats_abi.py holds them equal)
STAT_MIN, STAT_ARGMIN, STAT_MAX, STAT_ARGMAX, STAT_SUM, STAT_SUMSQ, STAT_HEAD_SUM, STAT_HEAD_SUMSQ = range(8)
STAT_COLS = 8
# DRX_PULSE_*: the columns of a drx_find_pulses record (tests/test_find_pulses_abi.py holds them equal)
PULSE_START, PULSE_WIDTH, PULSE_PEAK, PULSE_ARGPEAK, PULSE_SUM = range(5)
PULSE_COLS = 5
ENC_TWO_PASS, ENC_SEGMENTS, ENC_FUSED, ENC_PIECES, ENC_STREAM, ENC_STREAM_SEGS = 1, 2, 3, 4, 5, 6
DBG_BINS_LANES = 64
DBG_BINS_ALL_FALLBACK = 128
DBG_NO_LONG_PATHS = 256
DBG_LONG_NOT_BLOCKS = 512
DBG_TRANSCODE_LANES = 1024
DBG_NO_PARALLEL_WALKS = 2048
DBG_NO_PIECES = 4096
DBG_FORCE_SEGMENTS = 8192
DBG_TRANSCODE_ALL_FALLBACK = 16384
DBG_FORCE_PIECES = 32768
DBG_NO_WIDE_FUSED = 65536
DBG_RAGGED_ONE_LANES_LAUNCH = 131072
DBG_STREAM_THREE_WGS = 262144
DBG_FORCE_STREAM = 524288
DBG_REFILTER_SERIAL = 1048576
DBG_IIR_SEPARATE = 2097152
DBG_FORCE_STREAM_SEGS = 4194304
DBG_WALK_BY_SCAN = 8388608
DBG_WALK_BY_CHAINS = 16777216
DBG_GATHER_OTHER_COPY = 33554432
DBG_STATS_LANES = 67108864
DBG_STATS_ALL_FALLBACK = 134217728
DBG_PULSES_LANES = 268435456
DBG_PULSES_ALL_FALLBACK = 536870912
DBG_WINDOWS_LANES = 1073741824
DBG_WINDOWS_ALL_FALLBACK = 2147483648
# DRX_STATS_FORM_*: drx_plan_last_stats_form (tests/test_wave_stats_blocks_abi.py holds them equal)
STATS_FORM_LANES, STATS_FORM_BLOCKS, STATS_FORM_FALLBACK_ALL = 1, 2, 4
# DRX_PULSES_FORM_*: drx_plan_last_pulses_form (tests/test_find_pulses_blocks_abi.py holds them equal)
PULSES_FORM_LANES, PULSES_FORM_BLOCKS, PULSES_FORM_FALLBACK_ALL = 1, 2, 4
PULSES_STAGE_CAP = 8  # DRX_PULSES_STAGE_CAP
# DRX_WINDOWS_FORM_*: drx_plan_last_windows_form (tests/test_decode_windows_abi.py holds them equal)
WINDOWS_FORM_LANES, WINDOWS_FORM_BLOCKS, WINDOWS_FORM_FALLBACK_ALL = 1, 2, 4
# DRX_BINS_FORM_*: drx_plan_last_bins_form (tests/test_wave_bins_abi.py holds them equal)
BINS_FORM_LANES, BINS_FORM_BLOCKS, BINS_FORM_FALLBACK_ALL = 1, 2, 4
# DRX_TRANSCODE_FORM_*: drx_plan_last_transcode_form (tests/test_transcode_blocks_abi.py holds them equal)
TRANSCODE_FORM_LANES, TRANSCODE_FORM_BLOCKS, TRANSCODE_FORM_FALLBACK_ALL = 1, 2, 4
# ... or-ed in by the re-filter calls (tests/test_refilter_abi.py holds them equal)
TRANSCODE_FORM_REFILTER, TRANSCODE_FORM_REFILTER_SERIAL = 8, 16


class DrxOpts(C.Structure):
    _fields_ = [("rice_k", C.c_uint32), ("wave_len", C.c_int64), ("n_taps", C.c_uint32),
                ("taps", C.c_int32 * DRX_MAX_TAPS)]


class DeltaRiceError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")


# every symbol include/deltarice_hip.h declares: (restype, argtypes)
_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
SIGNATURES = {
    "drx_version": (C.c_char_p, []),
    "drx_status_str": (C.c_char_p, [C.c_int]),
    "drx_device_count": (C.c_int, []),
    "drx_parse_cd_values": (C.c_int, [C.c_size_t, C.POINTER(C.c_uint), C.POINTER(DrxOpts)]),
    "drx_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "drx_ctx_destroy": (None, [_vp]),
    "drx_ctx_synchronize": (C.c_int, [_vp]),
    "drx_ctx_last_error": (C.c_char_p, [_vp]),
    "drx_ctx_stream": (_vp, [_vp]),
    "drx_ctx_device": (C.c_int, [_vp]),
    "drx_ctx_host_staging": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "drx_ctx_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int64]),
    "drx_plan_create": (C.c_int, [_vp, _u64, C.POINTER(_u32), C.POINTER(_u32), _u32, C.POINTER(_vp)]),
    "drx_plan_create_uniform": (C.c_int, [_vp, _u64, _u32, _u32, _u32, C.POINTER(_vp)]),
    "drx_plan_set_filter": (C.c_int, [_vp, _u32, C.POINTER(C.c_int32)]),
    "drx_plan_destroy": (None, [_vp]),
    "drx_plan_n_chunks": (_u64, [_vp]),
    "drx_plan_total_samples": (_u64, [_vp]),
    "drx_plan_total_waves": (_u64, [_vp]),
    "drx_plan_max_encoded_words": (_u64, [_vp]),
    "drx_plan_wave_words": (_vp, [_vp]),
    "drx_plan_wave_word_off": (_vp, [_vp]),
    "drx_plan_last_decode_path": (C.c_uint32, [_vp]),
    "drx_plan_last_encode_path": (C.c_uint32, [_vp]),
    "drx_plan_last_stats_form": (C.c_uint32, [_vp]),
    "drx_plan_last_pulses_form": (C.c_uint32, [_vp]),
    "drx_plan_last_windows_form": (C.c_uint32, [_vp]),
    "drx_plan_last_windows_listed": (C.c_uint32, [_vp]),
    "drx_plan_last_bins_form": (C.c_uint32, [_vp]),
    "drx_plan_last_bins_listed": (C.c_uint32, [_vp]),
    "drx_plan_last_transcode_form": (C.c_uint32, [_vp]),
    "drx_plan_last_transcode_listed": (C.c_uint32, [_vp]),
    "drx_plan_last_pulses_listed": (C.c_uint32, [_vp]),
    "drx_plan_last_pulses_redone": (C.c_uint32, [_vp]),
    "drx_plan_read_wave_words": (C.c_int, [_vp, C.POINTER(_u32)]),
    "drx_encode": (C.c_int, [_vp, _vp, _vp, _u64, _vp]),
    "drx_decode": (C.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "drx_decode_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "drx_decode_select": (C.c_int, [_vp, _vp, _u64, _vp, C.POINTER(_u64), _u64, _vp, _u64]),
    "drx_decode_select_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, C.POINTER(_u64), _u64, _vp, _u64]),
    "drx_gather_encoded": (C.c_int, [_vp, _vp, _u64, _vp, C.POINTER(_u64), _u64, _u64, _vp, _u64, _vp, _vp]),
    "drx_gather_encoded_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, C.POINTER(_u64), _u64, _u64, _vp, _u64, _vp, _vp]),
    "drx_wave_stats": (C.c_int, [_vp, _vp, _u64, _vp, _u32, _vp]),
    "drx_wave_stats_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u32, _vp]),
    "drx_wave_bins": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, C.c_int64, _u32, _u32, _vp, _u64]),
    "drx_wave_bins_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_int64, _u32, _u32, _vp, _u64]),
    "drx_wave_stack": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, C.c_int64, _u32, _vp, _vp, _u64]),
    "drx_wave_stack_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_int64, _u32, _vp, _vp, _u64]),
    "drx_decode_window": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, C.c_int64, _u32, C.c_int16, _vp, _u64]),
    "drx_decode_window_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_int64, _u32, C.c_int16, _vp, _u64]),
    "drx_decode_windows": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _u32, C.c_int64, _u32, C.c_int16, _vp, _u64, _u64]),
    "drx_decode_windows_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _u64, _vp, _u32, C.c_int64, _u32, C.c_int16, _vp, _u64,
                                                     _u64]),
    "drx_find_pulses": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, C.c_int64, C.c_int32, _u32, _u32, _vp, _vp]),
    "drx_find_pulses_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_int64, C.c_int32, _u32, _u32, _vp, _vp]),
    "drx_transcode": (C.c_int, [_vp, _vp, _u64, _vp, _u32, _vp, _u64, _vp, _vp]),
    "drx_transcode_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u32, _vp, _u64, _vp, _vp]),
    "drx_estimate_words_encoded": (C.c_int, [_vp, _vp, _u64, _vp, _vp, C.POINTER(_u64)]),
    "drx_transcode_filter": (C.c_int, [_vp, _vp, _u64, _vp, _u32, _u32, C.POINTER(C.c_int32), _vp, _u64, _vp, _vp]),
    "drx_transcode_filter_with_wave_words": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, C.POINTER(C.c_int32), _vp, _u64, _vp, _vp]),
    "drx_estimate_words_encoded_filter": (C.c_int, [_vp, _vp, _u64, _vp, _vp, _u32, C.POINTER(C.c_int32), C.POINTER(_u64)]),
    "drx_estimate_words": (C.c_int, [_vp, _vp, C.POINTER(_u64)]),
    "drx_plan_last_timings": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "drx_plan_finish": (C.c_int, [_vp, C.POINTER(_u64)]),
    "drx_filter_chunk_host": (C.c_int, [_vp, C.c_int, C.c_size_t, C.POINTER(C.c_uint), _vp, C.c_size_t,
                                        C.POINTER(_vp), C.POINTER(C.c_size_t)]),
}

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make` (hipcc --offload-arch=gfx950). "
                "deltarice_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(lib, name)  # AttributeError if the ABI lost a symbol
            f.restype = res
            f.argtypes = args
        _lib = lib
    return _lib
