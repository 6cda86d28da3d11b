"""deltarice_amd -- MI355X-native Delta-Rice codec behind HDF5 filter 32025.

Layout: ``csrc/`` holds the HIP kernels, the C ABI and the H5Z plugin source;
``codec`` is the host-side batch API over device-resident chunks; ``h5`` mirrors
the reference's ``deltaRice.h5`` registration module; ``dist`` shards a batch of
chunks over the GPUs of a node; ``optimise`` searches RiceParameter and encoding filter
(docs/Optimization.md of the reference).  There is no CPU implementation in this package.
"""
from ._lib import DeltaRiceError, LIB_PATH, PLUGIN_PATH  # noqa: F401
from ._lib import (PATH_PULSES, PATH_STATS, PATH_TRANSCODE, PATH_WINDOW, PATH_WINDOWS, PULSE_ARGPEAK, PULSE_COLS, PULSE_PEAK, PULSE_START,  # noqa: F401
                   PULSE_SUM, PULSE_WIDTH)
from ._lib import (STAT_ARGMAX, STAT_ARGMIN, STAT_COLS, STAT_HEAD_SUM, STAT_HEAD_SUMSQ,  # noqa: F401
                   STAT_MAX, STAT_MIN, STAT_SUM, STAT_SUMSQ)

from ._lib import DBG_REFILTER_SERIAL, TRANSCODE_FORM_REFILTER, TRANSCODE_FORM_REFILTER_SERIAL  # noqa: F401
from ._lib import (BIN_COLS, BIN_MAX, BIN_MIN, BIN_SUM, BIN_SUMSQ, BINS_FORM_BLOCKS, BINS_FORM_FALLBACK_ALL, BINS_FORM_LANES,  # noqa: F401
                   DBG_BINS_ALL_FALLBACK, DBG_BINS_LANES, PATH_BINS)
from ._lib import PATH_STACK, STACK_COLS, STACK_COUNT, STACK_SUM, STACK_SUMSQ  # noqa: F401

H5FILTER = 32025


def __getattr__(name):
    # torch is only needed for the device-resident API; keep `import deltarice_amd` light
    if name in ("Context", "Plan", "EncodedBatch", "Gathered", "Transcoded", "parse_opts"):
        from . import codec
        return getattr(codec, name)
    if name == "optimise_encoded":  # (optimise() itself stays `from deltarice_amd.optimise import optimise`: the module has its name)
        from .optimise import optimise_encoded
        return optimise_encoded
    raise AttributeError(name)
