"""A stand-in plan for the CPU tests of deltarice_amd.codec's entries: a Plan made without a context or a GPU, as far as the
Python entries' own checks go, over a library that records what it is called with instead of doing it."""
import numpy as np
import torch

NULL_PLAN = 1  # DRX_ERR_ARG: what every drx_* call returns for a NULL plan (tests/test_codec_calls.py asks the real library)


class RecordingLib:
    """Every drx_* attribute is a function that appends (symbol, args) to ``calls`` and returns DRX_OK -- NULL_PLAN where the
    plan handle, the first argument, is None, as the library does."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("drx_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return NULL_PLAN if args[0] is None else 0
        return call


class _Ctx:
    def __init__(self, device):
        self.device, self.lib = device, RecordingLib()

    def _check(self, st):
        if st:
            from deltarice_amd import DeltaRiceError
            raise DeltaRiceError(st, "as recorded")


def plan(total_waves=3):
    """A plan of one chunk of 250 samples in waveforms of 100 on the device ``cpu``; ``plan.ctx.lib.calls`` is the record."""
    from deltarice_amd import codec
    plan = object.__new__(codec.Plan)
    plan.ctx, plan._h = _Ctx(torch.device("cpu")), 1
    plan.total_waves, plan.n_chunks = total_waves, 1
    plan.total_samples, plan.max_encoded_words = 250, 300
    plan._chunk_samples, plan._wave_lens = np.array([250]), np.array([100])
    plan._rice_m, plan._taps = 8, None
    return plan
