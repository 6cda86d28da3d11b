"""GPU: the four profiling events of every call that launches (drx_plan_last_timings).

bench.py and the tools under tools/ price kernels from these intervals; every call validates them at its end, in code the
calls share.  With the context option "profile" set before a call, last_timings() after finish() gives four finite times, none
negative, none of the first three above the fourth (the whole call); with the option back at 0 the same call leaves nothing to
read and last_timings() says which option to set.  No duration is asserted.  Empty selections and width 0 return before
anything is launched and are not part of this.

One uniform plan (4 chunks of 16 waveforms of 64 samples) and one ragged plan (WaveformLengths 64, 512 and 4096), the oracle's
streams of Gaussian noise; every call once without and, where it has that form, once with the side-band table."""
import math

import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_select import Stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# name -> (chunk samples, WaveformLengths, a selection whose output chunks of two entries each have one WaveformLength)
PLANS = {
    "uniform": ([16 * 64] * 4, [64] * 4, [3, 17, 40, 63, 5]),
    "ragged": ([16 * 64, 4 * 512, 2 * 4096], [64, 512, 4096], [1, 14, 17, 18, 20, 21]),
}
ERR_ARG = 1  # DRX_ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def streams(ctx):
    from oracle import oracle
    out = {}
    for name, (Ns, Ls, _) in PLANS.items():
        x = np.random.default_rng(len(name)).normal(0, 10, sum(Ns)).astype(np.int16)
        out[name] = Stream(ctx, oracle, x, Ns, Ls, 8)
    yield out
    for st in out.values():
        st.plan.close()


def check(ctx, plan, steps, what):
    """steps: the calls of one sequence, each given what finish() returned behind the one before it (None for the first)."""
    ctx.set_option("profile", 1)
    try:
        words = None
        for i, step in enumerate(steps):
            keep = step(words)  # (its tensors live until the call is through)
            words = plan.finish()
            del keep
            t = plan.last_timings()
            assert len(t) == 4 and all(math.isfinite(v) and v >= 0.0 for v in t), (what, i, t)
            assert all(v <= t[3] for v in t[:3]), (what, i, t)
    finally:
        ctx.set_option("profile", 0)
    words = None
    for i, step in enumerate(steps):
        keep = step(words)
        with pytest.raises(D.DeltaRiceError) as e:
            plan.last_timings()
        assert e.value.status == ERR_ARG and 'set the context option "profile"' in str(e.value), (what, i, str(e.value))
        words = plan.finish()
        del keep


def calls(ctx, st, sel, sideband):
    """name -> the steps of every call under test on the stream st; sideband: with the n_i table where the call takes one."""
    p, w, off, n = st.plan, st.enc.words, st.enc.chunk_word_off, st.enc.total_words
    tab = st.table if sideband else None
    idx = np.asarray(sel, np.int64)
    out_words = torch.empty(p.max_encoded_words, dtype=torch.int32, device=ctx.device)

    def gather_resumed(words):
        return p.gather_encoded_async(w, off, idx, 2, torch.empty(words, dtype=torch.int32, device=ctx.device), n, tab)

    both = {
        "decode": [lambda _: p.decode_with_wave_words(w, off, tab, in_words=n) if sideband else p.decode_async(w, off, in_words=n)],
        "decode_select": [lambda _: p.decode_select_async(w, off, idx, in_words=n, wave_words=tab)],
        "gather_encoded": [lambda _: p.gather_encoded_async(w, off, idx, 2, None, n, tab), gather_resumed],
        "wave_stats": [lambda _: p.wave_stats_async(w, off, 8, wave_words=tab, in_words=n)],
        "decode_window": [lambda _: p.decode_window_async(w, off, None, 16, offset=8, wave_words=tab, in_words=n)],
        "find_pulses": [lambda _: p.find_pulses_async(w, off, 15, wave_words=tab, in_words=n)],
        "transcode": [lambda _: p.transcode_async(w, off, 16, out_words, n, tab)],
        "estimate_words_encoded": [lambda _: p.estimate_words_encoded(st.enc, tab)],
    }
    if not sideband:
        both["encode"] = [lambda _: p.encode_async(st.xd)]
    return both


@pytest.mark.parametrize("sideband", [False, True], ids=["walk", "sideband"])
@pytest.mark.parametrize("name", list(PLANS))
def test_every_call_brackets_its_launches(ctx, streams, name, sideband):
    st = streams[name]
    for call, steps in calls(ctx, st, PLANS[name][2], sideband).items():
        check(ctx, st.plan, steps, (name, call, sideband))
