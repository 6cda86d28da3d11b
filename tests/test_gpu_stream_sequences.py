"""What a drx_plan carries from one call to the next when the calls READ an encoded batch -- wave_stats, wave_bins,
decode_window, decode_windows, find_pulses, transcode, refilter, the two estimates from the stream -- held to the oracle over
the schedules of tests/stream_sequences.py: every ordered pair with at least one such call on one plan, chains with no finish
between calls (device-side arguments among them), filter changes on a live plan, each block form's scratch allocated late, and
long interleaved sessions.  Every step works on other data than the plan's previous step, so a table, a block summary or a
fallback list that a call leaves behind is never what the next call computes.

The runner is tests/test_gpu_call_sequences.py's: every output buffer is pre-filled with a sentinel between guard elements
and compared WHOLE and exactly with its expected image.  Every step also asserts DRX_PATH_* and the call's form word against
the table tests/stream_sequences.py writes down by hand.  tests/test_stream_sequences_model.py holds the schedules themselves."""
import numpy as np
import pytest

import call_sequences as CS
import stream_sequences as SS
import test_gpu_call_sequences as T
from deltarice_amd import _lib as D
from test_gpu_call_sequences import finish_raw, guarded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()
    T.UPLOADS.clear()
    print("forms seen (geometry, filter, call, form word):", sorted(SS.OBSERVED))


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def up(ctx, key):
    """T.up() for the keys of both modules: the expected array goes up once, flat."""
    if key not in T.UPLOADS:
        a = np.ascontiguousarray(SS.resolve(key))
        a = a.view(np.int32) if a.dtype == np.uint32 else (a.astype(np.int64) if a.dtype == np.uint64 else a)
        T.UPLOADS[key] = torch.from_numpy(a).to(ctx.device)
    return T.UPLOADS[key]


def up_table(ctx, key):
    """An int64 / int32 table of a step's arguments on the device (None: none)."""
    if key is None:
        return None
    if key not in T.UPLOADS:
        T.UPLOADS[key] = torch.from_numpy(np.ascontiguousarray(SS.table(key))).to(ctx.device)
    return T.UPLOADS[key]


FORM_OF = {"stats": "last_stats_form", "bins": "last_bins_form", "windows": "last_windows_form", "pulses": "last_pulses_form",
           "transcode": "last_transcode_form", "refilter": "last_transcode_form"}


class Runner(T.Runner):
    """T.Runner with the operations of tests/stream_sequences.py; every other operation is the parent's."""

    def __init__(self, ctx, geoms):
        super().__init__(ctx, geoms)
        self.outs = {}  # step index -> {name: the elements the call wrote}: what a later call of a chain takes its arguments from

    def close(self):
        super().close()
        T.UPLOADS.clear()  # (the expected arrays of one schedule: bins of a sample each are 10 MB a step)

    def check(self, s, bufs):
        for name, (how, key) in s.out.items():
            if how == "exact" and name != "rows":
                up(self.ctx, key)  # (the parent's up() then finds the key)
        super().check(s, bufs)

    def source(self, s):
        """(words, offsets, words in the stream, side-band or None) of the batch a reader reads."""
        ctx, key = self.ctx, (s.geom, s.filt, s.ds)
        words, off, n_in = self.stream(s)
        tab = ("table",) + key
        damage = s.args.get("damage")
        if damage and damage[0] == "corrupt":
            words = up(ctx, ("corrupt",) + key + damage[1:])
        elif damage:
            words, off, tab = up(ctx, ("dwords",) + key + damage[1:]), up(ctx, ("doff",) + key + damage[1:]), ("dtable",) + key + damage[1:]
            n_in += damage[3]
        return words, off, n_in, (up(ctx, tab) if s.args["sideband"] else None)

    def forms(self, s):
        plan, a = self.plans[s.plan], s.args
        assert plan.last_decode_path() == a["path"], (s.label(), "path", plan.last_decode_path())
        if a["form"] is not None:
            got = getattr(plan, FORM_OF[a["family"]])()
            SS.OBSERVED.add((s.geom, s.filt, s.op if s.op not in SS.ERROR_OPS else a.get("reader", "transcode"), got))
            assert got == a["form"], (s.label(), "form", got, "the rule gives", a["form"])

    def run(self, i, s):
        ctx, op, a = self.ctx, s.op, s.args
        if a.get("total_key") is not None:  # (the size of the re-coded stream: the oracle's)
            s.total = int(SS.resolve(a["total_key"]).size)
        if op not in SS.NEW_OPS:
            return super().run(i, s)
        plan = self.plans[s.plan]
        self.last_enc.pop(s.plan, None)
        W = plan.total_waves
        reader = a.get("reader", op)
        words, off, n_in, tab = self.source(s)
        cur = torch.cuda.current_stream(ctx.device)
        bufs = {}

        def out(name, n, dtype):
            buf, view = guarded(ctx, n, dtype)
            bufs[name] = (buf, n)
            self.outs.setdefault(i, {})[name] = view
            return view

        if reader in ("estimate_encoded", "estimate_refiltered"):
            import deltarice_amd as dr
            enc = dr.EncodedBatch(words, off, n_in)
            if reader == "estimate_encoded":
                got = plan.estimate_words_encoded(enc, wave_words=tab)
            else:
                got = plan.estimate_words_refiltered(enc, CS.FILTERS[a["target"]], wave_words=tab)
            self.forms(s)
            sizes, k0 = SS.resolve(s.host)
            assert [int(v) for v in got[1:]] == sizes[1:], s.label()
            if k0:  # (RiceParameter 1 is defined only while every zig-zag value is below 32768)
                assert int(got[0]) == sizes[0], s.label()
            return
        if reader == "wave_stats":
            o = out("stats", W * D.STAT_COLS, torch.int64)
            ctx.stream.wait_stream(cur)
            plan.wave_stats_async(words, off, a["head"], out=o, wave_words=tab, in_words=n_in)
        elif reader == "wave_bins":
            o = out("bins", W * a["n_bins"] * D.BIN_COLS, torch.int64)
            if a["argmax_of"] is not None:  # the column as it lies in memory: a stride of 8
                start = self.outs[a["argmax_of"]]["stats"].view(W, D.STAT_COLS)[:, D.STAT_ARGMAX]
                assert start.stride(0) == D.STAT_COLS
            else:
                start = up_table(ctx, a["start"])
            ctx.stream.wait_stream(cur)
            plan.wave_bins_async(words, off, a["bin"], a["n_bins"], start=start, offset=a["offset"], out=o, wave_words=tab, in_words=n_in)
        elif reader == "decode_window":
            o = out("win", W * a["width"], torch.int16)
            start = up_table(ctx, a["start"])
            ctx.stream.wait_stream(cur)
            plan.decode_window_async(words, off, start, a["width"], a["offset"], a["pad"], out=o, wave_words=tab, in_words=n_in)
        elif reader == "decode_windows":
            o = out("wins", W * a["n_win"] * a["width"], torch.int16)
            if a["pulses_of"] is not None:  # the START column and the counts as find_pulses left them: strides of 5 * n_win and 5
                prev = self.outs[a["pulses_of"]]
                start = prev["pulses"].view(W, a["n_win"], D.PULSE_COLS)[:, :, D.PULSE_START]
                count = prev["pcount"]
                assert start.stride() == (a["n_win"] * D.PULSE_COLS, D.PULSE_COLS)
            else:
                start, count = up_table(ctx, a["start"]).view(W, a["n_win"]), up_table(ctx, a["count"])
            ctx.stream.wait_stream(cur)
            plan.decode_windows_async(words, off, start, a["width"], count, a["offset"], a["pad"], out=o, wave_words=tab, in_words=n_in)
        elif reader == "find_pulses":
            c = out("pcount", W, torch.int32)
            o = out("pulses", W * a["max_pulses"] * D.PULSE_COLS, torch.int64) if a["max_pulses"] else None
            ctx.stream.wait_stream(cur)
            plan.find_pulses_async(words, off, a["thr"], a["polarity"], a["min_width"], a["max_pulses"], 0, count=c, out=o, wave_words=tab,
                                   in_words=n_in)
        else:  # the re-coding calls
            oo = out("toff", plan.n_chunks + 1, torch.int64)
            ot = out("ttable", W, torch.int32)
            if reader == "refilter":
                launch = lambda w: plan.refilter_async(words, off, CS.FILTERS[a["target"]], a["m2"], w, n_in, tab, oo, ot)  # noqa: E731
            else:
                launch = lambda w: plan.transcode_async(words, off, a["m2"], w, n_in, tab, oo, ot)  # noqa: E731
            ow = None
            if op != "transcode_size_only":
                # (a damaged stream has no size of its own: the plan's bound on any result)
                ow = out("twords", (s.total if s.total is not None else plan.max_encoded_words) - a.get("cap_short_by", 0), torch.int32)
            ctx.stream.wait_stream(cur)
            if op in ("transcode_size_only", "transcode_after_sizing"):
                launch(None)
                if op == "transcode_after_sizing" and s.finish:
                    st, total = finish_raw(plan)
                    assert st == 0 and total == s.total, (s.label(), "sizing", st, total)
            if ow is not None:
                launch(ow)
        self.forms(s)
        return self.launched(s, {name: b for name, b in bufs.items() if name in s.out})


def geom_and_op():
    return [(g, a) for g in SS.PAIR_GEOMS for a in SS.ALL_OPS]


@pytest.mark.parametrize("geom,a", geom_and_op(), ids=lambda v: v)
def test_stream_pairs(ctx, O, geom, a):
    """A, then B on other data, on ONE plan, for every B: what B gives is the oracle's whatever A left in the tables, the block
    scratch, the staging and the status word (an A that fails included: B starts clean)."""
    geoms, steps, _ = SS.stream_pairs(geom)[a]
    Runner(ctx, geoms).run_all(steps)


def test_stream_chains(ctx, O):
    """No finish between the calls of a chain, one per plan at its end, every result in a buffer of its own: the block forms and
    the block decoder back to back on d_blk, the pulse staging regrown with a call in flight, the pipeline on device-side
    arguments, an error that must not outlive the call, a reader between a sizing call and its gather or transcode."""
    for name, geoms, steps in SS.stream_chains():
        try:
            Runner(ctx, geoms).run_all(steps)
        except AssertionError as e:
            raise AssertionError((name,) + e.args) from e


def test_stream_filter_cycle(ctx, O):
    """drx_plan_set_filter on used plans of `long` and `short`: every reader behind every change, the forms as they flip."""
    geoms, steps = SS.stream_filter_cycle()
    Runner(ctx, geoms).run_all(steps)


@pytest.mark.parametrize("family", list(SS.FORMS))
def test_stream_form_scratch(ctx, O, family):
    """A new plan whose first call of the kind is kept on lanes: the form's scratch is allocated by a LATER call."""
    geoms, steps = SS.stream_form_scratch(family)
    Runner(ctx, geoms).run_all(steps)


@pytest.mark.parametrize("seed", [0, 1])
def test_stream_sessions(ctx, O, seed):
    """300 steps of both modules' operations over three plans on one context, every result checked as it comes."""
    geoms, steps = SS.stream_session(seed)
    Runner(ctx, geoms).run_all(steps)
