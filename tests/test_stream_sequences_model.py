"""The schedules of tests/stream_sequences.py against the oracle and the numpy references alone (no GPU): a green
tests/test_gpu_stream_sequences.py means something only if every step it runs has an expectation that comes from a reference
over the oracle's decode, the schedules hold the sequences they promise, the damaged streams are ones every header walk
accepts and only a payload parse can refuse, and the forms the steps assert are the table's."""
import time

import numpy as np
import pytest

import call_sequences as CS
import filter_reference as F
import stream_sequences as SS
from deltarice_amd import _lib as D

SPENT = [0.0]  # seconds this module's tests and fixtures took
SEEDS = (0, 1)  # the seeds tests/test_gpu_stream_sequences.py::test_stream_sessions uses
KINDS = {"stats", "bins", "bins_at_argmax", "win", "wins", "wins_at_pulses", "pcount", "pulses", "rwords", "roff", "rtable"}
SAMPLE_READERS = ("wave_stats", "wave_bins", "decode_window", "decode_windows", "find_pulses")


def all_schedules():
    for g in SS.PAIR_GEOMS:
        for a, (_, steps, _) in SS.stream_pairs(g).items():
            yield f"pairs[{g}-{a}]", steps
    for name, _, steps in SS.stream_chains():
        yield f"chain[{name}]", steps
    yield "filters", SS.stream_filter_cycle()[1]
    for f in SS.FORMS:
        yield f"form scratch[{f}]", SS.stream_form_scratch(f)[1]
    for seed in SEEDS:
        yield f"session[{seed}]", SS.stream_session(seed)[1]


@pytest.fixture(autouse=True)
def _timed():
    t = time.time()
    yield
    SPENT[0] += time.time() - t


@pytest.fixture(scope="module")
def schedules():
    t = time.time()
    out = dict(all_schedules())
    SPENT[0] += time.time() - t
    return out


def test_every_step_has_an_expectation(schedules):
    """Every buffer a step of this module writes has a key of a kind resolve() computes from a reference, every value it
    returns a key too; only a call that must fail leaves a buffer's content open."""
    n = 0
    for name, steps in schedules.items():
        for s in steps:
            assert s.op in SS.ALL_OPS + ("finish", "gather_decode"), s.label()
            if s.op not in SS.NEW_OPS:
                continue
            n += 1
            assert s.out or s.host is not None, s.label()
            assert s.ds is not None and s.args["path"] == SS.PATH_OF[s.args["family"]], s.label()
            assert (s.status != 0) == (s.op in SS.ERROR_OPS), s.label()
            for buf, (check, key) in s.out.items():
                if check == "exact":
                    assert s.status == 0 and key[0] in KINDS and key[1:4] == (s.geom, s.filt, s.ds), s.label()
                else:
                    assert check in ("guards", "intact") and s.status in (3, 4), s.label()
            if s.op in ("transcode", "transcode_size_only", "transcode_after_sizing", "transcode_small", "refilter"):
                assert s.args["total_key"][0] == "rwords" and s.args["total_key"][1:4] == (s.geom, s.filt, s.ds), s.label()
            if s.host is not None:
                assert s.host[0] in ("estimate", "estimate_refiltered") and s.host[1:4] == (s.geom, s.filt, s.ds), s.label()
    assert n > 3000


def test_expectations_come_from_the_references(schedules):
    """The first step of every operation on every geometry, every chain and every form-scratch schedule resolved: arrays of
    the size the call writes, from the numpy references over Expect.decoded and from the oracle's encode_chunk."""
    seen, todo = set(), []
    for name, steps in schedules.items():
        whole = name.startswith(("chain", "form scratch"))
        for s in steps:
            if s.op in SS.NEW_OPS and s.status == 0 and (whole or (s.op, s.geom) not in seen):
                seen.add((s.op, s.geom))
                todo.append(s)
    assert {op for op, _ in seen} == set(SS.NEW_OPS) - set(SS.ERROR_OPS)
    for s in todo:
        e = CS.expect(s.geom, s.filt, s.ds)
        W, a = e.length.size, s.args
        for buf, (check, key) in s.out.items():
            got = SS.resolve(key)
            want = {"stats": W * 8, "bins": W * a.get("n_bins", 0) * 4, "win": W * a.get("width", 0), "wins": W * a.get("n_win", 0) * a.get("width", 0),
                    "pcount": W, "pulses": W * a.get("max_pulses", 0) * 5, "toff": len(e.Ns) + 1, "ttable": W}.get(buf)
            assert got.ndim == 1 and (want is None or got.size == want), (s.label(), buf, got.size, want)
        if s.host is not None:
            sizes, _ = SS.resolve(s.host)
            assert len(sizes) == 16, s.label()
        if "total_key" in a:  # the re-coded stream passes the oracle's header walk, chunk by chunk, and decodes to the same samples
            w, off, tab = (SS.resolve((k,) + a["total_key"][1:]) for k in ("rwords", "roff", "rtable"))
            assert off[-1] == w.size and tab.size == W, s.label()
            taps = e.taps if a.get("target") is None else CS.FILTERS[a["target"]]
            c = len(e.Ns) - 1
            y = SS.O.decode_chunk(w[off[c]:off[c + 1]], CS.opts_of(a["m2"], e.Ls[c], taps))
            if taps is None or abs(taps[0]) == 1 or a.get("target") is None:
                assert np.array_equal(y, e.decoded[e.at[c]:e.at[c + 1]]), s.label()


def test_sample_readers_of_a_lossy_lead_read_the_oracles_decode():
    """Under lead2 the stream does not decode to x: every expectation of a call that reads samples is over Expect.decoded."""
    e = CS.expect("short", "lead2", "uniform")
    assert not np.array_equal(e.decoded, e.x)
    M = SS.StreamModel(["short"], "lossy")
    M.set_filter(0, "lead2")
    for op in SAMPLE_READERS:
        s = M.do(op, 0, ds="uniform")
        for buf, (check, key) in s.out.items():
            got = SS.resolve(key)
            swapped = CS.Expect(e.Ns, e.Ls, e.m, e.taps, "uniform", 0)
            swapped.x = swapped.__dict__["decoded"] = e.x  # the same reference over x instead
            real = CS.expect
            try:
                SS.expect = lambda *k: swapped
                SS._stats.cache_clear(), SS._pulses.cache_clear()
                other = SS.resolve(key)
            finally:
                SS.expect = real
                SS._stats.cache_clear(), SS._pulses.cache_clear()
            assert got.shape == other.shape and not np.array_equal(got, other), (s.label(), buf)


def test_pairs_cover_exactly_the_promised_pairs():
    new, old = set(SS.NEW_OPS), set(SS.OLD_OPS)
    assert "host_filter" not in old and old == set(CS.OPS) - {"host_filter"} and not new & old
    promised = {(a, b) for a in new | old for b in new | old if a in new or b in new}
    for g in SS.PAIR_GEOMS:
        got = []
        for a, (geoms, steps, where) in SS.stream_pairs(g).items():
            assert geoms == [g]
            for i, j in where:
                A, B = steps[i], steps[j]
                assert j == i + 1 and A.op == a and A.plan <= 0 and B.plan <= 0
                got.append((A.op, B.op))
                if A.ds is not None and B.ds is not None:
                    assert A.ds != B.ds, (g, A.label(), B.label())
                if A.op in SS.ERROR_OPS:
                    assert A.status in (3, 4) and (B.status == 0 or B.op in SS.ERROR_OPS + CS.ERROR_OPS)
        assert len(got) == len(promised) == 29 * 29 - 15 * 15 and set(got) == promised, g


def test_chains_hold_the_named_sequences():
    chains = {name: steps for name, _, steps in SS.stream_chains()}
    ops = lambda name: [s.op for s in chains[name] if s.op != "finish"]  # noqa: E731
    steps = chains["the block forms and the block decoder back to back"]
    assert ops("the block forms and the block decoder back to back") == ["decode", "wave_stats", "find_pulses", "decode_windows", "transcode", "wave_bins"]
    assert all(a.ds != b.ds for a, b in zip(steps[:5], steps[1:6])) and all(s.geom == "long" and s.filt == "delta" for s in steps)
    assert [s.args["form"] for s in steps[1:5]] == [SS.BLOCKS] * 4
    assert [s.args["max_pulses"] for s in chains["the pulse staging regrows with a call in flight"][:3]] == [1, 64, 2]
    for name in ("the pipeline on device-side arguments, few long waveforms", "the pipeline on device-side arguments, many short waveforms"):
        steps = chains[name]
        assert ops(name) == ["encode", "find_pulses", "decode_windows", "wave_stats", "wave_bins"]
        assert [s.args.get("src") for s in steps[1:5]] == [0] * 4 and steps[2].args["pulses_of"] == 1 and steps[4].args["argmax_of"] == 3
        assert steps[2].out["wins"][1][0] == "wins_at_pulses" and steps[4].out["bins"][1][0] == "bins_at_argmax"
        assert steps[2].args["n_win"] == steps[1].args["max_pulses"] > 0
    for name in ("a payload a word off, then three good readers (lanes)", "a payload a word off, then three good readers (blocks)"):
        steps = chains[name]
        assert ops(name) == ["reader_payload_off_by_a_word", "wave_bins", "find_pulses", "transcode"]
        assert steps[0].status == 4 and steps[-1].op == "finish" and steps[-1].status == 0
        assert len({s.args.get("reader", s.op) for s in steps[:4]}) == 4 and len({s.ds for s in steps[:4]}) == 4
    for name, sideband in (("a gather's sizing call, a reader by the walk, then the same gather", False),
                           ("a gather's sizing call, a reader by the side-band, then the same gather", True)):
        steps = chains[name]
        for a, x, b in (steps[0:3], steps[3:6], steps[6:9]):
            assert a.op == "gather_size_only" and b.op == "gather" and x.op in SS.READERS and x.args["sideband"] == sideband
            assert (a.ds, a.args) == (b.ds, b.args) and x.ds != a.ds
    for name in ("a transcode's sizing call, statistics and a refilter, then the transcode", "a transcode's sizing call, statistics and a refilter, then the transcode (lanes)"):
        steps = chains[name]
        assert ops(name) == ["transcode_size_only", "wave_stats", "refilter", "transcode"]
        assert (steps[0].ds, steps[0].args["m2"], steps[0].args["sideband"]) == (steps[3].ds, steps[3].args["m2"], steps[3].args["sideband"])
        assert len({s.ds for s in steps[:3]}) == 3
    for name, steps in chains.items():
        calls = [s for s in steps if s.op != "finish"]
        assert all(not s.finish for s in calls if s.out), name
        fin = [s for s in steps if s.op == "finish"]
        assert {s.plan for s in fin} == {s.plan for s in calls if s.out} and steps[-len(fin):] == fin, name


def test_filter_cycle_and_form_scratch_hold_what_they_promise():
    _, steps = SS.stream_filter_cycle()
    sets = [i for i, s in enumerate(steps) if s.op == "set_filter"]
    assert [steps[i].args["name"] for i in sets] == list(SS.LONG_CYCLE) + list(CS.FILTER_CYCLE)
    for i in sets:
        assert tuple(s.op for s in steps[i + 1:i + 1 + len(SS.SESSION_READERS)]) == SS.SESSION_READERS
    flips = [(s.filt, s.args["form"]) for s in steps if s.op == "wave_stats" and s.geom == "long"]
    assert flips == [("delta", SS.BLOCKS), ("fir3", SS.LANES), ("lead2", SS.LANES), ("delta", SS.BLOCKS)]
    assert all(s.args["form"] == SS.BLOCKS for s in steps if s.op == "transcode" and s.geom == "long")
    for family, op in SS.FORMS.items():
        _, steps = SS.stream_form_scratch(family)
        lanes_flag, all_flag = SS.FORM_FLAGS[family]
        calls = [s for s in steps if s.op == op]
        assert [s.cfg[2] for s in calls] == [lanes_flag, 0, all_flag, D.DBG_NO_LONG_PATHS, 0]
        assert [s.args["form"] for s in calls] == [SS.LANES, SS.BLOCKS, SS.BLOCKS | SS.FALLBACK_ALL, SS.LANES, SS.BLOCKS]
        data = [s.ds for s in steps if s.ds is not None]
        assert all(a != b for a, b in zip(data, data[1:]))


def test_sessions_hold_what_they_promise():
    good = [o for o in SS.ALL_OPS if o not in SS.ERROR_OPS + CS.ERROR_OPS]
    for seed in SEEDS:
        geoms, steps = SS.stream_session(seed)
        assert geoms[:2] == ["short", "long"] and geoms[2] in ("ragged", "whole") and 300 <= len(steps) <= 303
        count = {o: sum(s.op == o for s in steps) for o in SS.NEW_OPS}
        assert min(count.values()) >= 8, count
        seen = set()
        for i, s in enumerate(steps):
            if s.op not in SS.ERROR_OPS:
                continue
            for t in steps[i + 1:]:
                if t.plan == s.plan or t.plan < 0:
                    seen.add((s.op, t.op))
                if t.plan == s.plan:
                    break
        missing = {(e, g) for e in SS.ERROR_OPS for g in good} - seen
        assert not missing, (seed, sorted(missing))
        assert SS.stream_session(seed)[1] == steps  # deterministic from the seed
        last = {}
        for s in steps:  # every step of a plan on other data than the plan's step before
            if s.plan >= 0 and s.ds is not None:
                assert last.get(s.plan) != s.ds, s.label()
                last[s.plan] = s.ds


def test_damaged_streams_pass_every_walk_and_only_a_parse_refuses_them(schedules):
    """A stream with a payload a word off: the oracle's header walk accepts every chunk and gives the mended table, the
    mended n_i is one a walk finds plausible ((1 + k) to 25 bits a sample) -- and it is NOT what the victim's codes round to."""
    n = c4 = 0
    for name, steps in schedules.items():
        for s in steps:
            if s.op == "reader_corrupt_header":
                e = CS.expect(s.geom, s.filt, s.ds)
                bad = e.corrupt(*s.args["damage"][1:])
                c = s.args["damage"][2]
                assert [CS.walk_chunk(bad[e.off[cc]:e.off[cc + 1]], e.Ns[cc], e.Ls[cc]) is None for cc in range(len(e.Ns))] == \
                       [cc == c for cc in range(len(e.Ns))], s.label()
                assert s.status == 4 and not s.args["sideband"]
                c4 += 1
            if s.op != "reader_payload_off_by_a_word":
                continue
            _, c, i, by = s.args["damage"]
            e = CS.expect(s.geom, s.filt, s.ds)
            w, off, tab = SS.damaged_stream(s.geom, s.filt, s.ds, c, i, by)
            assert by in (-1, 1) and w.size == e.words.size + by and off[-1] == w.size
            walked = [CS.walk_chunk(w[off[cc]:off[cc + 1]], e.Ns[cc], e.Ls[cc]) for cc in range(len(e.Ns))]
            assert all(t is not None for t in walked) and np.array_equal(np.concatenate(walked), tab), s.label()
            g = int(e.wave_base[c]) + i
            assert int(tab[g]) == int(e.table[g]) + by and (np.delete(tab, g) == np.delete(e.table, g)).all()
            k, L = e.m.bit_length() - 1, int(e.length[g])
            assert (L * (1 + k) + 31) // 32 <= int(tab[g]) <= (L * 25 + 31) // 32, s.label()
            taps = e.taps if e.taps is not None else (1, -1)
            d = F.chunk_residuals(e.chunk_x(c), e.Ls[c], taps)
            at = int(e.start[g] - e.at[c])
            bits = int(F.code_bits(d[at:at + L], k).sum())
            assert (bits + 31) // 32 == int(e.table[g]) != int(tab[g]), s.label()
            # (a window of the refused reader holds the waveform's last sample: a window reads no payload beyond its last code)
            if s.args["reader"] in ("decode_window", "decode_windows"):
                st = SS.table(s.args["start"])
                assert (st + s.args["offset"] < e.length).all() and (st + s.args["offset"] + s.args["width"] >= e.length).all()
            n += 1
    assert n > 150 and c4 > 150


def test_expected_forms_follow_the_table(schedules):
    """The form every step asserts, from the table stated once more, cell by cell."""
    cells = set()
    for name, steps in schedules.items():
        for s in steps:
            if s.op not in SS.NEW_OPS:
                continue
            family, form, flags = s.args["family"], s.args["form"], s.cfg[2]
            kept = bool(flags & (D.DBG_NO_LONG_PATHS | D.DBG_LONG_NOT_BLOCKS))
            if family == "window":
                assert form is None
            elif family == "bins":
                assert form == D.BINS_FORM_LANES
            elif family == "refilter":
                from test_gpu_refilter import form_of
                dst = CS.FILTERS[s.args["target"]] or (1, -1)
                assert form == form_of(CS.FILTERS[s.filt], dst) and form & (D.TRANSCODE_FORM_LANES | D.TRANSCODE_FORM_REFILTER) == 9
                assert not form & D.TRANSCODE_FORM_BLOCKS
            elif s.geom in ("short", "ragged"):
                assert form == SS.LANES, s.label()
            else:
                assert s.geom in ("long", "whole")
                lanes_flag, all_flag = SS.FORM_FLAGS[family]
                if kept or flags & lanes_flag or (s.filt != "delta" and family != "transcode"):
                    assert form == SS.LANES, s.label()
                else:
                    assert form == SS.BLOCKS | (SS.FALLBACK_ALL if flags & all_flag else 0), s.label()
            cells.add((s.geom, s.filt == "delta", family, form))
    for family in SS.FORMS:  # every cell of the table is asserted somewhere
        assert ("long", True, family, SS.BLOCKS) in cells and ("long", True, family, SS.LANES) in cells
        assert ("long", False, family, SS.BLOCKS if family == "transcode" else SS.LANES) in cells
        assert ("short", True, family, SS.LANES) in cells and ("ragged", False, family, SS.LANES) in cells
    assert (SS.LANES, SS.BLOCKS, SS.FALLBACK_ALL) == (D.STATS_FORM_LANES, D.STATS_FORM_BLOCKS, D.STATS_FORM_FALLBACK_ALL)


def test_zz_model_work_stays_short():
    """The whole module's work (this file runs on a machine without a GPU with every later pull request)."""
    spent = SPENT[0]
    print(f"stream-sequence model: {spent:.1f} s of oracle and reference work")
    assert spent < 30, spent
