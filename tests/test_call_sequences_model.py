"""The schedules of tests/call_sequences.py against the oracle alone (no GPU): a green tests/test_gpu_call_sequences.py means
something only if every step it runs has an expectation, the schedules hold the sequences they promise, the lists are ones
the library accepts and the damaged streams are ones the oracle's own header walk rejects."""
import time

import numpy as np
import pytest

import call_sequences as CS
from deltarice_amd.codec import gather_geometry

SPENT = [0.0]  # seconds this module's tests and fixtures took: oracle work, all of it
SEEDS = (0, 1)  # the seeds tests/test_gpu_call_sequences.py::test_long_sessions uses


def all_schedules():
    for g in CS.GEOMETRIES:
        yield f"pairs[{g}]", CS.pairs(g)[1]
    for seed in SEEDS:
        yield f"session[{seed}]", CS.session(seed)[1]
    for name, _, steps in CS.async_chains():
        yield f"chain[{name}]", steps
    yield "tour", CS.route_tour()[1]
    yield "filters", CS.filter_cycle()[1]
    yield "growth", CS.scratch_growth()[1]
    for seed in (0, 1, 2):
        yield f"host[{seed}]", CS.host_sequence(seed)


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


def check_expectation(s):
    """Every buffer a step writes and every value it returns has an expectation, and the expectation is the oracle's."""
    assert s.op in CS.OPS + ("finish", "gather_decode"), s.label()
    if s.op in ("set_filter", "set_flags", "finish"):
        return
    assert s.out or s.host is not None or s.op == "read_wave_words", s.label()
    for name, (check, key) in s.out.items():
        assert check in ("exact", "guards", "intact"), s.label()
        if check != "exact":
            assert s.status in (3, 4), s.label()  # only a call that fails leaves a buffer's content open
            continue
        got = CS.resolve(key)
        if key[0] == "rows":
            start, length = got
            e = CS.expect(*key[1:4])
            assert start.size == len(key[4]) and (length > 0).all() and (start + length <= e.decoded.size).all(), s.label()
        else:
            assert got.size > 0, s.label()
    if s.op == "estimate":
        sizes, _ = CS.resolve(s.host)
        e = CS.expect(*s.host[1:])
        k = e.m.bit_length() - 1
        assert len(sizes) == 16 and sizes[k] == e.words.size, s.label()  # (the helper module's count is the oracle's, at the plan's k)
    if s.op == "host_filter":
        assert CS.resolve(s.host).size > 0, s.label()
    if s.op in ("encode", "encode_small"):
        assert s.total == CS.expect(s.geom, s.filt, s.ds).words.size, s.label()


def test_every_step_has_an_expectation(schedules):
    n = 0
    for name, steps in schedules.items():
        for s in steps:
            check_expectation(s)
            n += 1
    assert n > 3000


def test_streams_decode_to_what_the_steps_expect():
    """The decoded samples are the oracle's decode of the oracle's stream -- the input itself where the filter's lead is a unit."""
    from oracle import oracle as O
    for g, G in CS.GEOMETRIES.items():
        for f in G.filters[:2]:
            e = CS.expect(g, f, "gauss10")
            for c in (0, len(G.Ns) - 1):
                got = O.decode_chunk(e.chunk_words[c], CS.opts_of(G.m, G.Ls[c], CS.FILTERS[f]))
                assert np.array_equal(got, e.decoded[e.at[c]:e.at[c + 1]]), (g, f, c)
    e = CS.expect("short", "lead2", "uniform")
    assert not np.array_equal(e.decoded, e.x)


def test_estimate_sizes_are_the_helper_modules():
    """Expect.estimate counts in 32-bit integers; F.words, one waveform at a time, is the statement it is held to."""
    import filter_reference as F
    for g, f, ds in (("short", "fir5", "uniform"), ("short", "taps64", "gauss400"), ("ragged", "lead2", "gauss400"), ("whole", "fir3", "gauss10"), ("mid", "delta", "zeros")):
        e = CS.expect(g, f, ds)
        sizes, k0 = e.estimate
        taps = e.taps if e.taps is not None else (1, -1)
        for k in (0, 1, 3, 9, 15):
            want = 0
            for c, (N, L) in enumerate(zip(e.Ns, e.Ls)):
                d = F.chunk_residuals(e.chunk_x(c), L, taps)
                want += 1 + sum(1 + F.words(d[s0:s0 + n], k) for s0, n in F.waveforms(N, L))
            assert sizes[k] == want, (g, f, ds, k)
        d = np.concatenate([F.chunk_residuals(e.chunk_x(c), L, taps) for c, L in enumerate(e.Ls)]).astype(np.int64)
        assert k0 == (int(np.where(d < 0, -2 * d - 1, 2 * d).max()) < 32768), (g, f, ds)


def test_geometries_and_datasets_are_what_the_schedules_need():
    """A shorter last waveform in a chunk of every geometry (the whole-chunk batch has one waveform a chunk: none can be
    shorter); code lengths more than 10-fold apart between datasets where the ring threshold matters; at most about 2 M
    samples, but for `iir`, whose 1536 waveforms of 2048 samples are the fewest that reach DRX_PATH_IIR_FUSED."""
    for g, G in CS.GEOMETRIES.items():
        if g != "whole":
            assert any(L and N % L for N, L in zip(G.Ns, G.Ls)), g
        assert sum(G.Ns) <= (3_200_000 if g == "iir" else 2_100_000), g
    for g in ("short", "mid"):
        assert CS.expect(g, "delta", "uniform").table.sum() > 10 * CS.expect(g, "delta", "zeros").table.sum(), g  # (code words, n_i)
    # a waveform of `mid` outgrows a ring of the persistent encoder (kEsRingWords, 2496 words) or fits it five times over
    assert CS.expect("mid", "delta", "uniform").table.min() > 2496 > 5 * CS.expect("mid", "delta", "zeros").table.max()


def test_filter_cycle_holds_every_call_behind_every_change():
    _, steps = CS.filter_cycle()
    assert [s.args["name"] for s in steps if s.op == "set_filter"] == list(CS.FILTER_CYCLE)
    assert [s.op for s in steps[:8]] == ["set_filter", "encode", "decode", "decode_sideband", "select", "gather", "gather_decode", "estimate"]
    assert len(steps) == 8 * len(CS.FILTER_CYCLE) and all(a.ds != b.ds for a, b in zip(steps[1:4], steps[2:5]))


def test_pairs_cover_every_ordered_pair():
    N = len(CS.OPS)
    for g in CS.GEOMETRIES:
        _, steps, where = CS.pairs(g)
        got = {(steps[a].op, steps[b].op) for a, b in where}
        assert got == {(a, b) for a in CS.OPS for b in CS.OPS} and len(where) == N * N, g
        for a, b in where:
            A, B = steps[a], steps[b]
            assert b == a + 1 and A.plan <= 0 and B.plan <= 0
            if A.ds is not None and B.ds is not None and "host_filter" not in (A.op, B.op):
                assert A.ds != B.ds, (g, A.label(), B.label())


def test_sessions_hold_what_they_promise():
    good = [o for o in CS.OPS if o not in CS.ERROR_OPS]
    for seed in SEEDS:
        geoms, steps = CS.session(seed)
        assert len(set(geoms)) == 3 and 300 <= len(steps) <= 302
        count = {o: sum(s.op == o for s in steps) for o in CS.OPS}
        assert min(count.values()) >= 10, count
        assert len({s.plan for s in steps if s.plan >= 0}) == 3
        # "an error, then a good call of every other kind on the same plan": the plan's next call, whatever ran on the
        # others in between (set_flags and host_filter are calls on the context: any of them before the plan's next call)
        seen = set()
        for i, s in enumerate(steps):
            if s.op not in CS.ERROR_OPS:
                continue
            for t in steps[i + 1:]:
                if t.plan == s.plan or t.plan < 0:
                    seen.add((s.op, t.op))
                if t.plan == s.plan:
                    break
        missing = {(e, g) for e in CS.ERROR_OPS for g in good} - seen
        assert not missing, (seed, sorted(missing))
        assert CS.session(seed)[1] == steps  # deterministic from the seed


def test_chains_hold_the_named_sequences():
    chains = {name: (geoms, steps) for name, geoms, steps in CS.async_chains()}
    ops = lambda name, p=None: [s.op for s in chains[name][1] if s.op != "finish" and (p is None or s.plan == p)]
    assert ops("encode-decode-encode-select-gather") == ["encode", "decode", "encode", "select", "gather"]
    _, steps = chains["encode-decode-encode-select-gather"]
    assert steps[0].ds != steps[2].ds and steps[1].args["src"] == 0 and steps[3].args["src"] == 2 and steps[4].args["src"] == 2
    geoms, steps = chains["the same chain alternating between two plans"]
    assert geoms[0] == geoms[1] and [(s.op, s.plan) for s in steps[:5]] == [("encode", 0), ("decode", 1), ("encode", 0), ("select", 1), ("gather", 0)]
    assert [s.args.get("src") for s in steps[1:5]] == [0, None, 2, 2]
    for name in ("a sizing call, an encode or a decode, then the same gather", "a sizing call, a side-band decode or a selection, then the same gather"):
        steps = chains[name][1]
        for a, x, b in (steps[0:3], steps[3:6]):
            assert a.op == "gather_size_only" and b.op == "gather" and x.op in ("encode", "decode", "decode_sideband", "select")
            assert (a.ds, a.args) == (b.ds, b.args) and x.ds != a.ds and a.plan == x.plan == b.plan
    sizes = [len(s.args["idx"]) for s in chains["selection scratch regrows with a call in flight"][1] if s.op == "select"]
    assert sizes == [5000, 3, 6000]
    geoms, steps = chains["ragged decodes back to back on two plans"]
    assert geoms == ["ragged", "ragged"] and [s.plan for s in steps[:2]] == [0, 1] and steps[0].op == steps[1].op == "decode"
    lost = chains["a capacity error, then an encode, no finish between"][1]
    assert [s.op for s in lost[2:]] == ["encode_small", "encode", "finish"] and lost[-1].status == 0 and lost[-1].total == lost[-2].total
    lost = chains["a damaged stream, then decodes, no finish between"][1]
    assert [s.op for s in lost[1:]] == ["decode_corrupt", "decode", "decode_sideband", "finish"] and lost[-1].status == 0
    for name, (geoms, steps) in chains.items():
        calls = [s for s in steps if s.op != "finish"]
        assert all(not s.finish for s in calls if s.out), name
        fin = [s for s in steps if s.op == "finish"]
        assert {s.plan for s in fin} == {s.plan for s in calls if s.out} and steps[-len(fin):] == fin, name


def test_gather_lists_are_valid(schedules):
    n = 0
    for name, steps in schedules.items():
        for s in steps:
            if not s.op.startswith("gather"):
                continue
            G = CS.GEOMETRIES[s.geom]
            for idx in (s.args["idx"],) + ((s.args["sized"],) if "sized" in s.args else ()):
                N, L = gather_geometry(G.Ns, G.Ls, np.array(idx), s.args["cw"])  # (raises where the list breaks the rule)
                _, off, tab = CS.expect(s.geom, s.filt, s.ds).gather(idx, s.args["cw"])
                assert off.size == N.size + 1 and tab.size == len(idx), s.label()
                n += 1
            if "sized" in s.args:
                assert len(s.args["sized"]) == len(s.args["idx"]) and s.args["sized"] != s.args["idx"], s.label()
    assert n > 500


def test_corrupt_streams_are_rejected_by_the_oracle_walk(schedules):
    """Walking n_i from the chunk's start must not end at the chunk's end (or the sample count is not the chunk's)."""
    n = 0
    for name, steps in schedules.items():
        for s in steps:
            if s.op == "decode_corrupt":
                e = CS.expect(s.geom, s.filt, s.ds)
                bad = e.corrupt(s.args["kind"], s.args["chunk"], s.args["wave"])
                assert (bad != e.words).sum() == 1, s.label()
                c = s.args["chunk"]
                for cc in range(len(e.Ns)):
                    got = CS.walk_chunk(bad[e.off[cc]:e.off[cc + 1]], e.Ns[cc], e.Ls[cc])
                    assert (got is None) == (cc == c), s.label()
                n += 1
            elif s.op == "host_filter" and "corrupt" in s.args:
                e = CS.host_expect(s.args["case"], s.ds)
                bad = e.corrupt(*s.args["corrupt"])
                assert (bad != e.words).sum() == 1, s.label()
                # (the host path takes the sample count from the stream itself)
                assert CS.walk_chunk(bad, int(bad[0]), e.Ls[0]) is None, s.label()
                n += 1
    assert n > 100


def test_tour_names_every_encoder_and_follower():
    _, steps = CS.route_tour()
    calls = [s for s in steps if s.plan == 0 and "path" not in s.args]
    follow = {}
    for a, b in zip(calls, calls[1:]):
        if a.op == "encode":
            follow.setdefault(a.args["enc"], set()).add(b.args.get("walk") or (b.op if b.op != "encode" else ("other" if b.args["enc"] != a.args["enc"] else "same")))
    assert sorted(follow) == [1, 2, 3, 4, 5, 6]
    assert all(v >= {"other", "fused", "parallel", "estimate"} for v in follow.values()), follow


def test_zz_oracle_work_stays_short():
    """The whole module's oracle work (this file runs on a machine without a GPU with every later pull request)."""
    spent = SPENT[0]
    print(f"call-sequence model: {spent:.1f} s of oracle work")
    assert spent < 30, spent
