"""What a drx_plan and a drx_ctx carry from one call to the next, held to the oracle over sequences of calls: the schedules
of tests/call_sequences.py (every ordered pair of operations on one plan, long interleaved sessions over three plans, chains
of calls with no finish between them, filter changes on a live plan, the one-chunk host path between geometries) driven
through deltarice_amd.  Every comparison is exact and on the device; every output buffer is pre-filled with a sentinel
between guard words and compared WHOLE with its expected image, so a call that writes a word too many, leaves one out or
leaves the last call's bytes in place fails.  tests/test_call_sequences_model.py holds the schedules to the oracle."""
import ctypes as C
import threading

import numpy as np
import pytest

import call_sequences as CS
from deltarice_amd import _lib as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64  # elements in front of and behind every output buffer
SENTINEL = {torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
ROW_PAD = 8  # samples between a selection's rows (the plan's longest waveform + these: every row is guarded)

UPLOADS = {}  # key -> device tensor: every expected array goes up once per module
ROUTES = {"enc": set(), "path": 0, "after": {}}  # DRX_ENC_* seen, DRX_PATH_* bits seen, encoder -> kinds of call that followed it


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()
    UPLOADS.clear()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def up(ctx, key):
    if key not in UPLOADS:
        a = np.ascontiguousarray(CS.resolve(key))
        a = a.view(np.int32) if a.dtype == np.uint32 else (a.astype(np.int64) if a.dtype == np.uint64 else a)
        UPLOADS[key] = torch.from_numpy(a).to(ctx.device)
    return UPLOADS[key]


def guarded(ctx, n, dtype):
    """-> (the whole allocation, the n elements a call may write), all of it the sentinel."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=ctx.device)
    return buf, buf[GUARD:GUARD + n]


def make_plan(ctx, geom):
    G = CS.GEOMETRIES[geom]
    if len(set(G.Ns)) == 1 and len(set(G.Ls)) == 1:
        plan = ctx.plan_uniform(len(G.Ns), G.Ns[0], (G.m, G.Ls[0]) if G.Ls[0] else (G.m,))
    else:
        plan = ctx.plan(list(G.Ns), list(G.Ls), G.m)
    plan.set_filter(CS.FILTERS[G.filters[0]])
    return plan


def finish_raw(plan):
    """drx_plan_finish as the ABI gives it: (status, total words)."""
    n = C.c_uint64()
    st = plan.ctx.lib.drx_plan_finish(plan._h, C.byref(n))
    return int(st), int(n.value)


def set_cfg(ctx, cfg):
    ctx.set_option("encode_impl", cfg[0])
    ctx.set_option("decode_impl", cfg[1])
    ctx.set_option("debug_flags", cfg[2])


class Runner:
    """Runs a schedule's steps on one context; a step with finish=False is checked when the chain's finish steps come."""

    def __init__(self, ctx, geoms):
        self.ctx = ctx
        self.plans = [make_plan(ctx, g) for g in geoms]
        self.pending = []     # (step, {name: (allocation, elements)}) not checked yet
        self.produced = {}    # step index -> (words, offsets, total) an encode of the chain wrote
        self.last_enc = {}    # plan index -> the encoder of its last call, if that was an encode

    def close(self):
        set_cfg(self.ctx, CS.DEFAULT_CFG)
        for p in self.plans:
            p.close()

    # -- what the route coverage at the module's end is made of --
    def note(self, s, kind, path=None):
        p = s.plan
        before = self.last_enc.pop(p, None)
        if kind == "encode":
            ROUTES["enc"].add(path)
            self.last_enc[p] = path
            if "enc" in s.args:
                assert path == s.args["enc"], s.label()
            kind = "another encoder" if before not in (None, path) else None
        elif kind == "decode":
            ROUTES["path"] |= path
            fused = bool(path & D.PATH_LANES_FUSED)
            # The library does not report the walk; one case proves it.  A uniform batch under decode_impl 8 without a side-band
            # takes the lane decoder WITH the walk inside (LANES_FUSED) unless a parallel walk takes the batch (route_decode()): there
            # PATH_LANES alone means a parallel walk ran.  Only such decodes are counted.
            G = CS.GEOMETRIES[s.geom]
            uniform = len(set(G.Ns)) == 1 and len(set(G.Ls)) == 1
            parallel = uniform and s.cfg[1] == 8 and s.op == "decode" and path == D.PATH_LANES
            if "walk" in s.args:  # (the tour, on `short`: the lane decoder, behind a parallel walk or with the walk inside)
                assert path == (D.PATH_LANES_FUSED if s.args["walk"] == "fused" else D.PATH_LANES) and (fused or parallel), s.label()
            if "path" in s.args:
                assert path == s.args["path"], (s.label(), path)
            kind = "fused-walk decode" if fused else ("parallel-walk decode" if parallel else None)
        if before is not None and kind:
            ROUTES["after"].setdefault(before, set()).add(kind)

    def stream(self, s):
        """The encoded batch a decoding step reads: an earlier step's output, or the oracle's stream."""
        if s.args.get("src") is not None:
            return self.produced[s.args["src"]]
        key = (s.geom, s.filt, s.ds)
        return up(self.ctx, ("words",) + key), up(self.ctx, ("off",) + key), int(CS.expect(*key).words.size)

    def check(self, s, bufs):
        ctx = self.ctx
        for name, (how, key) in s.out.items():
            buf, n = bufs[name]
            S = SENTINEL[buf.dtype]
            if how == "intact":
                assert bool((buf == S).all()), (s.label(), name, "written behind an error")
            elif how == "guards":
                assert bool((buf[:GUARD] == S).all()) and bool((buf[GUARD + n:] == S).all()), (s.label(), name, "guard words")
            elif name == "rows":
                start, length = (torch.from_numpy(a).to(ctx.device) for a in CS.resolve(key))
                dec = up(ctx, ("decoded",) + key[1:4])
                stride = n // max(1, start.numel())
                col = torch.arange(stride, device=ctx.device)
                at = (start[:, None] + col[None, :]).clamp_(max=dec.numel() - 1)
                img = torch.full_like(buf, S)
                img[GUARD:GUARD + n] = torch.where(col[None, :] < length[:, None], dec[at], torch.tensor(S, dtype=buf.dtype, device=ctx.device)).reshape(-1)
                assert torch.equal(buf, img), (s.label(), name)
            else:
                want = up(ctx, key)
                assert want.numel() == n, (s.label(), name, want.numel(), n)
                img = torch.full_like(buf, S)
                img[GUARD:GUARD + n] = want
                if not torch.equal(buf, img):
                    guards = bool((buf[:GUARD] == S).all()) and bool((buf[GUARD + n:] == S).all())
                    bad = torch.nonzero(buf[GUARD:GUARD + n] != want).reshape(-1)
                    raise AssertionError((s.label(), name, f"{bad.numel()} of {n} elements differ, the first at {int(bad[0]) if bad.numel() else None}",
                                          "guards intact" if guards else "GUARD WORDS WRITTEN"))

    def launched(self, s, bufs):
        plan = self.plans[s.plan]
        if not s.finish:
            self.pending.append((s, bufs))
            return
        st, total = finish_raw(plan)
        assert st == s.status, (s.label(), "status", st)
        if s.total is not None:
            assert total == s.total, (s.label(), "total", total)
        self.check(s, bufs)

    def run(self, i, s):
        ctx, op = self.ctx, s.op
        if op == "set_flags":
            return set_cfg(ctx, s.args["cfg"])
        if op == "host_filter":
            return host_step(ctx, s)
        plan = self.plans[s.plan]
        key = (s.geom, s.filt, s.ds)
        if op == "finish":
            st, total = finish_raw(plan)
            assert st == s.status, (s.label(), "status", st)
            if s.total is not None:
                assert total == s.total, (s.label(), "total", total)
            if all(t.op == "finish" for t in self.steps[i + 1:]) and i + 1 < len(self.steps):
                return  # (the other plans' finishes first)
            ctx.synchronize()
            for t, bufs in self.pending:
                self.check(t, bufs)
            self.pending = []
            return
        if op == "set_filter":
            self.last_enc.pop(s.plan, None)
            return plan.set_filter(CS.FILTERS[s.args["name"]])
        if op == "estimate":
            got = plan.estimate_words(up(ctx, ("x",) + key))
            sizes, k0 = CS.resolve(s.host)
            assert [int(v) for v in got[1:]] == sizes[1:], s.label()
            if k0:  # (RiceParameter 1 is defined only while every zig-zag value is below 32768)
                assert int(got[0]) == sizes[0], s.label()
            before = self.last_enc.pop(s.plan, None)
            if before is not None:
                ROUTES["after"].setdefault(before, set()).add("estimate")
            return
        if op == "read_wave_words":
            self.last_enc.pop(s.plan, None)
            got = plan.wave_words()
            assert got.shape == (plan.total_waves,), s.label()
            if s.host is not None:
                table, mask = CS.resolve(s.host)
                assert np.array_equal(got[mask], table[mask]), s.label()
            return
        cur = torch.cuda.current_stream(ctx.device)
        if op in ("encode", "encode_small"):
            cap = s.args.get("cap", s.total)
            wbuf, w = guarded(ctx, cap, torch.int32)
            obuf, o = guarded(ctx, plan.n_chunks + 1, torch.int64)
            x = up(ctx, ("x",) + key)
            ctx.stream.wait_stream(cur)
            plan.encode_async(x, w, o)
            self.note(s, "encode", plan.last_encode_path())
            self.produced[i] = (w, o, s.total)
            return self.launched(s, {"words": (wbuf, cap), "off": (obuf, plan.n_chunks + 1)})
        if op in ("decode", "decode_sideband", "decode_corrupt"):
            words, off, n_in = self.stream(s)
            if op == "decode_corrupt":
                words = up(ctx, ("corrupt",) + key + (s.args["kind"], s.args["chunk"], s.args["wave"]))
            ybuf, y = guarded(ctx, plan.total_samples, torch.int16)
            tab = up(ctx, ("table",) + key) if op == "decode_sideband" else None
            ctx.stream.wait_stream(cur)
            if tab is not None:
                plan.decode_with_wave_words(words, off, tab, y, in_words=n_in)
            else:
                plan.decode_async(words, off, y, in_words=n_in)
            self.note(s, "decode", plan.last_decode_path())
            return self.launched(s, {"samples": (ybuf, plan.total_samples)})
        if op == "gather_decode":
            return self.gather_decode(s)
        words, off, n_in = self.stream(s)
        tab = up(ctx, ("table",) + key) if s.args["sideband"] else None
        idx = np.array(s.args["idx"], np.uint64)
        if op == "select":
            stride = plan.longest_wave() + ROW_PAD
            rbuf, r = guarded(ctx, idx.size * stride, torch.int16)
            ctx.stream.wait_stream(cur)
            plan.decode_select_async(words, off, idx, r.view(idx.size, stride), in_words=n_in, wave_words=tab)
            assert plan.last_decode_path() == D.PATH_SELECT, s.label()
            self.note(s, "select")
            ROUTES["path"] |= D.PATH_SELECT
            return self.launched(s, {"rows": (rbuf, idx.size * stride)})
        # the gathers
        cw = s.args["cw"]
        n_out = -(-idx.size // cw)
        obuf, o = guarded(ctx, n_out + 1, torch.int64)
        tbuf, t = guarded(ctx, idx.size, torch.int32)
        bufs = {"goff": (obuf, n_out + 1), "gtable": (tbuf, idx.size)}
        ctx.stream.wait_stream(cur)
        if op in ("gather_size_only", "gather_after_sizing", "gather_after_sizing_other_list"):
            sized = np.array(s.args.get("sized", s.args["idx"]), np.uint64)
            plan.gather_encoded_async(words, off, sized, cw, None, n_in, tab, o, t)
            if op != "gather_size_only" and s.finish:
                st, total = finish_raw(plan)
                assert st == 0 and total == int(CS.expect(*key).gather(tuple(int(v) for v in sized), cw)[0].size), (s.label(), "sizing", st, total)
        if op != "gather_size_only":
            cap = s.args.get("cap", s.total)
            wbuf, w = guarded(ctx, cap, torch.int32)
            bufs["gwords"] = (wbuf, cap)
            ctx.stream.wait_stream(cur)
            plan.gather_encoded_async(words, off, idx, cw, w, n_in, tab, o, t)
        assert plan.last_decode_path() == D.PATH_GATHER, s.label()
        self.note(s, "gather")
        ROUTES["path"] |= D.PATH_GATHER
        return self.launched(s, bufs)

    def gather_decode(self, s):
        """Plan.gather_encoded into a guarded buffer, then the Gathered's own plan decodes it into another."""
        import deltarice_amd as dr
        ctx, plan = self.ctx, self.plans[s.plan]
        self.last_enc.pop(s.plan, None)
        words, off, n_in = self.stream(s)
        wbuf, w = guarded(ctx, int(up(ctx, s.out["gwords"][1]).numel()), torch.int32)
        got = plan.gather_encoded(dr.EncodedBatch(words, off, n_in), np.array(s.args["idx"], np.uint64), s.args["cw"], out_words=w)
        gp = got.plan(ctx)
        try:
            ybuf, y = guarded(ctx, gp.total_samples, torch.int16)
            ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
            gp.decode_async(got.enc.words, got.enc.chunk_word_off, y, in_words=got.enc.total_words)
            st, _ = finish_raw(gp)
            assert st == 0, (s.label(), "status", st)
            self.check(s, {"samples": (ybuf, gp.total_samples), "gwords": (wbuf, w.numel())})
        finally:
            gp.close()

    def run_all(self, steps):
        self.steps = steps
        try:
            for i, s in enumerate(steps):
                after = "after: " + (steps[i - 1].label() if i else "nothing")  # (the sequence is the finding, not the step)
                try:
                    self.run(i, s)
                except AssertionError as e:
                    raise AssertionError(e.args + (after,)) from e
                except Exception as e:  # (a DeltaRiceError from a call that must succeed: name the step)
                    raise AssertionError((s.label(), repr(e), after)) from e
            assert not self.pending
        finally:
            self.close()


def host_step(ctx, s):
    """One chunk through the H5Z callback's body; a damaged stream first where the step says so (status 4), then the good one."""
    import deltarice_amd as dr
    case, reverse = s.args["case"], s.args["reverse"]
    e = CS.host_expect(case, s.ds)
    opts = CS.host_opts(case)
    if "corrupt" in s.args:
        with pytest.raises(dr.DeltaRiceError) as err:
            ctx.filter_chunk(e.corrupt(*s.args["corrupt"]), opts, reverse=True)
        assert err.value.status == 4, s.label()
    want = CS.resolve(s.host)
    got = ctx.filter_chunk(e.words if reverse else e.x, opts, reverse=reverse)
    assert got == want.tobytes(), s.label()


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", list(CS.GEOMETRIES))
def test_every_ordered_pair(ctx, O, geom):
    """A, then B on other data, for every ordered pair of operations on ONE plan: B's result is the oracle's whatever A left
    in the scratch, the tables and the status word (an error A included: B starts clean)."""
    geoms, steps, _ = CS.pairs(geom)
    Runner(ctx, geoms).run_all(steps)


@pytest.mark.parametrize("seed", [0, 1])
def test_long_sessions(ctx, O, seed):
    """300 steps over three plans of different geometry on one context, every result checked as it comes."""
    geoms, steps = CS.session(seed)
    Runner(ctx, geoms).run_all(steps)


def test_async_chains(ctx, O):
    """Chains of calls with no finish between them, every result in its own buffer, checked behind one finish per plan."""
    for name, geoms, steps in CS.async_chains():
        Runner(ctx, geoms).run_all(steps)


def test_filter_changes_on_a_live_plan(ctx, O):
    """drx_plan_set_filter on a used plan, seven times: every call behind a change gives what a new plan of that filter
    gives, into guarded buffers like every other schedule, and the batch a gather makes decodes through Gathered.plan() --
    which carries the filter Plan.set_filter set."""
    geoms, steps = CS.filter_cycle()
    Runner(ctx, geoms).run_all(steps)


def test_host_path_between_geometries(ctx, O):
    """The context's cached one-chunk plan and its staging buffers between chunks of different geometry, k and taps, damaged
    streams among them; then from two threads on the one context, each with a sequence of its own."""
    for s in CS.host_sequence(0):
        host_step(ctx, s)
    errors = []

    def worker(seed):
        try:
            for s in CS.host_sequence(seed):
                host_step(ctx, s)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(seed,)) for seed in (1, 2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors[:3]


def test_scratch_grows_and_is_kept(ctx, O):
    """A new plan through CS.scratch_growth(): a list of 1, of 3000, of 1 through the selection's staging pair; a sizing call
    that regrows the gather's scratch, and the gather that resumes from it; a sizing call, a larger selection, then the
    gather the sizing call was for."""
    geoms, steps = CS.scratch_growth()
    Runner(ctx, geoms).run_all(steps)


@pytest.mark.parametrize("wave_len", [0, 300, 400])
def test_host_path_buffers_grow_and_are_kept(O, wave_len):
    """A NEW context's one-chunk path at 1000, then 200 000, then 1000 samples, forward and reverse: its device buffers are
    replaced by the second size and kept by the third, its cached plan is replaced each time.  WaveformLength 300 gives the large
    chunk 667 waveforms, more than the 512 up to which the header chain is walked on the CPU; 400 gives it 500, whose tables
    need a larger pinned buffer than the one the first call left."""
    import deltarice_amd as dr
    c = dr.Context(0)
    try:
        for n in (1000, 200_000, 1000):
            e = CS.Expect((n,), (wave_len,), 8, None, "gauss10", CS._seed("host growth", n, wave_len))
            opts = CS.opts_of(8, wave_len, None)
            assert c.filter_chunk(e.x, opts) == e.words.tobytes(), (n, wave_len, "forward")
            assert c.filter_chunk(e.words, opts, reverse=True) == e.x.tobytes(), (n, wave_len, "reverse")
    finally:
        c.close()


def test_host_staging_grows_and_is_kept():
    """drx_ctx_host_staging on a NEW context at 1000, then 200 000, then 1000 bytes: every byte asked for is the caller's to
    write, and the buffer the second call made serves the third."""
    import deltarice_amd as dr
    c = dr.Context(0)
    try:
        at = []
        for n in (1000, 200_000, 1000):
            p = C.c_void_p()
            assert c.lib.drx_ctx_host_staging(c._h, n, C.byref(p)) == 0 and p.value, n
            C.memset(p, 0x5A, n)
            assert C.string_at(p.value + n - 4, 4) == b"\x5a" * 4
            at.append(p.value)
        assert at[2] == at[1], at
    finally:
        c.close()


def test_routes_seen_over_the_module(ctx, O):
    """Every encoder and every decode path has run in this module, and every encoder has been followed, on the same plan,
    by another encoder, a decode with the header walk inside the launch, a decode behind a parallel walk and
    drx_estimate_words.  The tour (CS.route_tour) runs here and satisfies all of this by itself, so that the test stands on
    its own; what the other tests saw is merely counted with it.  This holds the ROUTES the tour names to the library's
    dispatch; it does not say which routes the pairs and the sessions reach."""
    geoms, steps = CS.route_tour()
    Runner(ctx, geoms).run_all(steps)
    assert ROUTES["enc"] == {1, 2, 3, 4, 5, 6}, ROUTES["enc"]
    every = (D.PATH_LANES_FUSED | D.PATH_LANES | D.PATH_BLOCKS | D.PATH_LONG | D.PATH_SIMPLE | D.PATH_IIR | D.PATH_IIR_FUSED |
             D.PATH_SELECT | D.PATH_GATHER)
    assert ROUTES["path"] == every, (ROUTES["path"], every)
    want = {"another encoder", "fused-walk decode", "parallel-walk decode", "estimate"}
    assert all(ROUTES["after"].get(e, set()) >= want for e in range(1, 7)), ROUTES["after"]
