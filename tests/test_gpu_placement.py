"""Where the caller's buffers lie: every codec route of tests/test_gpu_routes.py with its buffers at each 16-byte phase,
guarded by sentinels and filled with hostile data before the call.

The ABI (include/deltarice_hip.h) promises any alignment of the element type, no write outside [ptr, ptr + n), and results
that depend neither on what an output held before the call nor on the words outside [0, in_words).  A torch allocation is
512-byte aligned, starts zeroed more often than not and has unchecked slack behind it, so the other tests never leave those
safe conditions.  Here every buffer is a view `window()` cuts out of a larger tensor: 4 KiB of sentinel on each side, so a
stray access lands in the test's own allocation, and a check on the device says whether the sentinels are intact.  Every
cell asserts the route it took, so no cell quietly runs the aligned case's kernel."""
import numpy as np
import pytest

from deltarice_amd import _lib as D
from test_gpu_routes import BATCHES, EXPECTED, FLAGS, make_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096  # bytes of sentinel on each side of a window (a multiple of 16: the view keeps its byte offset's phase)
G16, G32, G64 = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
FF = -1  # 0xFFFFFFFF as int32: the worst word for a unary parse

# byte offset of each buffer from a 16-byte boundary.  Across the set the int16 samples sit at 0, 2, 6 and 14 mod 16 and the
# words at 0, 4, 8 and 12; chunk_word_off is 8 bytes off twice.
PLACEMENTS = {
    "aligned": dict(x=0, w=0, off=0, y=0),
    "misaligned": dict(x=2, w=4, off=8, y=14),
    "x6-w8": dict(x=6, w=8, off=0, y=6),
    "x14-w12": dict(x=14, w=12, off=8, y=2),
}
# the two 58.8 M-sample batches: the control and the all-misaligned placement
BIG = {"stream-quiet", "stream-loud"}
ENC_ONLY = (D.DBG_NO_PIECES | D.DBG_FORCE_SEGMENTS | D.DBG_FORCE_PIECES | D.DBG_NO_WIDE_FUSED | D.DBG_FORCE_STREAM |
            D.DBG_FORCE_STREAM_SEGS | D.DBG_STREAM_THREE_WGS)
DEC_FLAGS = tuple(f for f in FLAGS if not f & ENC_ONLY)  # walk forms, parallel walks, long paths, IIR, ragged launches
DEC_IMPLS = (0, 7, 8)
SLACK = 67  # words of 0xFFFFFFFF behind the stream in a decode's input window


class Window:
    """A view of n elements at byte_offset past a 16-byte boundary inside a larger tensor, sentinels on both sides."""

    def __init__(self, device, n, dtype, byte_offset, fill=None, guard=(0, 0)):
        es = torch.empty(0, dtype=dtype).element_size()
        assert byte_offset % es == 0, (byte_offset, dtype)
        self.front, self.back = guard
        self.lo = (GUARD + byte_offset) // es
        self.hi = self.lo + n
        self.base = torch.empty(self.hi + GUARD // es, dtype=dtype, device=device)
        assert self.base.data_ptr() % 16 == 0
        self.base[:self.lo].fill_(self.front)
        self.base[self.hi:].fill_(self.back)
        self.t = self.base[self.lo:self.hi]
        assert self.t.data_ptr() % 16 == byte_offset % 16
        if fill is not None:
            self.t.fill_(fill)

    def intact(self) -> bool:
        return bool(((self.base[:self.lo] == self.front).all() & (self.base[self.hi:] == self.back).all()).item())


def window(n, dtype, byte_offset, fill=None, guard=None, device="cuda"):
    g = {torch.int16: G16, torch.int32: G32, torch.int64: G64}[dtype] if guard is None else guard
    return Window(torch.device(device), n, dtype, byte_offset, fill, g if isinstance(g, tuple) else (g, g))


def placements(name):
    return [p for p in PLACEMENTS if name not in BIG or p in ("aligned", "misaligned")]


def encoder_cells(name):
    """{DRX_ENC_*: (encode_impl, debug_flags)}: the first cell of EXPECTED that reaches each distinct encoder."""
    cells = {}
    for eimpl, line in EXPECTED[name].items():
        for flags, cell in zip(FLAGS, line.split()):
            cells.setdefault(int(cell.split("/")[0]), (eimpl, flags))
    return cells


class Batch:
    def __init__(self, ctx, name):
        from oracle import oracle as O
        Ns, Ls, m, taps, sigma = BATCHES[name]
        self.name, self.ctx, self.Ns = name, ctx, Ns
        rng = np.random.default_rng(sum(map(ord, name)))
        x = rng.normal(0, sigma, sum(Ns)).astype(np.int16)
        ftaps = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()
        words, offs, at = [], [0], 0
        for N, L in zip(Ns, Ls):
            w = O.encode_chunk(x[at:at + N], ((m, L) if L else (m,)) + ftaps)
            words.append(w)
            offs.append(offs[-1] + w.size)
            at += N
        self.total = offs[-1]
        self.xd = torch.from_numpy(x).to(ctx.device)
        self.ref_w = torch.from_numpy(np.concatenate(words).view(np.int32)).to(ctx.device)
        self.ref_off = torch.tensor(offs, dtype=torch.int64, device=ctx.device)
        self.plan = make_plan(ctx, Ns, Ls, m, taps)
        self.plan.encode(self.xd)  # (the next encodes see the code length this one measured, as test_routes' cells do)


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=list(BATCHES))
def batch(request, ctx):
    b = Batch(ctx, request.param)
    yield b
    b.plan.close()
    ctx.set_option("debug_flags", 0)
    ctx.set_option("encode_impl", 2)
    ctx.set_option("decode_impl", 8)


def run(ctx, plan, launch):
    """Orders the launch behind the fills on torch's stream, waits, raises on device-side errors."""
    ctx.stream.wait_stream(torch.cuda.current_stream(ctx.device))
    launch()
    return plan.finish()


def test_encode_placements(ctx, batch):
    b, plan = batch, batch.plan
    n_off = len(b.Ns) + 1
    est = None
    try:
        for pname in placements(b.name):
            P = PLACEMENTS[pname]
            xw = window(plan.total_samples, torch.int16, P["x"], guard=(0x7FFF, -0x8000), device=ctx.device)
            xw.t.copy_(b.xd)
            e = plan.estimate_words(xw.t)
            est = e if est is None else est
            assert np.array_equal(e, est), (b.name, pname, "estimate_words")
            ww = window(plan.max_encoded_words, torch.int32, P["w"], device=ctx.device)
            ow = window(n_off, torch.int64, P["off"], device=ctx.device)
            for enc, (eimpl, flags) in encoder_cells(b.name).items():
                cell = (b.name, pname, enc, eimpl, flags)
                ctx.set_option("encode_impl", eimpl)
                ctx.set_option("debug_flags", flags)
                ww.t.fill_(FF)
                ow.t.fill_(-1)
                total = run(ctx, plan, lambda: plan.encode_async(xw.t, ww.t, ow.t))
                assert plan.last_encode_path() == enc, cell
                assert total == b.total, cell
                assert torch.equal(ow.t, b.ref_off) and torch.equal(ww.t[:total], b.ref_w), cell
                assert ww.intact() and ow.intact() and xw.intact(), cell
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("encode_impl", 2)


def test_encode_capacity_boundary(ctx, batch):
    """Every encoder: a buffer of exactly the encoded size suffices; one word less is DRX_ERR_CAPACITY and nothing lands
    behind it; the plan then encodes correctly again."""
    import deltarice_amd as dr
    b, plan = batch, batch.plan
    P = PLACEMENTS["misaligned"]
    n_off = len(b.Ns) + 1
    xw = window(plan.total_samples, torch.int16, P["x"], guard=(0x7FFF, -0x8000), device=ctx.device)
    xw.t.copy_(b.xd)
    ow = window(n_off, torch.int64, P["off"], device=ctx.device)
    exact = window(b.total, torch.int32, P["w"], device=ctx.device)
    short = window(b.total - 1, torch.int32, P["w"], device=ctx.device)
    try:
        for enc, (eimpl, flags) in encoder_cells(b.name).items():
            cell = (b.name, enc, eimpl, flags)
            ctx.set_option("encode_impl", eimpl)
            ctx.set_option("debug_flags", flags)
            for again in (False, True):
                exact.t.fill_(FF)
                ow.t.fill_(-1)
                assert run(ctx, plan, lambda: plan.encode_async(xw.t, exact.t, ow.t)) == b.total, cell
                assert plan.last_encode_path() == enc, cell
                assert torch.equal(ow.t, b.ref_off) and torch.equal(exact.t, b.ref_w), cell
                assert exact.intact() and ow.intact(), cell
                if again:
                    break
                short.t.fill_(FF)
                with pytest.raises(dr.DeltaRiceError) as ei:
                    run(ctx, plan, lambda: plan.encode_async(xw.t, short.t, ow.t))
                assert ei.value.status == 3, cell
                assert plan.last_encode_path() == enc, cell
                assert short.intact() and ow.intact(), cell
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("encode_impl", 2)


def test_decode_placements(ctx, batch):
    b, plan = batch, batch.plan
    n_off = len(b.Ns) + 1
    paths = {}
    try:
        for pname in placements(b.name):
            P = PLACEMENTS[pname]
            # the stream with 0xFFFFFFFF right in front of it and behind it
            ww = window(b.total + SLACK, torch.int32, P["w"], fill=FF, guard=FF, device=ctx.device)
            ww.t[:b.total].copy_(b.ref_w)
            ow = window(n_off, torch.int64, P["off"], device=ctx.device)
            ow.t.copy_(b.ref_off)
            yw = window(plan.total_samples, torch.int16, P["y"], device=ctx.device)
            for flags in DEC_FLAGS:
                ctx.set_option("debug_flags", flags)
                for impl in DEC_IMPLS:
                    ctx.set_option("decode_impl", impl)
                    cell = (b.name, pname, flags, impl)
                    for in_words in ((b.total, b.total + SLACK) if pname == "misaligned" else (b.total,)):
                        yw.t.fill_(0x7FFF)
                        run(ctx, plan, lambda: plan.decode_async(ww.t, ow.t, yw.t, in_words=in_words))
                        path = plan.last_decode_path()
                        assert paths.setdefault((flags, impl), path) == path, (cell, in_words, path)
                        same, intact = torch.equal(yw.t, b.xd), yw.intact() and ow.intact() and ww.intact()
                        assert same and intact, (cell, in_words, "samples differ" * (not same), "guard written" * (not intact))
            if pname == "misaligned":
                # the side-band decode, its wave_words table 4 bytes off (the n_i an encode of the same samples leaves)
                ctx.set_option("debug_flags", 0)
                ctx.set_option("decode_impl", 8)
                plan.encode(b.xd)
                tab = window(plan.total_waves, torch.int32, 4, device=ctx.device)
                tab.t.copy_(torch.from_numpy(plan.wave_words().view(np.int32)))
                yw.t.fill_(0x7FFF)
                run(ctx, plan, lambda: plan.decode_with_wave_words(ww.t, ow.t, tab.t, out=yw.t, in_words=b.total))
                assert torch.equal(yw.t, b.xd), (b.name, "side-band")
                assert yw.intact() and tab.intact(), (b.name, "side-band")
    finally:
        ctx.set_option("debug_flags", 0)
        ctx.set_option("decode_impl", 8)
