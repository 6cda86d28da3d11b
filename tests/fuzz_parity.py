#!/usr/bin/env python3
"""Randomised parity sweep on the GPU: random batch shapes (uniform and ragged), waveform lengths from 1 to
hundreds of thousands, every k, several signal kinds, general filters of 1 to 64 taps; GPU encode must equal the oracle's
bytes and GPU decode (default path and the variants a shape can take) must return the input; a random selection of each
batch's waveforms goes through drx_decode_select and drx_gather_encoded, against the same input and the oracle's bytes.
usage: python tests/fuzz_parity.py [cases] [seed]   (test infrastructure: it uses the oracle)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deltarice_amd as dr  # noqa: E402
from deltarice_amd import _lib as D  # noqa: E402
from oracle import oracle as O  # noqa: E402


def data(rng, kind, n, k):
    if kind == "gauss":
        return rng.normal(0, rng.choice([1, 10, 300, 5000]), n).astype(np.int16)
    if kind == "uniform":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    if kind == "zeros":
        return np.zeros(n, np.int16)
    if kind == "ramp":
        return ((np.arange(n) * int(rng.integers(1, 4))) % 60000 - 30000).astype(np.int16)
    if kind == "pulses":
        x = rng.normal(0, 3, n)
        x += 9000 * ((np.arange(n) % int(rng.integers(50, 5000))) < int(rng.integers(1, 40)))
        return x.astype(np.int16)
    raise ValueError(kind)


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def waves(Ns, Ls):
    """-> (first sample, length) of every waveform of the batch."""
    start, length, at = [], [], 0
    for N, L in zip(Ns, Ls):
        s = np.arange(0, N, L, dtype=np.int64)
        start.append(at + s)
        length.append(np.minimum(L, N - s))
        at += N
    return np.concatenate(start), np.concatenate(length)


def pick(srng, n_waves, longest):
    """How many waveforms a case selects: up to 64, fewer of very long ones (2 M samples a list: the sweep stays a sweep)."""
    return int(srng.integers(1, max(1, min(64, n_waves, 2_000_000 // longest)) + 1))


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    scale = int(os.environ.get("DRX_FUZZ_SCALE", 1))  # multiplies the chunk-size caps (bigger, fewer cases)
    ctx = dr.Context(0)
    t0 = time.time()
    lo, hi = 0, cases
    if os.environ.get("DRX_FUZZ_ONLY"):
        lo, hi = (int(v) for v in os.environ["DRX_FUZZ_ONLY"].split(":"))
    logf = open(os.environ["DRX_FUZZ_LOG"], "a") if os.environ.get("DRX_FUZZ_LOG") else None

    def log(msg):
        if logf:
            logf.write(msg + "\n")
            logf.flush()
            os.fsync(logf.fileno())

    for it in range(cases):
        k = int(rng.integers(1, 16)) if rng.random() < 0.9 else 0
        kind = str(rng.choice(["gauss", "uniform", "zeros", "ramp", "pulses"]))
        Lc = [1, 2, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000, 2047, 2048, 2049, 7000, 8191, 8192, 8193, 16384, 40000,
              65535, 65536, 65537, 100000, 300000]
        ragged = rng.random() < 0.25
        n_chunks = int(rng.integers(1, 6))
        taps = None
        if rng.random() < 0.2:  # (ragged batches too: drx_plan_set_filter applies to every chunk)
            nt = int(rng.integers(1, 6))
            taps = [int(rng.choice([1, -1])) if rng.random() < 0.8 else int(rng.integers(2, 5))] + [int(v) for v in rng.integers(-3, 4, nt - 1)]
        if taps is not None and k != 0:
            # a third of the filtered cases: the rest of what drx_plan_set_filter accepts -- 6 to 64 taps, coefficients of the
            # whole int16 range, now and then an int32 extreme, leads that are no unit or one only modulo 2^16.  Drawn from a
            # generator of their own (as srng below): the case sequence of a seed stays what it was.  Not at k = 0: such
            # residuals are full range, and M = 1 is defined only while z < 32768.
            frng = np.random.default_rng((seed, it, 64))
            if frng.random() < 1 / 3:
                nt = int(frng.integers(6, 65))
                taps = [int(frng.choice([1, -1, 2, -2, 3, -3, 65537, -32767]))] + [int(v) for v in frng.integers(-32767, 32768, nt - 1)]
                if frng.random() < 0.25:
                    taps[int(frng.integers(1, nt))] = int(frng.choice([2 ** 31 - 1, -2 ** 31, 65536, -65537]))
        if ragged:
            Ls = [int(rng.choice(Lc)) for _ in range(n_chunks)]
            Ns = [int(min(400000 * scale, max(1, L * int(rng.integers(1, 40 * scale)) + int(rng.integers(0, L))))) for L in Ls]
        else:
            L = int(rng.choice(Lc))
            N = int(min(600000 * scale, max(1, L * int(rng.integers(1, 60 * scale)) + (int(rng.integers(0, L)) if rng.random() < 0.5 else 0))))
            Ls, Ns = [L] * n_chunks, [N] * n_chunks
        if k == 0:
            kind = "zeros" if kind == "uniform" else kind  # M = 1 is defined only while z < 32768
        x = np.concatenate([data(rng, kind, n, k) for n in Ns])
        if k == 0:
            x = (x // 4).astype(np.int16)
        label = f"case {it}: k={k} {kind} chunks={n_chunks} L={Ls} N={Ns} taps={taps}"
        if it < lo or it >= hi:
            continue
        log(label)
        try:
            # oracle stream, chunk by chunk
            words, offs, copts = [], [0], []
            pos = 0
            for n, L in zip(Ns, Ls):
                opts = (1 << k, L) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())
                w = O.encode_chunk(x[pos:pos + n], opts)
                words.append(w)
                copts.append(opts)
                offs.append(offs[-1] + w.size)
                pos += n
            ref_w = np.concatenate(words)
            ref_off = np.array(offs, np.uint64)
            if ragged:
                plan = ctx.plan(Ns, Ls, 1 << k, taps=taps)
            else:
                opts = (1 << k, Ls[0]) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())
                plan = ctx.plan_uniform(n_chunks, Ns[0], opts)
            xd = dev(ctx, x)
            # (every forcing flag takes its encoder wherever that encoder can run the batch; include/deltarice_hip.h)
            for flags in (0, D.DBG_NO_LONG_PATHS, D.DBG_NO_PIECES, D.DBG_FORCE_SEGMENTS, D.DBG_FORCE_PIECES, D.DBG_NO_WIDE_FUSED,
                          D.DBG_FORCE_STREAM_SEGS, D.DBG_FORCE_STREAM_SEGS | D.DBG_STREAM_THREE_WGS):
                for eimpl in ((2, 1, 0) if flags in (0, D.DBG_NO_LONG_PATHS) else (2,)):
                    ctx.set_option("encode_impl", eimpl)
                    # (and the persistent encoder whatever the batch's size)
                    ctx.set_option("debug_flags", flags | (D.DBG_FORCE_STREAM if eimpl == 2 and flags in (0, D.DBG_NO_LONG_PATHS) else 0))
                    log(f"  encode flags {flags} impl {eimpl}")
                    w, off = plan.encode(xd).to_numpy()
                    assert np.array_equal(off, ref_off), f"offsets (flags {flags}, encoder {eimpl})"
                    assert np.array_equal(w, ref_w), f"stream (flags {flags}, encoder {eimpl})"
            ctx.set_option("encode_impl", 2)
            enc = dr.EncodedBatch(dev(ctx, ref_w.view(np.int32)), dev(ctx, ref_off.astype(np.int64)), ref_w.size)
            lossless = taps is None or abs(taps[0]) == 1
            expect = x
            if not lossless:
                expect = np.concatenate([O.decode_chunk(ww, oo) for ww, oo in zip(words, copts)])
            # (WALK_BY_CHAINS: the chunk-wide walk by chains also for these few chunks; WALK_BY_SCAN: by reading the chunks)
            for flags, impl in ((0, 8), (D.DBG_NO_LONG_PATHS, 8), (D.DBG_LONG_NOT_BLOCKS, 8), (0, 7), (D.DBG_NO_LONG_PATHS, 7), (0, 0), (D.DBG_RAGGED_ONE_LANES_LAUNCH, 8), (D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_CHAINS, 8), (D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_SCAN, 8)):
                ctx.set_option("debug_flags", flags)
                ctx.set_option("decode_impl", impl)
                log(f"  decode flags {flags} impl {impl}")
                y = plan.decode(enc).cpu().numpy()
                assert np.array_equal(y, expect), f"decode (flags {flags}, impl {impl})"
            ctx.set_option("debug_flags", 0)
            ctx.set_option("decode_impl", 8)
            # the encoder's n_i table as a side-band (drx_decode_with_wave_words)
            log("  side-band decode")
            plan.encode(xd)
            table = plan.wave_words_device()
            y = plan.decode_with_wave_words(enc.words, enc.chunk_word_off, table, in_words=enc.total_words)
            plan.finish()
            assert np.array_equal(y.cpu().numpy(), expect), "side-band decode"
            # the one-chunk host path (what the H5Z callback runs) on the first chunk
            opts0 = (1 << k, Ls[0]) + ((len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ())
            log("  host path")
            eb = ctx.filter_chunk(x[:Ns[0]], opts0, reverse=False)
            assert eb == words[0].tobytes(), "host path encode"
            db = np.frombuffer(ctx.filter_chunk(eb, opts0, reverse=True), np.int16)
            assert np.array_equal(db, expect[:Ns[0]]), "host path decode"
            # selected waveforms: decoded alone, and regrouped without decoding (drawn from a generator of their own: the case
            # sequence of a seed does not depend on them)
            srng = np.random.default_rng((seed, it))
            start, length = waves(Ns, Ls)
            ftaps = (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps) if taps else ()
            ed = xd if lossless else dev(ctx, expect)
            sel = srng.integers(0, start.size, pick(srng, start.size, int(length.max())))
            for tab in (None, table):
                log(f"  select {sel.size} side-band {tab is not None}")
                y = plan.decode_select(enc, sel, wave_words=tab)
                assert plan.last_decode_path() == D.PATH_SELECT
                for i, g in enumerate(sel):
                    s, n = int(start[g]), int(length[g])
                    assert torch.equal(y[i, :n], ed[s:s + n]) and not bool(y[i, n:].any()), f"select row {i} (side-band {tab is not None})"
            same = np.nonzero(length == length[srng.integers(0, start.size)])[0]  # one length: any chunking of them is a batch
            gsel = srng.choice(same, pick(srng, same.size, int(length[same[0]])))
            cw = int(srng.integers(1, gsel.size + 1))
            Lg = int(length[gsel[0]])
            want = [O.encode_chunk(np.concatenate([x[start[g]:start[g] + Lg] for g in gsel[c0:c0 + cw]]), (1 << k, Lg) + ftaps)
                    for c0 in range(0, gsel.size, cw)]
            want_off = np.cumsum([0] + [w.size for w in want])
            gflags = D.DBG_GATHER_OTHER_COPY if it & 1 else 0
            ctx.set_option("debug_flags", gflags)
            for tab in (None, table):
                log(f"  gather {gsel.size} by {cw} flags {gflags} side-band {tab is not None}")
                got = plan.gather_encoded(enc, gsel, cw, wave_words=tab)
                assert plan.last_decode_path() == D.PATH_GATHER
                assert np.array_equal(got.enc.chunk_word_off.cpu().numpy(), want_off), f"gather offsets (side-band {tab is not None})"
                assert np.array_equal(got.enc.words.cpu().numpy().view(np.uint32), np.concatenate(want)), f"gather (side-band {tab is not None})"
                if not lossless:  # ... and what those bytes decode to: the oracle's decode of the source
                    gp = got.plan(ctx)
                    rows = torch.cat([ed[start[g]:start[g] + Lg] for g in gsel])
                    assert torch.equal(gp.decode(got.enc), rows), "gather, decoded"
                    gp.close()
            ctx.set_option("debug_flags", 0)
            if os.environ.get("DRX_FUZZ_CORRUPT"):
                # payload bits flipped (headers intact): any result or DRX_ERR_CORRUPT is fine, a fault is not
                bad = ref_w.copy()
                hdr = set(int(o) for o in ref_off[:-1])
                for _ in range(4):
                    j = int(rng.integers(0, bad.size))
                    if j not in hdr:
                        bad[j] ^= np.uint32(1 << int(rng.integers(0, 32)))
                encb = dr.EncodedBatch(dev(ctx, bad.view(np.int32)), dev(ctx, ref_off.astype(np.int64)), bad.size)
                for flags, impl in ((0, 8), (D.DBG_NO_LONG_PATHS, 8), (D.DBG_LONG_NOT_BLOCKS, 8), (0, 7), (0, 0), (D.DBG_NO_LONG_PATHS | D.DBG_WALK_BY_CHAINS, 8)):
                    ctx.set_option("debug_flags", flags)
                    ctx.set_option("decode_impl", impl)
                    log(f"  corrupt decode flags {flags} impl {impl}")
                    try:
                        plan.decode(encb)
                    except dr.DeltaRiceError:
                        pass
                ctx.set_option("debug_flags", 0)
                ctx.set_option("decode_impl", 8)
                # ... and through the selections (the select kernels follow no table once a walk has failed; the gather copies
                # nothing then): any rows or DRX_ERR_CORRUPT; behind an error the gather has written nothing
                for tab in (None, table):
                    log(f"  corrupt select / gather side-band {tab is not None}")
                    try:
                        plan.decode_select(encb, sel, wave_words=tab)
                    except dr.DeltaRiceError:
                        pass
                    out = torch.full((int(want_off[-1]) + 64,), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device)
                    try:
                        plan.gather_encoded(encb, gsel, cw, wave_words=tab, out_words=out)
                    except dr.DeltaRiceError:
                        assert bool((out == 0x5A5A5A5A).all()), "gather wrote behind an error"
        except Exception as e:  # noqa: BLE001
            print("FAIL", label, "->", repr(e), flush=True)
            return 1
        if it % 20 == 19:
            print(f"{it + 1} cases ok ({time.time() - t0:.0f} s)", flush=True)
    print(f"all {cases} cases ok (seed {seed}, {time.time() - t0:.0f} s)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
