"""GPU: h5io.recompress -- a dataset into a new file with every stored chunk re-coded at another RiceParameter as encoded
words (drx_h5_recompress): the new file reads back as x, its stored chunks are the CPU oracle's bytes at the new parameter,
and its shape, element type and filter settings are the source's except cd_values[0]."""
import os

import numpy as np
import pytest

from test_gpu_h5io_copy import h5info  # noqa: F401 (fixture)
from test_gpu_h5io_rows import env, h5tool  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, src, x, crows, opts, rice_m, tag):
    """opts: the source's compression_opts; rice_m: the target, None for the best -> the RiceParameter of the new file."""
    from oracle import oracle as O
    rows, cols = x.shape
    n = int(h5tool("chunks", src, tmp_path / "src").stdout)
    stored = sum(os.path.getsize(f"{tmp_path}/src.{c}") for c in range(n))
    dst = tmp_path / f"re_{tag}.h5"
    st = h5io.recompress(ctx, str(src), "test", str(dst), rice_m=rice_m)
    assert st["n_chunks"] == n == -(-rows // crows) and st["stored_bytes"] == stored, tag  # what was fetched
    assert st["raw_bytes"] == rows * cols * 2 and st["rows"] == rows and st["chunk_rows"] == crows, tag
    # shape, element type, chunking and filter settings: the source's, but for cd_values[0]
    a, b = h5info(src, "test").split(" | "), h5info(dst, "test").split(" | ")
    assert a[0] == b[0], tag
    diff = [(i, p, q) for i, (p, q) in enumerate(zip(a[1].split(), b[1].split())) if p != q]
    assert len(a[1].split()) == len(b[1].split()) and a[2:] == b[2:], tag
    padded = np.zeros((n * crows, cols), np.int16)
    padded[:rows] = x
    if rice_m is None:  # the smallest dataset among the sixteen, by the oracle's count; on a tie the smaller parameter
        sizes = [sum(O.encode_chunk(padded[c * crows:(c + 1) * crows], (1 << k,) + tuple(opts[1:])).size for c in range(n)) for k in range(16)]
        rice_m = 1 << int(np.argmin(sizes))
    assert len(diff) <= 1 and all(p == str(opts[0]) and q == str(rice_m) for _, p, q in diff), (tag, diff)
    assert (len(diff) == 1) == (rice_m != opts[0]), (tag, diff)
    # the new file read back
    y = torch.empty(x.size, dtype=torch.int16, device=ctx.device)
    h5io.read(ctx, str(dst), "test", y)
    assert y.cpu().numpy().tobytes() == x.tobytes(), tag
    # its stored chunks: the oracle's bytes at the new parameter (a last chunk padded with the fill value)
    assert int(h5tool("chunks", dst, tmp_path / "dst").stdout) == n, tag
    for c in range(n):
        got = np.fromfile(f"{tmp_path}/dst.{c}", np.uint32)
        assert got.tobytes() == O.encode_chunk(padded[c * crows:(c + 1) * crows], (rice_m,) + tuple(opts[1:])).tobytes(), (tag, c)
    return rice_m


def test_recompress_a_directly_written_file(env, h5tool, h5info, tmp_path):  # noqa: F811
    import deltarice_amd as dr
    ctx, h5io = env
    rows, cols, crows = 4000, 7000, 200  # 20 chunks of 200 x 7000
    x = np.random.default_rng(4000).normal(0, 10, (rows, cols)).astype(np.int16)
    f = tmp_path / "direct.h5"
    h5io.write(ctx, str(f), "test", torch.from_numpy(x.reshape(-1)).to(ctx.device), rows, cols, crows, 8, cols)
    assert check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, (8, cols), 16, "m16") == 16
    best = check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, (8, cols), None, "best")
    assert best in (4, 8, 16)  # (sigma = 10: a few bits of remainder)
    # the source itself, under either spelling, and a RiceParameter that is none
    before = f.read_bytes()
    for dst in (f, os.path.join(str(tmp_path), ".", "direct.h5")):
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.recompress(ctx, str(f), "test", str(dst), rice_m=16)
        assert e.value.status == 1
    assert f.read_bytes() == before
    with pytest.raises(dr.DeltaRiceError) as e:
        h5io.recompress(ctx, str(f), "test", str(tmp_path / "bad.h5"), rice_m=12)
    assert e.value.status == 1 and not (tmp_path / "bad.h5").exists()


def test_recompress_to_a_dataset_that_cannot_be_created(env, h5tool, h5info, tmp_path):  # noqa: F811
    """H5Dcreate2 refuses a name under a group that does not exist: by then the destination file has been created."""
    import deltarice_amd as dr
    from test_gpu_h5io_rows import small_file
    ctx, h5io = env
    src, x = small_file(h5tool, tmp_path)
    before = src.read_bytes()
    for rice_m, tag in ((16, "m16"), (None, "best")):
        dst = tmp_path / f"re_{tag}.h5"  # (the file check_recompressed then writes)
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.recompress(ctx, str(src), "test", str(dst), dst_name="nogroup/x", rice_m=rice_m)
        assert e.value.status == 1 and not dst.exists()
        assert src.read_bytes() == before
        check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, src, x, 4, (8, 500), rice_m, tag)


def test_recompress_a_damaged_chunk(env, h5tool, h5info, tmp_path):  # noqa: F811
    import deltarice_amd as dr
    from test_gpu_h5io_rows import small_file
    ctx, h5io = env
    src, _ = small_file(h5tool, tmp_path, damaged_chunk=2)
    for kw in ({"rice_m": 16}, {"rice_m": None}, {"rice_m": 16, "taps": (1, -1, 1, -1)}):
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.recompress(ctx, str(src), "test", str(tmp_path / "re.h5"), **kw)
        assert e.value.status == 4 and not (tmp_path / "re.h5").exists(), kw
    good, x = small_file(h5tool, tmp_path, name="sound.h5")  # the context after the refusals
    check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, good, x, 4, (8, 500), 32, "after")


def test_recompress_a_dataset_stored_with_default_options(env, h5tool, h5info, tmp_path):  # noqa: F811
    """No cd_values at all (RiceParameter 8, the whole chunk one waveform): the new dataset names its RiceParameter alone."""
    from oracle import oracle as O
    ctx, h5io = env
    x = np.random.default_rng(5).normal(0, 40, (16, 1000)).astype(np.int16)
    raw, src, dst = tmp_path / "raw.bin", tmp_path / "default.h5", tmp_path / "re.h5"
    x.tofile(raw)
    h5tool("write", src, raw, 16, 1000, 4)
    a = h5info(src, "test").split(" | ")
    assert a[1].split()[2:] == ["0"]
    sizes = [sum(O.encode_chunk(x[c * 4:(c + 1) * 4], (1 << k,)).size for c in range(4)) for k in range(16)]
    m = 1 << int(np.argmin(sizes))
    assert m != 8  # (sigma 40: the default is not the best)
    st = h5io.recompress(ctx, str(src), "test", str(dst))
    assert st["n_chunks"] == 4 and st["rows"] == 16 and st["chunk_rows"] == 4 and st["raw_bytes"] == x.nbytes
    b = h5info(dst, "test").split(" | ")
    assert a[0] == b[0] and b[1].split() == a[1].split()[:2] + ["1", str(m)]
    assert int(h5tool("chunks", dst, tmp_path / "dst").stdout) == 4
    for c in range(4):
        assert np.fromfile(f"{tmp_path}/dst.{c}", np.uint32).tobytes() == O.encode_chunk(x[c * 4:(c + 1) * 4], (m,)).tobytes(), c
    y = torch.empty(x.size, dtype=torch.int16, device=ctx.device)
    h5io.read(ctx, str(dst), "test", y)
    assert y.cpu().numpy().tobytes() == x.tobytes()


def test_recompress_keeps_a_general_filter(env, h5tool, h5info, tmp_path):  # noqa: F811
    ctx, h5io = env
    rows, cols, crows, taps = 330, 3000, 50, (1, -1, 1, -1)  # two waveforms per row, a padded last chunk
    x = np.random.default_rng(330).normal(0, 30, (rows, cols)).astype(np.int16)
    f = tmp_path / "fir4.h5"
    h5io.write(ctx, str(f), "test", torch.from_numpy(x.reshape(-1)).to(ctx.device), rows, cols, crows, 8, 1500, taps=taps)
    opts = (8, 1500, 4) + tuple(t & 0xFFFFFFFF for t in taps)
    check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, opts, 64, "fir4-m64")
    check_recompressed(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, opts, None, "fir4-best")
