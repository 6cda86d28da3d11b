"""GPU: h5io.recompress(..., taps=...) -- a dataset into a new file with every stored chunk re-coded under another prediction
filter as encoded words (drx_h5_recompress_filtered): the new file's filter options hold the new RiceParameter and the new
taps, its stored chunks are the CPU oracle's bytes for the rows under them, and it reads back as the samples."""
import numpy as np
import pytest

from test_gpu_h5io_copy import h5info  # noqa: F401 (fixture)
from test_gpu_h5io_rows import env, h5tool  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIR4 = (1, -1, 1, -1)


def cd_values(info):
    """the cd_values of filter 32025 from h5_filter_info's line: `... | id flags ncd cd...`"""
    for part in info.split(" | ")[1:]:
        f = part.split()
        if int(f[0]) == 32025:
            assert int(f[2]) == len(f) - 3
            return tuple(int(v) for v in f[3:])
    raise AssertionError(info)


def check_refiltered(ctx, h5io, h5tool, h5info, tmp_path, src, x, crows, wave_len, taps, rice_m, tag):
    from oracle import oracle as O
    rows, cols = x.shape
    n = -(-rows // crows)
    dst = tmp_path / f"re_{tag}.h5"
    st = h5io.recompress(ctx, str(src), "test", str(dst), rice_m=rice_m, taps=taps)
    assert st["n_chunks"] == n and st["raw_bytes"] == rows * cols * 2 and st["rows"] == rows and st["chunk_rows"] == crows, tag
    a, b = h5info(src, "test").split(" | "), h5info(dst, "test").split(" | ")
    assert a[0] == b[0] and len(a) == len(b), tag  # shape, chunking, element type; the same filters
    delta = tuple(taps) == (1, -1)
    tail = () if delta else (len(taps),) + tuple(t & 0xFFFFFFFF for t in taps)
    padded = np.zeros((n * crows, cols), np.int16)
    padded[:rows] = x
    if rice_m is None:  # the smallest dataset among the sixteen, by the oracle's count; on a tie the smaller parameter
        sizes = [sum(O.encode_chunk(padded[c * crows:(c + 1) * crows], (1 << k, wave_len) + tail).size for c in range(n)) for k in range(16)]
        rice_m = 1 << int(np.argmin(sizes))
    opts = (rice_m, wave_len) + tail
    assert cd_values(h5info(dst, "test")) == opts, tag  # the new RiceParameter and taps; a delta target: the two-value form
    # its stored chunks: the oracle's bytes for the rows under the new options (a last chunk padded with the fill value)
    assert int(h5tool("chunks", dst, tmp_path / f"dst_{tag}").stdout) == n, tag
    for c in range(n):
        got = np.fromfile(f"{tmp_path}/dst_{tag}.{c}", np.uint32)
        assert got.tobytes() == O.encode_chunk(padded[c * crows:(c + 1) * crows], opts).tobytes(), (tag, c)
    # the new file read back
    y = torch.empty(x.size, dtype=torch.int16, device=ctx.device)
    h5io.read(ctx, str(dst), "test", y)
    assert y.cpu().numpy().tobytes() == x.tobytes(), tag
    return rice_m, dst


def test_refilter_a_delta_dataset(env, h5tool, h5info, tmp_path):  # noqa: F811
    import deltarice_amd as dr
    ctx, h5io = env
    rows, cols, crows = 330, 1000, 100  # 4 chunks of 100 x 1000, the last one of 30 rows and padding
    x = np.random.default_rng(330).normal(0, 10, (rows, cols)).astype(np.int16)
    f = tmp_path / "delta.h5"
    h5io.write(ctx, str(f), "test", torch.from_numpy(x.reshape(-1)).to(ctx.device), rows, cols, crows, 8, cols)
    assert cd_values(h5info(f, "test")) == (8, cols)
    m, _ = check_refiltered(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, cols, FIR4, 16, "fir4_m16")
    assert m == 16
    best, dst = check_refiltered(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, cols, FIR4, None, "fir4_best")
    assert best in (8, 16, 32)  # (white noise of sigma 10 under [1,-1,1,-1]: residuals of sigma 20)
    # ... and back: a delta target stores the two-value form, and a 5-tap target takes the serial kernels
    check_refiltered(ctx, h5io, h5tool, h5info, tmp_path, dst, x, crows, cols, (1, -1), 8, "back_to_delta")
    check_refiltered(ctx, h5io, h5tool, h5info, tmp_path, dst, x, crows, cols, (1, -1, 1, -1, 1), 16, "fir5")
    # arguments
    for bad in ((0, 1), (1,) * 65):
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.recompress(ctx, str(f), "test", str(tmp_path / "bad.h5"), taps=bad)
        assert e.value.status == 1 and not (tmp_path / "bad.h5").exists()


def test_refilter_to_a_dataset_that_cannot_be_created(env, h5tool, h5info, tmp_path):  # noqa: F811
    """H5Dcreate2 refuses a name under a group that does not exist: by then the destination file has been created."""
    import deltarice_amd as dr
    from test_gpu_h5io_rows import small_file
    ctx, h5io = env
    src, x = small_file(h5tool, tmp_path)
    before = src.read_bytes()
    for rice_m, tag in ((16, "m16"), (None, "best")):
        dst = tmp_path / f"re_{tag}.h5"  # (the file check_refiltered then writes)
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.recompress(ctx, str(src), "test", str(dst), dst_name="nogroup/x", rice_m=rice_m, taps=FIR4)
        assert e.value.status == 1 and not dst.exists()
        assert src.read_bytes() == before
        check_refiltered(ctx, h5io, h5tool, h5info, tmp_path, src, x, 4, 500, FIR4, rice_m, tag)
