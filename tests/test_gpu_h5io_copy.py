"""GPU: h5io.copy_rows -- dataset rows of one file into a new file, regrouped as encoded words (drx_h5_copy_rows): the new
file reads back as x[rows], its stored chunks are the CPU oracle's bytes for those rows, and its filter settings are the
source's."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_h5io_rows import HDF5_DIR, ROOT, env, h5tool, row_sets  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def h5info(tmp_path_factory):
    d = tmp_path_factory.mktemp("h5info")
    exe = str(d / "h5_filter_info")
    subprocess.run(["gcc", "-O1", "-o", exe, os.path.join(ROOT, "tests", "h5_filter_info.c"),
                    f"-I{HDF5_DIR}/include", f"-L{HDF5_DIR}/lib", "-lhdf5", f"-Wl,-rpath,{HDF5_DIR}/lib"], check=True)
    return lambda path, name: subprocess.run([exe, str(path), name], check=True, capture_output=True, text=True).stdout.strip()


def check_copies(ctx, h5io, h5tool, h5info, tmp_path, src, x, crows, opts, dst_chunk_rows):
    from oracle import oracle as O
    rows, cols = x.shape
    n_src = int(h5tool("chunks", src, tmp_path / "src").stdout)
    stored = [os.path.getsize(f"{tmp_path}/src.{c}") for c in range(n_src)]
    src_info = h5info(src, "test")
    for name, sel in row_sets(rows, crows, np.random.default_rng(rows)).items():
        for dcr in dst_chunk_rows:
            dcr = crows if dcr is None else dcr
            if dcr > len(sel):
                continue
            dst = tmp_path / f"copy_{name}_{dcr}.h5"
            st = h5io.copy_rows(ctx, str(src), "test", sel, str(dst), chunk_rows=None if dcr == crows and crows <= len(sel) else dcr)
            cell = (name, dcr)
            touched = sorted({r // crows for r in sel})
            assert st["n_chunks"] == len(touched), cell                      # only the fetched chunks are counted
            assert st["stored_bytes"] == sum(stored[c] for c in touched), cell
            assert st["raw_bytes"] == len(sel) * cols * 2 and st["rows"] == len(sel) and st["chunk_rows"] == dcr, cell
            # the new file read back
            want = x[np.array(sel)]
            y = torch.empty(want.size, dtype=torch.int16, device=ctx.device)
            h5io.read(ctx, str(dst), "test", y)
            assert np.array_equal(y.cpu().numpy().reshape(want.shape), want), cell
            # its stored chunks: the oracle's bytes for those rows (a last chunk padded with the fill value)
            n_dst = int(h5tool("chunks", dst, tmp_path / "dst").stdout)
            assert n_dst == -(-len(sel) // dcr), cell
            padded = np.zeros((n_dst * dcr, cols), np.int16)
            padded[:len(sel)] = want
            for c in range(n_dst):
                got = np.fromfile(f"{tmp_path}/dst.{c}", np.uint32)
                assert got.tobytes() == O.encode_chunk(padded[c * dcr:(c + 1) * dcr], opts).tobytes(), (cell, c)
            # shape, element type and filter settings: the source's, but for the rows and the chunk rows
            a, b = src_info.split(" | "), h5info(dst, "test").split(" | ")
            assert a[1:] == b[1:], cell                                       # filter id, flags, cd_values verbatim
            assert b[0].split() == [str(len(sel)), str(cols), str(dcr), str(cols)] + a[0].split()[4:], cell


@pytest.mark.parametrize("rows", [4000, 3930], ids=["whole-chunks", "padded-last-chunk"])
def test_copy_rows_of_a_directly_written_file(env, h5tool, h5info, tmp_path, rows):
    ctx, h5io = env
    cols, crows = 7000, 200  # 20 chunks of 200 x 7000
    x = np.random.default_rng(rows).normal(0, 10, (rows, cols)).astype(np.int16)
    f = tmp_path / "direct.h5"
    h5io.write(ctx, str(f), "test", torch.from_numpy(x.reshape(-1)).to(ctx.device), rows, cols, crows, 8, cols)
    check_copies(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, (8, cols), (None, 1, 3, 64))


def test_copy_rows_of_a_file_with_a_general_filter(env, h5tool, h5info, tmp_path):
    ctx, h5io = env
    rows, cols, crows, taps = 330, 3000, 50, (1, -1, 1, -1, 1)  # five taps, two waveforms per row, a padded last chunk
    x = np.random.default_rng(330).normal(0, 30, (rows, cols)).astype(np.int16)
    f = tmp_path / "fir5.h5"
    h5io.write(ctx, str(f), "test", torch.from_numpy(x.reshape(-1)).to(ctx.device), rows, cols, crows, 16, 1500, taps=taps)
    opts = (16, 1500, 5) + tuple(t & 0xFFFFFFFF for t in taps)
    check_copies(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, opts, (None, 7))


def test_copy_rows_of_a_file_the_cpu_oracle_encoded(env, h5tool, h5info, tmp_path):
    from oracle import oracle as O
    ctx, h5io = env
    rows, cols, crows, M, L = 203, 4096, 20, 16, 1024  # four waveforms per row, a padded last chunk
    x = np.random.default_rng(203).normal(0, 25, (rows, cols)).astype(np.int16)
    n = -(-rows // crows)
    xp = np.zeros((n * crows, cols), np.int16)
    xp[:rows] = x
    for c in range(n):
        O.encode_chunk(xp[c * crows:(c + 1) * crows], (M, L)).tofile(f"{tmp_path}/cpu.{c}")
    f = tmp_path / "cpu.h5"
    h5tool("writeraw", f, rows, cols, crows, M, L, tmp_path / "cpu")
    check_copies(ctx, h5io, h5tool, h5info, tmp_path, f, x, crows, (M, L), (None, 1, 9))


def test_copy_rows_refusals(env, h5tool, tmp_path):
    import deltarice_amd as dr
    ctx, h5io = env
    x = np.random.default_rng(4).normal(0, 10, (16, 1000)).astype(np.int16)
    raw = tmp_path / "raw.bin"
    x.tofile(raw)
    good = tmp_path / "L500.h5"
    h5tool("write", good, raw, 16, 1000, 4, 8, 500)
    before = good.read_bytes()
    for dst in (good, os.path.join(str(tmp_path), ".", "L500.h5")):  # the source itself, under either spelling
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.copy_rows(ctx, str(good), "test", [1, 2], str(dst))
        assert e.value.status == 1
    assert good.read_bytes() == before
    for rows_, cr in (([0, 16], 1), ([], 1), ([1, 2], 3)):  # a row past the end, no rows, chunk rows above the rows
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.copy_rows(ctx, str(good), "test", rows_, str(tmp_path / "out.h5"), chunk_rows=cr)
        assert e.value.status == 1, (rows_, cr)
    for L, name in ((300, "L300.h5"), (4000, "L4000.h5")):  # cols % WaveformLength != 0: waveforms straddle rows
        f = tmp_path / name
        h5tool("write", f, raw, 16, 1000, 4, 8, L)
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.copy_rows(ctx, str(f), "test", [1], str(tmp_path / "out.h5"))
        assert e.value.status == 5
    h5io.copy_rows(ctx, str(good), "test", [5, 1, 5], str(tmp_path / "out.h5"), dst_name="picked", chunk_rows=2)
    st = h5io.copy_rows(ctx, str(good), "test", [5, 1], str(tmp_path / "out2.h5"))  # None: the source's 4 rows, but only 2 exist
    assert st["chunk_rows"] == 2 and st["rows"] == 2


def check_small_copy(ctx, h5io, h5tool, h5info, tmp_path, src, x, sel, dcr, dst):
    """what check_copies holds a copy to, for the rows sel of small_file's dataset in chunks of dcr rows"""
    from oracle import oracle as O
    st = h5io.copy_rows(ctx, str(src), "test", sel, str(dst), chunk_rows=dcr)
    assert st["n_chunks"] == len({r // 4 for r in sel}) and st["rows"] == len(sel) and st["chunk_rows"] == dcr
    want = x[np.array(sel)]
    y = torch.empty(want.size, dtype=torch.int16, device=ctx.device)
    h5io.read(ctx, str(dst), "test", y)
    assert np.array_equal(y.cpu().numpy().reshape(want.shape), want)
    n_dst = int(h5tool("chunks", dst, tmp_path / "dst").stdout)
    assert n_dst == -(-len(sel) // dcr)
    padded = np.zeros((n_dst * dcr, 1000), np.int16)
    padded[:len(sel)] = want
    for c in range(n_dst):
        got = np.fromfile(f"{tmp_path}/dst.{c}", np.uint32)
        assert got.tobytes() == O.encode_chunk(padded[c * dcr:(c + 1) * dcr], (8, 500)).tobytes(), c
    a, b = h5info(src, "test").split(" | "), h5info(dst, "test").split(" | ")
    assert a[1:] == b[1:]
    assert b[0].split() == [str(len(sel)), "1000", str(dcr), "1000"] + a[0].split()[4:]


def test_copy_rows_to_a_dataset_that_cannot_be_created(env, h5tool, h5info, tmp_path):
    """H5Dcreate2 refuses a name under a group that does not exist: by then the destination file has been created."""
    import deltarice_amd as dr
    from test_gpu_h5io_rows import small_file
    ctx, h5io = env
    src, x = small_file(h5tool, tmp_path)
    before = src.read_bytes()
    dst = tmp_path / "copy.h5"
    for sel, dcr in (([5, 1, 9, 9], 2), ([5, 1, 9], 2)):  # whole chunks; a padded last chunk
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.copy_rows(ctx, str(src), "test", sel, str(dst), dst_name="nogroup/x", chunk_rows=dcr)
        assert e.value.status == 1 and not dst.exists()
        assert src.read_bytes() == before
        check_small_copy(ctx, h5io, h5tool, h5info, tmp_path, src, x, sel, dcr, dst)  # the same context, the same file name
        dst.unlink()


def test_copy_rows_out_of_a_damaged_chunk(env, h5tool, h5info, tmp_path):
    import deltarice_amd as dr
    from test_gpu_h5io_rows import small_file
    ctx, h5io = env
    src, x = small_file(h5tool, tmp_path, damaged_chunk=2)  # rows 8 .. 11
    dst = tmp_path / "copy.h5"
    with pytest.raises(dr.DeltaRiceError) as e:  # two whole chunks of sound rows, the padded last chunk out of the damaged one
        h5io.copy_rows(ctx, str(src), "test", [0, 1, 4, 5, 9], str(dst), chunk_rows=2)
    assert e.value.status == 4 and not dst.exists()
    with pytest.raises(dr.DeltaRiceError) as e:  # ... and a whole chunk out of it
        h5io.copy_rows(ctx, str(src), "test", [0, 9], str(dst), chunk_rows=2)
    assert e.value.status == 4 and not dst.exists()
    check_small_copy(ctx, h5io, h5tool, h5info, tmp_path, src, x, [0, 1, 4, 5, 13], 2, dst)  # the other chunks: neither read nor validated
