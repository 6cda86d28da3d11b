"""GPU: h5io.read_rows -- dataset rows out of a file, fetching only the chunks they lie in (drx_h5_read_rows)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDF5_DIR = os.environ.get("HDF5_DIR", "/opt/conda")


@pytest.fixture(scope="module")
def env():
    import deltarice_amd as dr
    from deltarice_amd import h5io
    if not os.path.exists(h5io.H5IO_PATH):
        pytest.skip("libdeltarice_h5io.so not built (no HDF5 C library?)")
    c = dr.Context(0)
    yield c, h5io
    c.close()


@pytest.fixture(scope="module")
def h5tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("h5tool")
    exe = str(d / "h5_roundtrip")
    subprocess.run(["gcc", "-O1", "-o", exe, os.path.join(ROOT, "tests", "h5_roundtrip.c"),
                    f"-I{HDF5_DIR}/include", f"-L{HDF5_DIR}/lib", "-lhdf5", f"-Wl,-rpath,{HDF5_DIR}/lib"], check=True)
    e = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(ROOT, "deltarice_amd", "plugin"))
    return lambda *a: subprocess.run([exe, *map(str, a)], env=e, check=True, capture_output=True, text=True)


def row_sets(rows, crows, rng):
    """rows lying in 1, 3 and all chunks (any order, a duplicate among them)"""
    n_chunks = -(-rows // crows)
    last = rows - 1
    one = [crows + 3, crows, crows + 3, 2 * crows - 1]
    three = [last, 5, crows * 7 + 1, 6, last - 1]
    every = rng.permutation(rows)[:max(rows // 2, n_chunks * 4)].tolist() + [c * crows for c in range(n_chunks)]
    return {"one": one, "three": three, "all": every}


def small_file(h5tool, tmp_path, name="small.h5", damaged_chunk=None):
    """16 x 1000 int16 in chunks of 4 rows, RiceParameter 8, WaveformLength 500, its four chunks the CPU oracle's bytes
    (H5Dwrite_chunk) -> (path, x).  damaged_chunk: that chunk with ONE word changed, the length header n_i of its second
    waveform plus one (tests/call_sequences.py's "n_plus"): the header chain no longer ends at the chunk's end, which every
    call that walks the chunk must answer with DRX_ERR_CORRUPT (a changed code word may decode to anything)."""
    from oracle import oracle as O
    x = np.random.default_rng(16).normal(0, 10, (16, 1000)).astype(np.int16)
    prefix = tmp_path / (name + ".chunk")
    for c in range(4):
        w = O.encode_chunk(x[c * 4:(c + 1) * 4], (8, 500))
        if c == damaged_chunk:
            w[1 + int(w[1]) + 1] += 1
        w.tofile(f"{prefix}.{c}")
    h5tool("writeraw", tmp_path / name, 16, 1000, 4, 8, 500, prefix)
    return tmp_path / name, x


def check_file(ctx, h5io, h5tool, tmp_path, path, x, crows):
    rows, cols = x.shape
    n = int(h5tool("chunks", path, tmp_path / "stored").stdout)
    stored = [os.path.getsize(f"{tmp_path}/stored.{c}") for c in range(n)]
    xd = torch.from_numpy(x).to(ctx.device)
    for name, sel in row_sets(rows, crows, np.random.default_rng(rows)).items():
        y, st = h5io.read_rows(ctx, str(path), "test", sel)
        assert y.shape == (len(sel), cols)
        assert torch.equal(y, xd[torch.tensor(sel, device=ctx.device)]), name
        touched = sorted({r // crows for r in sel})
        assert len(touched) == {"one": 1, "three": 3, "all": n}[name]
        assert st["n_chunks"] == len(touched), name
        assert st["stored_bytes"] == sum(stored[c] for c in touched), name
        assert st["raw_bytes"] == len(sel) * cols * 2
    # into the caller's tensor; a row past the end
    import deltarice_amd as dr
    out = torch.full((3, cols), 0x5A5A, dtype=torch.int16, device=ctx.device)
    y, _ = h5io.read_rows(ctx, str(path), "test", np.array([rows - 1, 0]), out=out)
    assert y.data_ptr() == out.data_ptr() and torch.equal(out[:2], xd[[rows - 1, 0]]) and bool((out[2] == 0x5A5A).all())
    with pytest.raises(dr.DeltaRiceError) as e:
        h5io.read_rows(ctx, str(path), "test", [0, rows])
    assert e.value.status == 1


@pytest.mark.parametrize("rows", [4000, 3930], ids=["whole-chunks", "padded-last-chunk"])
def test_read_rows_of_a_directly_written_file(env, h5tool, tmp_path, rows):
    ctx, h5io = env
    cols, crows = 7000, 200  # 20 chunks of 200 x 7000
    x = np.random.default_rng(rows).normal(0, 10, (rows, cols)).astype(np.int16)
    f = tmp_path / "direct.h5"
    st = h5io.write(ctx, str(f), "test", torch.from_numpy(x.reshape(-1)).to(ctx.device), rows, cols, crows, 8, cols)
    assert st["n_chunks"] == 20
    check_file(ctx, h5io, h5tool, tmp_path, f, x, crows)


def test_read_rows_of_a_file_the_cpu_oracle_encoded(env, h5tool, tmp_path):
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
    check_file(ctx, h5io, h5tool, tmp_path, f, x, crows)


def test_read_rows_needs_whole_waveforms_per_row(env, h5tool, tmp_path):
    import deltarice_amd as dr
    ctx, h5io = env
    x = np.random.default_rng(4).normal(0, 10, (16, 1000)).astype(np.int16)
    raw = tmp_path / "raw.bin"
    x.tofile(raw)
    for L, name in ((300, "L300.h5"), (4000, "L4000.h5")):  # cols % WaveformLength != 0: waveforms straddle rows
        f = tmp_path / name
        h5tool("write", f, raw, 16, 1000, 4, 8, L)
        with pytest.raises(dr.DeltaRiceError) as e:
            h5io.read_rows(ctx, str(f), "test", [1])
        assert e.value.status == 5
        y = torch.empty(16 * 1000, dtype=torch.int16, device=ctx.device)
        h5io.read(ctx, str(f), "test", y)  # the whole-dataset path reads such a file
        assert np.array_equal(y.cpu().numpy(), x.reshape(-1))


def test_read_and_read_rows_of_a_damaged_chunk(env, h5tool, tmp_path):
    import deltarice_amd as dr
    ctx, h5io = env
    f, x = small_file(h5tool, tmp_path, damaged_chunk=2)  # rows 8 .. 11
    y = torch.empty(x.size, dtype=torch.int16, device=ctx.device)
    for call in (lambda: h5io.read(ctx, str(f), "test", y), lambda: h5io.read_rows(ctx, str(f), "test", [1, 9])):
        with pytest.raises(dr.DeltaRiceError) as e:
            call()
        assert e.value.status == 4
    sel = [15, 0, 7, 12, 0]  # the other chunks are not validated: their rows are delivered
    got, st = h5io.read_rows(ctx, str(f), "test", sel)
    assert np.array_equal(got.cpu().numpy(), x[sel]) and st["n_chunks"] == 3
