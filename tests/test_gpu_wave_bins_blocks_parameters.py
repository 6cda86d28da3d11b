"""GPU: the block form of drx_wave_bins ("bins_impl" = 1) at every RiceParameter, on every (lanes per block, stream words per
lane) class and on data that the parameter does not suit: the cells of tests/block_cells.py (tests/test_block_cells_model.py
proves on the CPU which class each one runs and which of them need the second parse).

The streams are the oracle's, the expected rows numpy's over the oracle's input (tests/wave_bins_reference.py); every comparison
is exact, by the walk and by the side-band, and every call asserts its path and its form.  The block form leaves the waveforms it
flags to the lane kernel behind it: on the matched cells with k >= 1 the list must be empty -- the blocks did the work, and the
fallback did not hide them (drx_decode_windows is held to the same on the same cells: the flags are phase 1's, which the forms
share); on the other cells the count goes into the failure message."""
import numpy as np
import pytest

import block_cells as bc
from deltarice_amd import _lib as D
from test_gpu_select import Stream
from test_gpu_wave_bins_blocks import ALL, BLOCKS, check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    import deltarice_amd as dr
    c = dr.Context(0)
    yield c
    c.set_option("bins_impl", 0)
    c.set_option("debug_flags", 0)
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("cell", bc.CELLS, ids=lambda c: c.id)
def test_wave_bins(ctx, O, cell):
    x = cell.x()
    st = Stream(ctx, O, x, cell.Ns, cell.Ls, cell.m)
    W = st.plan.total_waves
    blocks_alone = cell.kind == "matched" and cell.k >= 1
    listed = (lambda k: k == 0) if blocks_alone else None
    try:
        start = torch.from_numpy(np.random.default_rng(cell.k + cell.L).integers(-300, cell.L + 301, W)).to(ctx.device)
        for bin in (17, 250, cell.L):
            for origin in (None, start):
                check(ctx, st, x, bin, None, origin, 0, BLOCKS, what=cell.id, listed=listed)
        # every waveform listed: the same rows, written by the lane kernel behind the blocks over what the blocks merged
        check(ctx, st, x, 250, None, start, 0, BLOCKS | ALL, what=cell.id, flags=D.DBG_BINS_ALL_FALLBACK, listed=lambda k: k == W)
    finally:
        st.plan.close()
