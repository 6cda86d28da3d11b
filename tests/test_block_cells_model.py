"""CPU: the table of tests/block_cells.py proves what it claims.  Every cell's stream is the oracle's; its class -- lanes per
block and stream words per lane, hence the template instantiation that each block form runs on it -- comes from the mirrored
geometry rules (tests/test_blk_rule_host.py pins them to the C++).  The table must hold every k from 0 to 15, all 12 classes,
a cell at each lanes-per-block value on which some lane provably holds more codes than its share of the staging buffer (several
staging passes), and matched cells whose codes have at least three different lengths (a parse falls into step on them, which is
why the GPU tests may assert that the blocks left no waveform to the lane kernel there).  The residue streams place the end of
a payload on and around a block's border."""
import pytest

import block_cells as bc


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def measured(O):
    rows = [bc.measure(O, c) for c in bc.CELLS]
    print("\ncell                       k  lanes  words/lane  cap  bits/sample  codes on some lane >=  several passes  code lengths")
    for c, r in zip(bc.CELLS, rows):
        print(f"{c.id:24s} {r['k']:3d} {r['lanes']:6d} {r['sw']:11d} {r['cap']:4d} {r['bits']:12.3f} {r['most']:22.1f}  "
              f"{'yes' if r['passes'] else 'no':>14s} {r['lengths']:13d}")
    return rows


def test_every_rice_parameter_occurs(measured):
    ks = sorted({r["k"] for r in measured})
    print("k:", ks)
    assert ks == list(range(16))


def test_every_class_occurs(measured):
    pairs = sorted({(r["lanes"], r["sw"]) for r in measured})
    print("classes:", pairs)
    assert pairs == [(nt, sw) for nt in (64, 128, 256) for sw in (9, 11, 15, 19)]


def test_several_staging_passes_at_every_lanes_per_block(measured):
    for nt in (64, 128, 256):
        cells = [c.id for c, r in zip(bc.CELLS, measured) if r["lanes"] == nt and r["passes"]]
        print(nt, "lanes, several passes:", cells)
        assert cells, nt
    # ... and inside a waveform of noise: the zero stretch of every stretch cell with k <= 2
    assert all(r["passes"] for c, r in zip(bc.CELLS, measured) if c.kind == "stretch" and c.k <= 2)
    assert {r["lanes"] for c, r in zip(bc.CELLS, measured) if c.kind == "stretch" and c.k <= 2} == {64, 128, 256}


def test_matched_cells_hold_codes_of_three_lengths(measured):
    """At least three lengths in every matched cell with k >= 1 -- where the format has three: a zig-zag value is below 2^16,
    so at k = 15 its quotient is 0 or 1 and no stream of any data holds more than the two lengths 16 and 17; there both occur."""
    for c, r in zip(bc.CELLS, measured):
        if c.kind == "matched" and c.k >= 1:
            assert r["lengths"] >= (3 if c.k < 15 else 2), (c, r["lengths"])


def test_lengths_take_the_lanes_the_table_says():
    for c in bc.CELLS:
        want = {3000: 64 if c.k <= 6 or c.k in (8, 9) else 128, 6000: 64 if c.k == 0 else 128 if c.k <= 6 or c.k in (8, 9) else 256, 20000: 256}[c.L]
        assert bc.nt_for_len(c.L, c.k) == want, c


@pytest.mark.parametrize("k,L,kind", bc.RESIDUE_CELLS)
def test_payload_ends_around_a_block_border(O, k, L, kind):
    base = bc.measure(O, bc.Cell(k, L, kind))
    found = bc.residue_cells(O, k, L, kind)
    assert list(found) == [0, 1, 3, 4, 5, 8, 9, "B-1"]
    top = int(bc.measure(O, bc.Cell(k, L, kind, last=L))["n_i"][2])
    for name, cell in found.items():
        r = base["B"] - 1 if name == "B-1" else name
        if cell is None:
            # no length from 1 to L gives the residue: a waveform of L samples has fewer payload words than that
            assert top < (r if r >= 1 else base["B"]), (k, L, kind, name, top)
            print(f"k{k}-L{L}-{kind}: residue {name} NOT REACHABLE: B = {base['B']} words, a waveform of {L} samples has {top}")
            continue
        got, B, cls = bc.residue_of(O, cell)
        print(f"k{k}-L{L}-{kind}: residue {name}: last waveform of {cell.last} samples, n mod {B} = {got}, class {cls}")
        assert cls == (base["lanes"], base["sw"]), (k, L, kind, name, "the class moved", cls)  # the class did not move
        assert got == (B - 1 if name == "B-1" else name), (k, L, kind, name, got)
    assert any(c is not None for c in found.values())
