"""-m "not gpu": tests/recover_spec.py against itself and cell_spec.py.  The consensus-spec route (8192-point transforms) and the device's
column route (transforms of 64 and 128 points) both return cell_spec.blob_coefficients of the blob for every shape of index set; they agree
on an inconsistent input, where -- and only where -- the column route sees nonzero upper halves; the refusals raise; the cells of a
coefficient vector are the same by both constructions."""
import random

import pytest

import cell_spec as cs
import recover_spec as rs
from synth import random_blob

R = cs.R


def index_sets():
    sets = [("first64", list(range(64))), ("last64", list(range(64, 128))), ("odd", list(range(1, 128, 2))), ("even", list(range(0, 128, 2)))]
    for n in (64, 65, 100, 128):
        sets.append((f"random{n}", sorted(random.Random(1000 + n).sample(range(128), n))))
    return sets


@pytest.fixture(scope="module")
def blob_and_cells():
    blob = random_blob(7700)
    return blob, cs.compute_cells(blob)


@pytest.mark.parametrize("name,ix", index_sets(), ids=[n for n, _ in index_sets()])
def test_both_routes_return_the_blob_coefficients(blob_and_cells, name, ix):
    blob, cells = blob_and_cells
    want = cs.blob_coefficients(blob)
    known = [cells[k] for k in ix]
    low, high = rs.recover_coefficients_spec(ix, known, with_high=True)
    assert low == want and not any(high)
    f, hi = rs.recover_coefficients_columns(ix, known)
    assert f == want and hi is False


def test_second_blob_and_cells_of_the_coefficients():
    blob = random_blob(7701)
    cells = cs.compute_cells(blob)
    ix = sorted(random.Random(5).sample(range(128), 77))
    f, hi = rs.recover_coefficients_columns(ix, [cells[k] for k in ix])
    assert f == cs.blob_coefficients(blob) and hi is False
    assert rs.cells_from_coefficients(f) == cells
    assert rs.cells_from_coefficients_columns(f) == cells


def test_cell_coefficients_are_the_interpolant(blob_and_cells):
    _, cells = blob_and_cells
    for k in (0, 1, 77, 127):
        vals = cs.cell_values(cells[k])
        assert rs.cell_coefficients(vals, k) == cs.cell_interpolant(vals, k)


def test_inconsistent_input_both_routes_agree_and_only_then_the_high_halves_show():
    blob = random_blob(7702)
    cells = cs.compute_cells(blob)
    ix = list(range(20, 100))
    bad = [cells[k] for k in ix]
    t = bytearray(bad[3])
    t[31] ^= 1
    bad[3] = bytes(t)
    low, high = rs.recover_coefficients_spec(ix, bad, with_high=True)
    f, hi = rs.recover_coefficients_columns(ix, bad)
    assert f == low and low != cs.blob_coefficients(blob)
    assert hi is True and any(high)
    # the cells of what was recovered are NOT the input at the changed cell's neighbours in general, but both constructions agree on them
    assert rs.cells_from_coefficients(f) == rs.cells_from_coefficients_columns(f)
    # with exactly 64 cells every input is consistent: a changed element gives another polynomial, not an error and no high half
    ix64 = list(range(0, 128, 2))
    known = [cells[k] for k in ix64]
    t = bytearray(known[9])
    t[63] ^= 4
    known[9] = bytes(t)
    f64, hi64 = rs.recover_coefficients_columns(ix64, known)
    assert hi64 is False and f64 != cs.blob_coefficients(blob)
    got = rs.cells_from_coefficients(f64)
    assert [got[k] for k in ix64] == known


def test_refusals(blob_and_cells):
    _, cells = blob_and_cells
    bad_sets = [list(range(63)), list(range(128)) + [128], list(range(63)) + [128], list(range(63)) + [62], list(range(62)) + [70, 69],
                [5] * 64, list(range(64))[::-1], []]
    for ix in bad_sets:
        with pytest.raises(cs.BadArgs):
            rs.check_indices(ix)
    assert rs.check_indices(range(64)) == list(range(64))
    assert rs.check_indices(range(128)) == list(range(128))
    ix = list(range(64))
    for fn in (rs.recover_coefficients_spec, rs.recover_coefficients_columns):
        with pytest.raises(cs.BadArgs):
            fn(ix, [cells[k] for k in ix][:-1])                   # length mismatch
        with pytest.raises(cs.BadArgs):
            fn(ix, [R.to_bytes(32, "big") + cells[0][32:]] + [cells[k] for k in ix[1:]])   # element = r
        with pytest.raises(cs.BadArgs):
            fn(list(range(63)), [cells[k] for k in range(63)])
