"""-m "not gpu": the units and expected answers of tests/test_gpu_cell_recover_at.py (tests/recover_at_cases.py) pinned on the CPU.  The shapes
are what the GPU tests say they are, every expected answer has the length its want list asks for, and the route of
recover_cells_and_kzg_proofs_at holds over Python integers: the coefficients the device's recovery leaves
(recover_spec.recover_coefficients_columns) pushed through the per-pair quotient (cell_proofs_at_spec.quotient_scalars) commit, with the
Lagrange stand-in of tests/test_cell_proofs_at_spec.py, to fk20_spec.quotient_at at the wanted indices -- for a consistent unit, where they
are the blob's own coefficients, and for an inconsistent one, where they are the 4096 the specs' algorithm keeps."""
import pytest

import cell_proofs_at_spec as spec
import cell_spec as cs
import fk20_spec as fk
import recover_at_cases as cases
import recover_spec as rs

R = cs.R
T = pow(5, 7594, R)                                              # a point outside the domain


@pytest.fixture(scope="module")
def lagrange():
    assert pow(T, cs.N_FE, R) != 1
    return spec.lagrange_at(T)


def test_index_sets_are_those_of_the_recovery_tests():
    import test_gpu_cell_recover_sets as sets_tests
    assert cases.index_sets() == sets_tests.index_sets()


@pytest.mark.parametrize("kind", cases.WANT_KINDS)
def test_nine_units(kind):
    units, exp = cases.nine(kind)
    fx = cases.fixture()
    assert len(units) == len(exp) == 9
    for j, ((ix, cells, want), (ec, ep)) in enumerate(zip(units, exp)):
        assert rs.check_indices(ix) == ix and cells == [fx["cells"][j % 3][k] for k in ix]
        assert (ec, ep) == ([fx["cells"][j % 3][k] for k in want], [fx["P"][j % 3][k] for k in want])
        if kind == "missing":
            assert sorted(want + ix) == list(range(128)) and want == sorted(want)
        elif kind == "fixed":
            assert want == [0, 1, 63, 64, 127, 5, 5]
        else:
            assert sorted(want) == list(range(128)) and want != sorted(want)
    if kind == "missing":
        assert [len(u[2]) for u in units] == [64, 64, 64, 64, 64, 63, 28, 1, 0]
    else:
        known, want = set(units[0][0]), units[0][2]
        assert any(k in known for k in want) and any(k not in known for k in want)


def test_refusals_hold_one_per_rule():
    rows = cases.refusals()
    assert [r[0] for r in rows] == ["63 known cells", "129 known cells", "known index 128", "known indices not ascending", "cell element >= r",
                                    "wanted index 128", "129 wanted", "nothing wanted", "nothing wanted, spoiled"]
    for name, units, statuses, (e_left, e_right) in rows:
        assert len(units) == 3 and statuses == ([0, 0, 0] if name == "nothing wanted" else [0, 1, 0]), name
        for u, e in ((units[0], e_left), (units[2], e_right)):
            assert rs.check_indices(u[0]) == u[0] and len(e[0]) == len(e[1]) == len(u[2]), name
        ix, cells, want = units[1]
        assert len(ix) == len(cells), name
        lists_ok = True
        try:
            rs.check_indices(ix)
        except cs.BadArgs:
            lists_ok = False
        canonical = all(int.from_bytes(c[32 * i:32 * i + 32], "big") < R for c in cells for i in range(64))
        want_ok = len(want) <= 128 and all(k < 128 for k in want)
        assert [lists_ok, canonical, want_ok].count(False) == (0 if name == "nothing wanted" else 1), name      # one rule at a time


def check_route(f, want, lagrange):
    for k in sorted(set(want)):
        s = spec.quotient_scalars(f, k)
        assert sum(a * b for a, b in zip(s, lagrange)) % R == fk.quotient_at(f, k, T), k


def test_route_on_a_consistent_unit(lagrange):
    units, _ = cases.nine("fixed")
    ix, cells, want = units[5]                                     # random65, fixture blob 2
    f, high = rs.recover_coefficients_columns(ix, cells)
    assert not high and f == cs.blob_coefficients(cases.fixture()["blobs"][2])
    check_route(f, want, lagrange)


def test_route_on_the_inconsistent_unit(lagrange):
    units, f_spec, exp_cells, exp_good = cases.inconsistent()
    ix, cells, want = units[0]
    assert len(ix) == 65 and len(exp_cells) == len(want) == len(cases.INCONSISTENT_WANT)
    f, high = rs.recover_coefficients_columns(ix, cells)
    assert high and f == f_spec and f != cs.blob_coefficients(cases.fixture()["blobs"][2])
    assert exp_cells == [rs.cells_from_coefficients_columns(f)[k] for k in want]
    # the changed cell comes back as the kept coefficients have it, not as it was handed in
    assert 30 in want and exp_cells[want.index(30)] != cells[0]
    check_route(f, want, lagrange)
    gix, gcells, gwant = units[1]
    assert sorted(gix + gwant) == list(range(128)) and len(exp_good[0]) == len(exp_good[1]) == 64
