"""-m "not gpu": the identity behind verify_blob_cell_proofs_batch's interpolation (tests/blob_cell_cases.py), in Python
integers against tests/cell_spec.py: the batch interpolant of all 128 cells of every blob, from the blobs' coefficients and 64 weights, equals the
sum over the cells of r^k times cell_spec.cell_interpolant, and its commitment is the [I(tau)]_1 of cell_spec.verify_cell_kzg_proof_batch."""
import random

import pytest

import blob_cell_cases as bcc
import cell_device_cases as dcases
import cell_spec as cs

R = cs.R


@pytest.fixture(scope="module")
def fx():
    fx = dcases.fixture()
    fx["coef"] = [cs.blob_coefficients(b) for b in fx["blobs"]]
    fx["mono"] = cs.load_monomial(cs.CELL_FE)
    fx["g2"] = cs.g2_points()
    return fx


def check_group(oracle, fx, blobs, r_free):
    """the identity at a free r, and -- at the group's own challenge -- against what the spec's check computes"""
    cells = [fx["cells"][b] for b in blobs]
    coef = [fx["coef"][b] for b in blobs]
    assert bcc.interpolant_from_coefficients(r_free, coef) == bcc.interpolant_by_cells(r_free, cells)
    commitments, proofs = [fx["C"][b] for b in blobs], [p for b in blobs for p in fx["P"][b]]
    args = bcc.group_args(cells, commitments, proofs)
    r, uniq, pos = cs.challenge(*args)
    out, ok = bcc.expected(oracle, cells, commitments, proofs, fx["mono"], fx["g2"])
    assert ok is True and out[:32] == r.to_bytes(32, "big")
    assert out[32:80] == cs.lincomb(oracle, fx["mono"], bcc.interpolant_from_coefficients(r, coef))
    return r, uniq, pos, out


def test_two_random_blobs(oracle, fx):
    r, uniq, pos, _ = check_group(oracle, fx, [0, 1], random.Random(0x7594).randrange(R))
    assert uniq == [fx["C"][0], fx["C"][1]] and pos == [0] * 128 + [1] * 128


def test_the_same_blob_twice(oracle, fx):
    r, uniq, pos, out = check_group(oracle, fx, [2, 2], random.Random(0x7595).randrange(R))
    assert uniq == [fx["C"][2]] and pos == [0] * 256, "one unique commitment"
    # its weight is r^0 + .. + r^255: RL = w C - [I(tau)]_1 + sum_k r^k a_k pi_k with that w
    w = sum(pow(r, k, R) for k in range(256)) % R
    a = [pow(cs.coset_shift(k), cs.CELL_FE, R) for k in range(128)]
    proofs = fx["P"][2] * 2
    rl = cs.lincomb(oracle, [fx["C"][2], out[32:80]] + proofs, [w, R - 1] + [pow(r, k, R) * a[k % 128] % R for k in range(256)])
    assert rl == out[128:176]
    # and the interpolant is that of the blob itself times (1 + r^128)
    one = bcc.interpolant_from_coefficients(r, [fx["coef"][2]])
    assert bcc.interpolant_from_coefficients(r, [fx["coef"][2]] * 2) == [(1 + pow(r, 128, R)) * v % R for v in one]


def test_the_zero_blob(oracle, fx):
    zero = bytes(32 * cs.N_FE)
    cells = cs.compute_cells(zero)
    assert cells == [bytes(cs.BYTES_PER_CELL)] * 128 and cs.blob_coefficients(zero) == [0] * cs.N_FE
    r = random.Random(0x7596).randrange(R)
    assert bcc.interpolant_from_coefficients(r, [[0] * cs.N_FE]) == bcc.interpolant_by_cells(r, [cells]) == [0] * cs.CELL_FE
    out, ok = bcc.expected(oracle, [cells], [bcc.INF], [bcc.INF] * 128, fx["mono"], fx["g2"])
    assert ok is True and out[32:] == bcc.INF * 3


def test_the_weights_are_a_table_lookup():
    """a_k^u = w128^(rev7(k) u mod 128): what the weights kernel reads instead of powering"""
    w128 = pow(cs.W, 64, R)
    for k in (0, 1, 5, 77, 127):
        a = pow(cs.coset_shift(k), cs.CELL_FE, R)
        for u in (0, 1, 2, 31, 63):
            assert pow(a, u, R) == pow(w128, cs.rev(k, 7) * u % 128, R)
