"""-m "not gpu": the route of compute_kzg_proofs_at restated in Python integers (tests/point_proofs_at_spec.py) against the definition it
implements.  The blocked scan (segments of 8, doubling rounds, second pass) equals plain synthetic division; and the forward transform of the
quotient, in blob order, equals the evaluation-form quotient that oracle/pyref.py's compute_kzg_proof_impl commits to (kzg.rs:461-528), on
both of its branches: z outside the domain, and z = w_m, where the reference takes its own formula for position m."""
import random

import pytest

import cell_spec as cs
import point_proofs_at_spec as spec
from oracle import pyref
from synth import random_blob

R = cs.R
ROOTS = pyref.compute_roots_of_unity(4096)                           # blob order: ROOTS[i] = w4096^rev12(i)
POINTS = {"outside": pow(5, 4844, R), "zero": 0, "r_minus_1": R - 1, "w_0": ROOTS[0], "w_1": ROOTS[1], "w_2048": ROOTS[2048], "w_4095": ROOTS[4095]}


class EvaluationForm:
    """what compute_kzg_proof_impl reads of a settings object; with pyref's lincomb and compression stood in for, it hands back q itself"""
    roots = ROOTS
    g1 = None


@pytest.fixture(scope="module")
def blob():
    return random_blob(4844)


@pytest.fixture(scope="module")
def coefficients(blob):
    return cs.blob_coefficients(blob)


def test_the_points_are_what_their_names_say():
    assert pow(POINTS["outside"], 4096, R) != 1 and ROOTS[0] == 1 and ROOTS[1] == R - 1
    assert all(pow(POINTS[k], 4096, R) == 1 for k in ("w_0", "w_1", "w_2048", "w_4095", "r_minus_1"))


@pytest.mark.parametrize("n", [4096, 64], ids=["4096", "64"])
def test_blocked_scan_is_synthetic_division(n):
    rng = random.Random(19 * n)
    for z in [rng.randrange(R), 0, 1, R - 1, rng.randrange(R)]:
        f = [rng.randrange(R) for _ in range(n)]
        q, y = spec.blocked_division(f, z)
        assert (q, y) == spec.synthetic_division(f, z)
        assert q[n - 1] == 0
        horner = 0
        for c in reversed(f):
            horner = (horner * z + c) % R
        assert y == horner


def test_monomials_divide_to_powers_of_z():
    z = POINTS["outside"]
    for k in (1, 7, 8, 9, 511, 512, 4088, 4095):
        f = [0] * 4096
        f[k] = 1
        q, y = spec.blocked_division(f, z)
        assert y == pow(z, k, R) and q == [pow(z, k - 1 - j, R) for j in range(k)] + [0] * (4096 - k)


@pytest.mark.parametrize("name", list(POINTS))
def test_scalars_are_the_references_evaluation_form_quotient(monkeypatch, blob, coefficients, name):
    z = POINTS[name]
    monkeypatch.setattr(pyref, "g1_lincomb", lambda points, scalars: [s % R for s in scalars])
    monkeypatch.setattr(pyref, "g1_compress", lambda q: q)
    want_q, want_y = pyref.compute_kzg_proof_impl(pyref.blob_to_polynomial(blob), z, EvaluationForm)
    assert spec.quotient_scalars(coefficients, z) == want_q
    assert spec.blocked_division(coefficients, z)[1] == want_y
