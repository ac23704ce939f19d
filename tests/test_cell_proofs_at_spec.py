"""-m "not gpu": the route of compute_cell_kzg_proofs_at restated in Python integers (tests/cell_proofs_at_spec.py) against the definition it
implements.  Over Fr, with [tau^j]_1 replaced by t^j and the Lagrange setup points by L_i(t), the linear combination of the route's scalars
must be q_k(t) as fk20_spec.quotient_at divides it out; in the group, the scalars' lincomb over the Lagrange setup must be the oracle-derived
proof of tests/golden/cells.json."""
import json
import os
import random

import pytest

import cell_proofs_at_spec as spec
import cell_spec as cs
import fk20_spec as fk
from synth import random_blob

R = cs.R
HERE = os.path.dirname(os.path.abspath(__file__))
T = pow(5, 7594, R)                                              # a point outside the domain
KS = [0, 1, 63, 64, 127] + random.Random(15).sample(range(128), 2)


@pytest.fixture(scope="module")
def lagrange():
    assert pow(T, cs.N_FE, R) != 1
    return spec.lagrange_at(T)


@pytest.fixture(scope="module", params=["random", "x4095"])
def coefficients(request):
    if request.param == "x4095":
        return [0] * 4095 + [1]
    return cs.blob_coefficients(random_blob(7594))


def test_lagrange_stand_in(lagrange):
    """sum_i p(x_i) L_i(t) = p(t) for the blob order of the domain: what makes L_i(t) the stand-in of the setup points"""
    blob = random_blob(15)
    f = cs.blob_coefficients(blob)
    vals = [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(cs.N_FE)]
    horner = 0
    for c in reversed(f):
        horner = (horner * T + c) % R
    assert sum(v * l for v, l in zip(vals, lagrange)) % R == horner


@pytest.mark.parametrize("k", KS)
def test_scalars_commit_to_the_quotient(coefficients, lagrange, k):
    q = spec.quotient_coefficients(coefficients, k)
    assert q[cs.N_FE - cs.CELL_FE:] == [0] * cs.CELL_FE
    s = spec.quotient_scalars(coefficients, k)
    assert sum(a * b for a, b in zip(s, lagrange)) % R == fk.quotient_at(coefficients, k, T)


def test_x4095_quotient_is_the_closed_form():
    """q[64u + 63] = a_k^(62-u) and nothing else: what tests/test_gpu_cell_proofs_at.py sums over the monomial points"""
    for k in (0, 1, 127):
        a = fk.a_k(k)
        want = [0] * cs.N_FE
        for u in range(63):
            want[64 * u + 63] = pow(a, 62 - u, R)
        assert spec.quotient_coefficients([0] * 4095 + [1], k) == want


@pytest.mark.parametrize("k", [0, 127])
def test_group_form_is_the_fixture_proof(oracle, setup_bytes, k):
    fx = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    g1 = setup_bytes[0]
    # the setup file holds [L_j(tau)]_1 for the domain point w4096^j; blob order puts w4096^rev12(i) at position i (the handle permutes them at load)
    lagrange_setup = [g1[48 * cs.rev(i, 12):48 * cs.rev(i, 12) + 48] for i in range(cs.N_FE)]
    f = cs.blob_coefficients(random_blob(fx["blob_seeds"][0]))
    assert cs.lincomb(oracle, lagrange_setup, spec.quotient_scalars(f, k)) == bytes.fromhex(fx["proofs"][0][k])
