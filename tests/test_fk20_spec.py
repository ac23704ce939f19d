"""CPU (-m "not gpu"): the FK20 restatement tests/fk20_spec.py.  The device's index route over Fr (circulant layout, transform orders, the
dropped half, the bit reversal) gives every cell quotient at a random point, for random and special blobs; the coset route gives cell_spec's
cells; and the H formula through the oracle reproduces the 128 proofs of fixture blob 0 in tests/golden/cells.json."""
import json
import os
import random

import pytest

import cell_spec as cs
import fk20_spec as fk
from synth import random_blob

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R


def blob_of_values(vals):
    return b"".join((v % R).to_bytes(32, "big") for v in vals)


def blob_of_coefficients(f):
    """the blob (bit-reversed evaluations) of the polynomial with coefficients f"""
    w4096 = fk.W4096
    out = []
    for i in range(cs.N_FE):
        x = pow(w4096, cs.rev(i, 12), R)
        acc = 0
        for c in reversed(f):
            acc = (acc * x + c) % R
        out.append(acc)
    return blob_of_values(out)


def special_coefficients():
    c = 0x1234567
    yield "zero", [0] * cs.N_FE
    yield "x64_plus_c", [c] + [0] * 63 + [1] + [0] * (cs.N_FE - 65)
    yield "x4095", [0] * (cs.N_FE - 1) + [1]
    yield "x_64_plus_t", [0] * 77 + [1] + [0] * (cs.N_FE - 78)


@pytest.fixture(scope="module")
def route_setup():
    rng = random.Random(2024)
    t = rng.randrange(1, R)
    return t, fk.setup_columns(lambda j: pow(t, j, R))


def check_route(f, t, X):
    pi, h = fk.route_proofs(f, X)
    assert h[:63] == fk.h_field(f, t)
    assert h[63] == 0
    for k in range(cs.CELLS_PER_EXT_BLOB):
        assert pi[k] == fk.quotient_at(f, k, t), k


def test_route_over_fr_random_blobs(route_setup):
    t, X = route_setup
    for seed in (0, 7):
        check_route(cs.blob_coefficients(random_blob(seed)), t, X)


def test_route_over_fr_random_coefficients(route_setup):
    t, X = route_setup
    rng = random.Random(5)
    check_route([rng.randrange(R) for _ in range(cs.N_FE)], t, X)


@pytest.mark.parametrize("name,f", list(special_coefficients()))
def test_route_over_fr_special(route_setup, name, f):
    t, X = route_setup
    check_route(f, t, X)


def test_special_blobs_round_trip_to_their_coefficients():
    for name, f in special_coefficients():
        if name in ("zero", "x64_plus_c"):
            assert cs.blob_coefficients(blob_of_coefficients(f)) == f, name


def test_coset_route_gives_the_cells():
    for seed in (3,):
        blob = random_blob(seed)
        f, hi = fk.route_cells(blob)
        assert f == cs.blob_coefficients(blob)
        assert hi == cs.compute_cells(blob)[64:]


def test_h_points_reproduce_the_fixture_proofs(oracle):
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    blob = random_blob(d["blob_seeds"][0])
    H = fk.h_points(oracle, blob, cs.load_monomial())
    assert len(H) == 63
    assert [p.hex() for p in fk.proofs_from_h(oracle, H)] == d["proofs"][0]
