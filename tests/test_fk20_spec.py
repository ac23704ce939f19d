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


# ---- the edge-case constructions used by tests/test_gpu_cell_compute_edges.py
def test_blob_from_coefficients_inverts_blob_coefficients():
    rng = random.Random(11)
    for f in ([rng.randrange(R) for _ in range(cs.N_FE)], [rng.randrange(R) for _ in range(100)] + [0] * (cs.N_FE - 100), [R - 1] + [0] * (cs.N_FE - 1)):
        assert cs.blob_coefficients(fk.blob_from_coefficients(f)) == f
    short = [rng.randrange(R) for _ in range(70)]                # Horner at every domain point agrees
    assert fk.blob_from_coefficients(short) == blob_of_coefficients(short)


def test_comb_digits_restate_the_recoding():
    rng = random.Random(12)
    corpus = fk.comb_corpus()
    assert len({k for _, k in corpus}) == len(corpus) >= 64
    for name, k in corpus + [("random", rng.randrange(R)) for _ in range(2000)]:
        assert 0 <= k < R, name
        ds = fk.comb_digits(k)
        assert len(ds) == 64 and all(-8 <= d <= 7 for d in ds) and ds[63] >= 0, name
        assert fk.from_digits(ds) == k, name
    named = dict(corpus)
    assert fk.comb_digits(named["-8s under 7"]) == [-8] * 63 + [7]
    assert fk.comb_digits(named["7s, 3 at 62, under 7"]) == [7] * 62 + [3, 7]
    assert fk.comb_digits(named["-8/7 under 3"]) == [-8 if w % 2 == 0 else 7 for w in range(63)] + [3]
    assert fk.comb_digits(named["-8 at 31 under 1"]) == [-8 if w == 31 else 0 for w in range(63)] + [1]
    assert fk.comb_digits(2 ** 252 - 1) == [-1] + [0] * 62 + [1]
    assert fk.comb_digits(0) == [0] * 64
    assert fk.comb_digits(R - 1)[63] == 7


def test_k_star_is_the_one_doubling_scalar():
    assert fk.K_STAR == 0x6c1258acd66282b7ccc627f7f65e27faac425bfd0001a40100000000ffffffff
    assert fk.comb_digits(fk.K_STAR)[63] == 7
    assert fk.comb_doubling_windows(fk.K_STAR) == [("dbl", 63)]
    for k in (fk.K_STAR - 1, fk.K_STAR + 1, fk.K_STAR - 16 ** 62, fk.K_STAR + 16 ** 62, fk.K_STAR - 16 ** 63, R - 1, 0, 1):
        assert fk.comb_doubling_windows(k) == [], hex(k)
    hits = [n for n, k in fk.comb_corpus() if fk.comb_doubling_windows(k)]
    assert hits == ["k*"]
    rng = random.Random(13)
    assert not any(fk.comb_doubling_windows(rng.randrange(R)) for _ in range(3000))
    # Why k* is the only one.  Before window w the accumulator is S X, S = sum_(v<w) d_v 16^v, |S| <= B_w = 8 (16^w - 1) / 15 < 16^w, and
    # S != 0 once a digit was added.  A hit needs S = +-d_w 16^w (mod r) with d_w != 0.
    #   w < 63: 0 < |S -+ d_w 16^w| <= B_62 + 8 16^62 < r, so there is none.
    #   w = 63, d = d_63 in 1..7: S = -d 16^63 (mod r) means k = S + d 16^63 = 0 (mod r), but 0 <= k < r and k = 0 has d_63 = 0.  S = d 16^63
    #   (mod r): S - d 16^63 lies in [-B_63 - 7 16^63, B_63 - 16^63] = [-7.54 16^63, -0.46 16^63] and r = 7.24 16^63, so it is -r:
    #   S = d 16^63 - r, and |S| <= B_63 leaves d = 7 alone: k = S + 7 16^63 = 14 16^63 - r.
    def B(w):
        return 8 * (16 ** w - 1) // 15

    assert B(62) + 8 * 16 ** 62 < R
    assert -B(63) - 7 * 16 ** 63 > -2 * R and B(63) - 16 ** 63 < 0
    assert [d for d in range(1, 8) if abs(d * 16 ** 63 - R) <= B(63)] == [7]


def test_no_scalar_below_r_meets_an_inverse():
    # the inverse case at window 63 would need k = 0 (mod r) with d_63 > 0 (above); below 63 no hit of either sign exists
    assert fk.comb_doubling_windows(R) == [("inv", 63)]           # k = r itself: the partial sum is -7 16^63 before a digit 7
    rng = random.Random(14)
    for name, k in fk.comb_corpus() + [("random", rng.randrange(R)) for _ in range(1000)]:
        assert all(kind == "dbl" for kind, _ in fk.comb_doubling_windows(k)), name


def test_column_blob_puts_one_scalar_in_every_bin():
    s = [k for _, k in fk.comb_corpus()[:64]]
    blob = fk.column_blob(s)
    f = cs.blob_coefficients(blob)
    assert [m for m in range(cs.N_FE) if f[m]] == [4032 + r for r in range(64) if s[r]]
    assert fk.field_columns(f) == [[s[r]] * 128 for r in range(64)]


def test_column_pair_and_vanishing_columns():
    rng = random.Random(15)
    for i0 in (0, 1, 64, 127):
        c = fk.column_pair(fk.K_STAR, i0, rng.randrange(R))
        C = fk.field_columns(cs.blob_coefficients(fk.columns_blob([[0]] * 9 + [c])))
        assert C[9][i0] == fk.K_STAR and sum(v == fk.K_STAR for v in C[9]) == 1
        assert all(v == 0 for r in range(9) for v in C[r])
    bins = (0, 5, 64, 127)
    cols = [fk.column_vanishing(bins, [rng.randrange(1, R) for _ in range(3)]) for _ in range(64)]
    C = fk.field_columns(cs.blob_coefficients(fk.columns_blob(cols)))
    for r in range(64):
        assert [i for i in range(128) if C[r][i] == 0] == list(bins)


def test_route_over_fr_column_blobs(route_setup):
    t, X = route_setup
    rng = random.Random(16)
    check_route(cs.blob_coefficients(fk.column_blob([fk.K_STAR] * 64)), t, X)
    cols = [fk.column_vanishing((0, 127), [rng.randrange(R)]) for _ in range(64)]
    check_route(cs.blob_coefficients(fk.columns_blob(cols)), t, X)


def test_sparse_h_points_match_the_full_lincombs(oracle):
    mono = cs.load_monomial()
    rng = random.Random(17)
    f = [0] * cs.N_FE
    for m in rng.sample(range(64, cs.N_FE), 40):
        f[m] = rng.randrange(R)
    blob = fk.blob_from_coefficients(f)
    H = fk.h_points(oracle, blob, mono)
    for e in (0, 30, 62):
        assert H[e] == cs.lincomb(oracle, mono[:cs.N_FE - 64 * (e + 1)], f[64 * (e + 1):]), e
    for k in (0, 77):
        assert fk.proofs_from_h(oracle, H, cells=[k]) == [cs.lincomb(oracle, H, [pow(fk.a_k(k), e, R) for e in range(63)])]
    assert fk.h_points(oracle, bytes(cs.N_FE * 32), mono) == [fk.G1_INF] * 63
    assert fk.proofs_from_h(oracle, [fk.G1_INF] * 63, cells=[3]) == [fk.G1_INF]
