"""-m "not gpu": the identity behind the commitment output of the FK20 chain, over Fr with fk20_spec's stand-in
T(j) = t^j of [tau^j]_1.  The chain keeps conv[62 - e] (e < 63) of conv = dit(Z, w128^-1) as H_e; one slot further

    conv[63] = sum_r sum_d c_r[d] x_r[63 - d] = sum_r sum_u f_(64u+r) T(64u + r) = p(t),

the stand-in of the blob's commitment: the indices 63 - d stay in 0..63 and c_r is zero above d = 63, so nothing wraps around.  It is the one
slot that reads x_r[63] = T(4032 + r), which no proof depends on.  Reading it changes nothing the proofs are made of."""
import random

import pytest

from oracle.pyref import R

import fk20_spec as fk

T_POINT = 0x1d0c0ffee5eed % R


def _T(j):
    return pow(T_POINT, j, R)


@pytest.fixture(scope="module")
def X():
    return fk.setup_columns(_T)


def conv_of(f, X):
    C = fk.field_columns(f)
    Z = [sum(C[r][i] * X[r][i] for r in range(fk.CELL_FE)) % R for i in range(fk.FFT)]
    return fk.dit(Z, pow(fk.W128, -1, R))


def p_at_t(f):
    acc = 0
    for c in reversed(f):
        acc = (acc * T_POINT + c) % R
    return acc


def monomial(d):
    f = [0] * fk.N_FE
    f[d] = 1
    return f


def _cases():
    rng = random.Random(0x7594)
    high = [0] * fk.N_FE
    for m in range(fk.N_FE - fk.CELL_FE, fk.N_FE):
        high[m] = rng.randrange(R)
    return [("random", [rng.randrange(R) for _ in range(fk.N_FE)]), ("zero", [0] * fk.N_FE), ("degrees >= 4032", high)] + \
           [(f"X^{d}", monomial(d)) for d in (0, 63, 64, 4032, 4095)]


CASES = _cases()


@pytest.mark.parametrize("name,f", CASES, ids=[n for n, _ in CASES])
def test_slot_63_of_the_convolution_is_the_polynomial_at_t(X, name, f):
    conv = conv_of(f, X)
    assert conv[fk.CELL_FE - 1] == p_at_t(f)
    if name.startswith("X^"):
        assert conv[fk.CELL_FE - 1] == _T(int(name[2:]))
    # and the slots next to it are what route_proofs keeps: reading slot 63 changes none of them
    proofs, h = fk.route_proofs(f, X)
    assert h == [conv[fk.CELL_FE - 2 - e] for e in range(fk.CELL_FE - 1)] + [0]
    assert h[:fk.CELL_FE - 1] == fk.h_field(f, T_POINT)


def test_slot_63_is_the_only_reader_of_the_top_setup_points(X):
    """With T zeroed at 4032..4095 (x_r[63] = 0), every proof of a random polynomial is unchanged and conv[63] loses exactly those terms."""
    rng = random.Random(63)
    f = [rng.randrange(R) for _ in range(fk.N_FE)]
    top = fk.N_FE - fk.CELL_FE
    X0 = fk.setup_columns(lambda j: 0 if j >= top else _T(j))
    assert fk.route_proofs(f, X0) == fk.route_proofs(f, X)
    assert conv_of(f, X0)[fk.CELL_FE - 1] == p_at_t(f[:top])
    assert conv_of(f, X)[fk.CELL_FE - 1] == p_at_t(f)
