"""CPU restatement of recover_cells_and_kzg_proofs (consensus specs fulu/polynomial-commitments-sampling.md), the yardstick of
kzg355_recover_cells_and_kzg_proofs (k_cell_recover.hip).  Python integers over Fr; cell and element order as in cell_spec.py.

  * check_indices: what the call refuses before it looks at a cell: fewer than 64 or more than 128 indices, an index >= 128, indices not
    strictly ascending (which covers duplicates).
  * recover_coefficients_spec: the spec's route as written there.  Vanishing polynomial of the missing cells, one short factor (y - a_m) per
    missing cell spread by 64 (Z(x) = prod (x^64 - a_m)); E = the known evaluations in natural order, 0 at the missing ones; (E Z) by an 8192-
    point inverse transform; division by Z on the coset 7 <w>; the first 4096 coefficients of the quotient.  About 0.7 s per call.
  * recover_coefficients_columns: the device's route.  p(x) = sum_{r<64} x^r P_r(x^64), deg P_r < 64; the interpolant of cell k has the
    coefficients u_r(k) = P_r(a_k), a_k = w128^rev7(k), so each column r is an erasure-decoding problem of length 128 with the same known
    positions.  With S(y) = prod_{m missing} (y - a_m):
        u        = dit64(cell k, w64^-1) / 64, coefficient t times h_k^-t              (per known cell)
        c        = dit128(u_r(k) S(a_k), 0 at the missing k; w128^-1) / 128            (coefficients of P_r S, degree < 128)
        q        = dif128(c_i g^i; w128)[k] / S(g a_k)                                 (P_r on the coset g <w128>, g = w)
        P_r[i]   = dit128(q; w128^-1)[i] / 128 g^-i
    f_(64u+r) = P_r[u] for u < 64.  P_r[64..127] is zero exactly when the cells lie on one polynomial of degree < 4096; the second return value
    says whether any of them is not.  dif: natural order in, bit-reversed out; dit: bit-reversed in, natural out (fk20_spec); cell order is
    the bit-reversed order of the 128-point domain, element order that of the 64-point coset, so no permutation appears.
  * cells_from_coefficients: the 128 cells of a coefficient vector (what both calls return for it), also through the device's last two steps
    (cells_from_coefficients_columns): P_r(a_k) by dif128 of (P_r | 0^64), then per cell coefficient r times h_k^r and dif64."""
from oracle.pyref import R

import cell_spec as cs
import fk20_spec as fk

N_FE = cs.N_FE
CELL_FE = cs.CELL_FE
CELLS = cs.CELLS_PER_EXT_BLOB
W128 = fk.W128
W64 = cs.W64


def check_indices(cell_indices):
    ix = [int(i) for i in cell_indices]
    if len(ix) < CELLS // 2 or len(ix) > CELLS:
        raise cs.BadArgs("number of cells")
    if any(i < 0 or i >= CELLS for i in ix):
        raise cs.BadArgs("cell index")
    if any(b <= a for a, b in zip(ix, ix[1:])):
        raise cs.BadArgs("cell indices not strictly ascending")
    return ix


def _check_input(cell_indices, cells):
    ix = check_indices(cell_indices)
    if len(cells) != len(ix):
        raise cs.BadArgs("length mismatch")
    return ix, [cs.cell_values(c) for c in cells]


# ---- the consensus-spec route
def recover_coefficients_spec(cell_indices, cells, with_high=False):
    ix, vals = _check_input(cell_indices, cells)
    missing = [k for k in range(CELLS) if k not in ix]
    short = [1]                                                   # prod (y - a_m), lowest coefficient first
    for m in missing:
        a = fk.a_k(m)
        short = [((short[d - 1] if d else 0) - a * (short[d] if d < len(short) else 0)) % R for d in range(len(short) + 1)]
    Z = [0] * cs.EXT
    for i, c in enumerate(short):
        Z[CELL_FE * i] = c
    brp = [0] * cs.EXT
    for k, v in zip(ix, vals):
        brp[CELL_FE * k:CELL_FE * (k + 1)] = v
    E = [brp[cs.rev(i, 13)] for i in range(cs.EXT)]               # value at w^i, 0 where unknown
    inv, winv = pow(cs.EXT, -1, R), pow(cs.W, -1, R)
    Zev = cs._ntt(Z, cs.W)
    EZ = [x * inv % R for x in cs._ntt([e * z % R for e, z in zip(E, Zev)], winv)]
    g = 7
    shift = lambda p, s: [c * pow(s, i, R) % R for i, c in enumerate(p)]
    num, den = cs._ntt(shift(EZ, g), cs.W), cs._ntt(shift(Z, g), cs.W)
    q = [x * pow(y, -1, R) % R for x, y in zip(num, den)]
    qc = shift([x * inv % R for x in cs._ntt(q, winv)], pow(g, -1, R))
    return (qc[:N_FE], qc[N_FE:]) if with_high else qc[:N_FE]


# ---- the device's route
def vanishing_tables(ix, g=cs.W):
    """S(a_k) and 1 / S(g a_k) in cell order (S = 1 when nothing is missing)"""
    missing = [fk.a_k(m) for m in range(CELLS) if m not in ix]
    sd, sci = [], []
    for k in range(CELLS):
        a = fk.a_k(k)
        d = c = 1
        for am in missing:
            d = d * (a - am) % R
            c = c * (g * a - am) % R
        sd.append(d)
        sci.append(pow(c, -1, R))
    return sd, sci


def cell_coefficients(vals, k):
    """u_t(k): dit64 of the cell's elements as they stand, / 64, times h_k^-t (equal to cell_spec.cell_interpolant)"""
    q = fk.dit(vals, pow(W64, -1, R))
    inv64, hinv = pow(CELL_FE, -1, R), pow(cs.coset_shift(k), -1, R)
    return [q[t] * inv64 % R * pow(hinv, t, R) % R for t in range(CELL_FE)]


def recover_coefficients_columns(cell_indices, cells):
    """(the 4096 coefficients, whether any column had a nonzero coefficient 64..127)"""
    ix, vals = _check_input(cell_indices, cells)
    g = cs.W
    assert pow(g, 2 * CELL_FE, R) != 1
    u = {k: cell_coefficients(v, k) for k, v in zip(ix, vals)}
    sd, sci = vanishing_tables(ix, g)
    inv128, w128i, gi = pow(2 * CELL_FE, -1, R), pow(W128, -1, R), pow(g, -1, R)
    f = [0] * N_FE
    high = False
    for r in range(CELL_FE):
        ev = [u[k][r] * sd[k] % R if k in u else 0 for k in range(CELLS)]
        c = [x * inv128 % R for x in fk.dit(ev, w128i)]
        on_coset = fk.dif([x * pow(g, i, R) % R for i, x in enumerate(c)], W128)
        q = [x * y % R for x, y in zip(on_coset, sci)]
        p = [x * inv128 % R * pow(gi, i, R) % R for i, x in enumerate(fk.dit(q, w128i))]
        high |= any(p[CELL_FE:])
        for i in range(CELL_FE):
            f[CELL_FE * i + r] = p[i]
    return f, high


# ---- cells of a coefficient vector
def cells_from_coefficients(f):
    """the 128 cells of the polynomial with the 4096 coefficients f"""
    return cs.compute_cells(fk.blob_from_coefficients(f))


def cells_from_coefficients_columns(f):
    """the same by the device's last two steps"""
    vals = [fk.dif([f[CELL_FE * i + r] for i in range(CELL_FE)] + [0] * CELL_FE, W128) for r in range(CELL_FE)]   # vals[r][k] = P_r(a_k)
    out = []
    for k in range(CELLS):
        h = cs.coset_shift(k)
        el = fk.dif([vals[r][k] * pow(h, r, R) % R for r in range(CELL_FE)], W64)
        out.append(b"".join(v.to_bytes(32, "big") for v in el))
    return out
