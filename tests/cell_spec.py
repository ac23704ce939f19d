"""CPU restatement of EIP-7594 cell proofs (consensus specs fulu/polynomial-commitments-sampling.md), the yardstick of
kzg355_verify_cell_kzg_proof_batch.  Big-integer arithmetic in Python plus the C oracle's g1_lincomb / pairings_verify / g1_validate.

  * FIELD_ELEMENTS_PER_CELL = 64, BYTES_PER_CELL = 2048, CELLS_PER_EXT_BLOB = 128, extended domain 8192.
  * w = 7^((r-1)/8192); brp = the 13-bit bit-reversal permutation of [w^0 .. w^8191].  Cell k is the blob polynomial at brp[64k .. 64k+63]:
    element j of cell k sits at h_k * w64^rev6(j), h_k = brp[64k] = w^rev7(k), w64 = w^128.  Cells 0..63 are the blob itself.
  * verify_cell_kzg_proof_batch(commitments, cell_indices, cells, proofs): n = 0 -> True; a cell index >= 128, a commitment / proof failing
    validate_kzg_g1 or a cell element >= r -> BadArgs.  Commitments are deduplicated by bytes in first-appearance order.
    r = int(SHA256(T)) mod r_BLS, T = "RCKZGCBATCH__V1_" | u64be(4096) | u64be(64) | u64be(#unique) | u64be(n) | unique commitments |
    per cell: u64be(commitment position) | u64be(cell index) | cell | proof.
    Check e(LL, [tau^64]_2) == e(RL, G2) with LL = sum r^k pi_k, RL = sum_i w_i C_i - [I(tau)]_1 + sum_k r^k h_k^64 pi_k, w_i = sum of r^k over
    the cells of C_i, I = sum_k r^k I_k (I_k: the degree < 64 interpolant of cell k on its coset), [I(tau)]_1 = sum_t I_t [tau^t]_1.
  * Cell proofs: pi_k = sum_t q_t [tau^t]_1 with q = (p - I_k) / (X^64 - h_k^64)."""
import hashlib
import os

from oracle.pyref import R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

N_FE = 4096
CELL_FE = 64
BYTES_PER_CELL = 2048
CELLS_PER_EXT_BLOB = 128
EXT = 8192
DOMAIN = b"RCKZGCBATCH__V1_"
W = pow(7, (R - 1) // EXT, R)
W64 = pow(W, 128, R)


class BadArgs(Exception):
    pass


def rev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


def coset_shift(k):
    return pow(W, rev(k, 7), R)


def _ntt(a, root):
    """natural-order DFT of len(a) (power of two) values at root^i, iterative radix-2"""
    n = len(a)
    bits = n.bit_length() - 1
    a = [a[rev(i, bits)] for i in range(n)]
    m = 2
    while m <= n:
        wm = pow(root, n // m, R)
        for s in range(0, n, m):
            wk = 1
            for j in range(m // 2):
                u, t = a[s + j], a[s + j + m // 2] * wk % R
                a[s + j], a[s + j + m // 2] = (u + t) % R, (u - t) % R
                wk = wk * wm % R
        m *= 2
    return a


def blob_coefficients(blob):
    """monomial coefficients of the blob polynomial (the blob holds its values at the bit-reversed 4096-point domain)"""
    vals = [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(N_FE)]
    nat = [vals[rev(i, 12)] for i in range(N_FE)]                 # value at w4096^i
    w4096 = W * W % R
    c = _ntt(nat, pow(w4096, -1, R))
    inv = pow(N_FE, -1, R)
    return [x * inv % R for x in c]


def compute_cells(blob):
    """the 128 cells of the 2x extension (NTT in Python integers)"""
    coeffs = blob_coefficients(blob)
    ev = _ntt(coeffs + [0] * N_FE, W)                             # value at w^i
    brp = [ev[rev(i, 13)] for i in range(EXT)]
    return [b"".join(v.to_bytes(32, "big") for v in brp[CELL_FE * k:CELL_FE * k + CELL_FE]) for k in range(CELLS_PER_EXT_BLOB)]


def cell_values(cell):
    vals = [int.from_bytes(cell[32 * j:32 * j + 32], "big") for j in range(CELL_FE)]
    if any(v >= R for v in vals):
        raise BadArgs("non-canonical cell element")
    return vals


def cell_interpolant(vals, k):
    """degree < 64 interpolant of the values of cell k on its coset h_k <w64>"""
    h = coset_shift(k)
    u = [vals[rev(j, 6)] for j in range(CELL_FE)]                 # value at h w64^j
    q = _ntt(u, pow(W64, -1, R))
    inv64, hinv = pow(CELL_FE, -1, R), pow(h, -1, R)
    return [q[t] * inv64 % R * pow(hinv, t, R) % R for t in range(CELL_FE)]


def load_monomial(n=N_FE):
    raw = open(os.path.join(GOLDEN, "setup_g1_monomial.bin"), "rb").read()
    return [raw[48 * i:48 * i + 48] for i in range(n)]


def g2_points():
    raw = open(os.path.join(GOLDEN, "trusted_setup_g2.bin"), "rb").read()
    return [raw[96 * i:96 * i + 96] for i in range(65)]


def _be(v):
    return (v % R).to_bytes(32, "big")


def lincomb(o, points, scalars):
    return o.g1_lincomb(points, [_be(s) for s in scalars])


def cell_proofs(o, blob, mono, cells=range(CELLS_PER_EXT_BLOB)):
    """pi_k = sum_t q_t [tau^t]_1, q = (p - I_k) / (X^64 - h_k^64): the quotient of p by X^64 - a (its remainder is I_k)"""
    p = blob_coefficients(blob)
    out = []
    for k in cells:
        a = pow(coset_shift(k), CELL_FE, R)
        q = [0] * (N_FE - CELL_FE)
        rem = list(p)
        for i in range(N_FE - 1, CELL_FE - 1, -1):                # long division by X^64 - a
            c = rem[i]
            q[i - CELL_FE] = c
            rem[i - CELL_FE] = (rem[i - CELL_FE] + c * a) % R
            rem[i] = 0
        out.append(lincomb(o, mono[:N_FE - CELL_FE], q))
    return out


def challenge(commitments, cell_indices, cells, proofs):
    uniq, pos = [], []
    for c in commitments:
        if c not in uniq:
            uniq.append(c)
        pos.append(uniq.index(c))
    n = len(commitments)
    t = [DOMAIN + N_FE.to_bytes(8, "big") + CELL_FE.to_bytes(8, "big") + len(uniq).to_bytes(8, "big") + n.to_bytes(8, "big") + b"".join(uniq)]
    for k in range(n):                                            # (joined once: appending to one bytes object copies it per cell)
        t.append(pos[k].to_bytes(8, "big") + int(cell_indices[k]).to_bytes(8, "big") + bytes(cells[k]) + bytes(proofs[k]))
    return int.from_bytes(hashlib.sha256(b"".join(t)).digest(), "big") % R, uniq, pos


def verify_cell_kzg_proof_batch(o, commitments, cell_indices, cells, proofs, mono=None, g2=None, intermediates=False):
    """the spec's check; intermediates=True returns (ok, {r, itau, ll, rl}) with r as 32 big-endian bytes and the points compressed"""
    n = len(commitments)
    if not (len(cell_indices) == len(cells) == len(proofs) == n):
        raise BadArgs("length mismatch")
    if n == 0:
        return (True, None) if intermediates else True
    if any(int(i) >= CELLS_PER_EXT_BLOB for i in cell_indices):
        raise BadArgs("cell index")
    for b in list(commitments) + list(proofs):
        if o.g1_validate(b) != 0:
            raise BadArgs("validate_kzg_g1")
    vals = [cell_values(c) for c in cells]
    mono = mono or load_monomial(CELL_FE)
    g2 = g2 or g2_points()
    r, uniq, pos = challenge(commitments, cell_indices, cells, proofs)
    rp = [pow(r, k, R) for k in range(n)]
    w = [0] * len(uniq)
    for k in range(n):
        w[pos[k]] = (w[pos[k]] + rp[k]) % R
    # I by columns: weighted column sums, then one interpolation per column
    cols = {}
    for k in range(n):
        c = int(cell_indices[k])
        acc = cols.setdefault(c, [0] * CELL_FE)
        for j in range(CELL_FE):
            acc[j] = (acc[j] + rp[k] * vals[k][j]) % R
    I = [0] * CELL_FE
    for c, acc in cols.items():
        for t, v in enumerate(cell_interpolant(acc, c)):
            I[t] = (I[t] + v) % R
    itau = lincomb(o, mono[:CELL_FE], I)
    ll = lincomb(o, list(proofs), rp)
    rl = lincomb(o, list(uniq) + list(mono[:CELL_FE]) + list(proofs),
                 w + [(-x) % R for x in I] + [rp[k] * pow(coset_shift(int(cell_indices[k])), CELL_FE, R) % R for k in range(n)])
    ok = o.pairings_verify(ll, g2[CELL_FE], rl, g2[0])
    if intermediates:
        return ok, {"r": _be(r), "itau": itau, "ll": ll, "rl": rl}
    return ok


def single_cell_check(o, commitment, k, cell, proof, mono=None, g2=None):
    """e(pi, [tau^64]_2 - [h^64]_2) == e(C - [I_k(tau)]_1, G2), written as e(pi, [tau^64]_2) == e(C - [I_k(tau)]_1 + h^64 pi, G2)"""
    mono = mono or load_monomial(CELL_FE)
    g2 = g2 or g2_points()
    I = cell_interpolant(cell_values(cell), k)
    rhs = lincomb(o, [commitment] + list(mono[:CELL_FE]) + [proof], [1] + [(-x) % R for x in I] + [pow(coset_shift(k), CELL_FE, R)])
    return o.pairings_verify(proof, g2[CELL_FE], rhs, g2[0])
