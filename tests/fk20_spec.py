"""CPU restatement of compute_cells_and_kzg_proofs by FK20, the yardstick of kzg355_compute_cells_and_kzg_proofs (k_cell_compute.hip).

  * f_0 .. f_4095: the blob polynomial's coefficients (cell_spec.blob_coefficients); a_k = h_k^64 = w128^rev7(k), w128 = w^64.
  * H_e = sum_{m >= 64(e+1)} f_m [tau^(m - 64(e+1))]_1 (e < 63) and pi_k = sum_e a_k^e H_e, the quotient of p by X^64 - a_k at tau: h_points and
    proofs_from_h, with the oracle's g1_lincomb (one 4032-term lincomb for H_0; about 11 s in all).
  * The device's index route, restated over Fr with [tau^j]_1 replaced by t^j (every step is linear, so it must give q_k(t)):
      X_r   = dif(x_r | 0^64),       x_r[v] = T(64v + r)                         (setup, bit-reversed order)
      C_r   = dif(c_r | 0^64),       c_r[d] = f_(64(63-d)+r) / 128              (field stage, bit-reversed order)
      Z[i]  = sum_r C_r[i] X_r[i]                                                 (fixed-base stage)
      conv  = dit(Z, w128^-1);  h_e = conv[62 - e] (e < 63), 0 above;  pi = dif(h)   (G1 stage; pi comes out in cell order)
    dif: natural order in, bit-reversed out; dit: bit-reversed in, natural out (both unnormalised DFTs at the given root).
  * Cells 64..127, read as one array: dif of f_m w^m at w4096 (the coset evaluations in 12-bit bit-reversed order)."""
from oracle.pyref import R

import cell_spec as cs

N_FE = cs.N_FE
CELL_FE = cs.CELL_FE
FFT = 2 * CELL_FE
W128 = pow(cs.W, 64, R)
W4096 = cs.W * cs.W % R


def a_k(k):
    return pow(W128, cs.rev(k, 7), R)


def dif(a, root):
    a = list(a)
    n = len(a)
    h = n // 2
    while h >= 1:
        ws = pow(root, n // (2 * h), R)
        for s in range(0, n, 2 * h):
            wj = 1
            for j in range(h):
                u, v = a[s + j], a[s + j + h]
                a[s + j], a[s + j + h] = (u + v) % R, (u - v) * wj % R
                wj = wj * ws % R
        h //= 2
    return a


def dit(a, root):
    a = list(a)
    n = len(a)
    h = 1
    while h < n:
        ws = pow(root, n // (2 * h), R)
        for s in range(0, n, 2 * h):
            wj = 1
            for j in range(h):
                u, v = a[s + j], a[s + j + h] * wj % R
                a[s + j], a[s + j + h] = (u + v) % R, (u - v) % R
                wj = wj * ws % R
        h *= 2
    return a


# ---- the device route over Fr
def setup_columns(T):
    """X_r for r < 64 from T(j) = the stand-in of [tau^j]_1"""
    return [dif([T(CELL_FE * v + r) for v in range(CELL_FE)] + [0] * CELL_FE, W128) for r in range(CELL_FE)]


def field_columns(f):
    inv = pow(FFT, -1, R)
    return [dif([f[CELL_FE * (CELL_FE - 1 - d) + r] * inv % R for d in range(CELL_FE)] + [0] * CELL_FE, W128) for r in range(CELL_FE)]


def route_proofs(f, X):
    C = field_columns(f)
    Z = [sum(C[r][i] * X[r][i] for r in range(CELL_FE)) % R for i in range(FFT)]
    conv = dit(Z, pow(W128, -1, R))
    h = [conv[CELL_FE - 2 - e] for e in range(CELL_FE - 1)] + [0] * (FFT - CELL_FE + 1)
    return dif(h, W128), h[:CELL_FE]


def route_cells(blob):
    """cells 64..127 as the field stage computes them (inverse dit, twist by w^m, dif), as 64 cells of 2048 bytes"""
    vals = [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(N_FE)]
    inv = pow(N_FE, -1, R)
    f = [x * inv % R for x in dit(vals, pow(W4096, -1, R))]
    ev = dif([f[m] * pow(cs.W, m, R) % R for m in range(N_FE)], W4096)
    flat = b"".join(v.to_bytes(32, "big") for v in ev)
    return f, [flat[cs.BYTES_PER_CELL * k:cs.BYTES_PER_CELL * (k + 1)] for k in range(CELL_FE)]


def quotient_at(f, k, t):
    """q_k(t), q_k = p div (X^64 - a_k)"""
    a = a_k(k)
    rem = list(f)
    q = [0] * (N_FE - CELL_FE)
    for i in range(N_FE - 1, CELL_FE - 1, -1):
        c = rem[i]
        q[i - CELL_FE] = c
        rem[i - CELL_FE] = (rem[i - CELL_FE] + c * a) % R
    acc = 0
    for c in reversed(q):
        acc = (acc * t + c) % R
    return acc


def h_field(f, t):
    """H_e with [tau^j]_1 replaced by t^j"""
    return [sum(f[m] * pow(t, m - CELL_FE * (e + 1), R) for m in range(CELL_FE * (e + 1), N_FE)) % R for e in range(CELL_FE - 1)]


# ---- the group form, through the oracle
def h_points(o, blob, mono):
    """H_0 .. H_62 compressed; mono: the 4096 monomial points (cell_spec.load_monomial())"""
    f = cs.blob_coefficients(blob)
    return [cs.lincomb(o, mono[:N_FE - CELL_FE * (e + 1)], f[CELL_FE * (e + 1):]) for e in range(CELL_FE - 1)]


def proofs_from_h(o, H, cells=range(cs.CELLS_PER_EXT_BLOB)):
    return [cs.lincomb(o, H, [pow(a_k(k), e, R) for e in range(len(H))]) for k in cells]
