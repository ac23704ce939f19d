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
  * Cells 64..127, read as one array: dif of f_m w^m at w4096 (the coset evaluations in 12-bit bit-reversed order).
  * Edge-case constructions: blob_from_coefficients (the inverse of cell_spec.blob_coefficients), columns_blob / column_blob (blobs whose
    circulant columns c_r are chosen, so the fixed-base scalars C_r[i] are known), column_pair / column_vanishing (C_r[i0] set, or 0 at chosen
    bins), and comb_digits / comb_doubling_windows (k_cc_msm's signed 4-bit recoding and the windows where its accumulator meets +- the point
    it adds)."""
import random

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


# ---- blobs with chosen columns
def blob_from_coefficients(f):
    """the blob of the polynomial with coefficients f (len <= 4096): dif at w4096 gives p(w4096^rev12(i)) in blob order"""
    f = [x % R for x in f] + [0] * (N_FE - len(f))
    return b"".join(v.to_bytes(32, "big") for v in dif(f, W4096))


def columns_blob(cols):
    """the blob whose column r is c_r = cols[r] (len <= 64): f_(64(63-d)+r) = 128 c_r[d]; missing columns are 0"""
    f = [0] * N_FE
    for r, c in enumerate(cols):
        for d, v in enumerate(c):
            f[CELL_FE * (CELL_FE - 1 - d) + r] = FFT * v % R
    return blob_from_coefficients(f)


def column_blob(s):
    """p = sum_r 128 s_r X^(4032+r): c_r = (s_r, 0, ...), so C_r[i] = s_r in every bin i"""
    return columns_blob([[v] for v in s])


def bin_point(i):
    """the point of bin i of C_r = dif(c_r | 0^64): C_r[i] = c_r(w128^rev7(i))"""
    return pow(W128, cs.rev(i, 7), R)


def column_pair(target, i0, b):
    """c = (a, b) with C[i0] = a + b w128^rev7(i0) = target; C[i] = target + b (w128^rev7(i) - w128^rev7(i0)) elsewhere"""
    return [(target - b * bin_point(i0)) % R, b % R]


def column_vanishing(bins, g):
    """c = g(Y) prod_(i in bins) (Y - w128^rev7(i)): C[i] = 0 in those bins (g: low coefficients first)"""
    c = [x % R for x in g]
    for i in bins:
        x = bin_point(i)
        c = [((c[d - 1] if d else 0) - x * (c[d] if d < len(c) else 0)) % R for d in range(len(c) + 1)]
    assert len(c) <= CELL_FE
    return c


# ---- k_cc_msm's comb: lane r adds d_w [16^w] X_r[i] for the signed digits d_w of C_r[i], w = 0 .. 63, starting from the first d_w != 0
COMB_WINDOWS = 64
COMB_BIAS = int("8" * COMB_WINDOWS, 16)                         # 0x888...8


def comb_digits(k):
    """the device recoding: e = k + 0x888...8 (eight 32-bit words, the carry out of the top word dropped), d_w = nibble_w(e) - 8 in [-8, 7]"""
    e = (k + COMB_BIAS) % (1 << 256)
    return [((e >> (4 * w)) & 15) - 8 for w in range(COMB_WINDOWS)]


def comb_doubling_windows(k):
    """replays the accumulation mod r (as multiples of X): [("dbl", w)] where the accumulator equals the point added (the addition must
    double), [("inv", w)] where it equals its negation (the result is infinity)"""
    acc, out = 0, []
    for w, d in enumerate(comb_digits(k)):
        if not d:
            continue
        p = d * pow(16, w, R) % R
        if acc:                                                  # started (a started accumulator is never 0 for k < r: see the tests)
            if acc == p:
                out.append(("dbl", w))
            elif acc == (-p) % R:
                out.append(("inv", w))
        acc = (acc + p) % R
    return out


# k* = 14 16^63 - r: the one scalar below r whose last addition (window 63, digit 7) doubles
K_STAR = 14 * 16 ** 63 - R


def from_digits(ds):
    return sum(d * 16 ** w for w, d in enumerate(ds))


def comb_corpus():
    """(name, k) scalars below r at the recoding's corners: small and top values, k* and its neighbours, digit patterns (all -8, all 7,
    alternating, a lone -8) under a nonnegative top digit, then seeded random digit strings; at least 64 distinct scalars"""
    out = [("0", 0), ("1", 1), ("2", 2), ("r-1", R - 1), ("r-2", R - 2), ("(r-1)/2", (R - 1) // 2), ("2^252", 2 ** 252), ("2^252-1", 2 ** 252 - 1),
           ("k*", K_STAR), ("k*+1", K_STAR + 1), ("k*-1", K_STAR - 1), ("k*+16^62", K_STAR + 16 ** 62), ("k*-16^62", K_STAR - 16 ** 62)]
    low = COMB_WINDOWS - 1
    pats = []
    for t in range(1, 8):
        pats.append((f"-8s under {t}", [-8] * low + [t]))
        pats.append((f"7s under {t}", [7] * low + [t]))
        pats.append((f"-8/7 under {t}", [-8 if w % 2 == 0 else 7 for w in range(low)] + [t]))
        pats.append((f"7/-8 under {t}", [7 if w % 2 == 0 else -8 for w in range(low)] + [t]))
    pats.append(("7s, 3 at 62, under 7", [7] * (low - 1) + [3, 7]))              # 0x7377..7: 7 in every window r allows
    for t in (1, 7):
        for w0 in (0, 31, 62):
            pats.append((f"-8 at {w0} under {t}", [-8 if w == w0 else 0 for w in range(low)] + [t]))
    for w0 in (0, 31, 62):
        pats.append((f"7 at {w0}", [7 if w == w0 else 0 for w in range(COMB_WINDOWS)]))
    out += [(n, from_digits(ds)) for n, ds in pats if from_digits(ds) < R]
    rng = random.Random(0xc0b)
    while len(out) < 72:
        ds = [rng.choice((-8, -7, -1, 0, 1, 7)) for _ in range(low)] + [rng.randrange(8)]
        if 0 <= from_digits(ds) < R:
            out.append((f"digits seed {len(out)}", from_digits(ds)))
    return out


# ---- the group form, through the oracle
G1_INF = bytes([0xc0]) + bytes(47)


def sparse_lincomb(o, points, scalars):
    """lincomb over the nonzero scalars and finite points only (the point at infinity if none is left)"""
    terms = [(p, s % R) for p, s in zip(points, scalars) if s % R and p != G1_INF]
    return cs.lincomb(o, [p for p, _ in terms], [s for _, s in terms]) if terms else G1_INF


def h_points(o, blob, mono):
    """H_0 .. H_62 compressed; mono: the 4096 monomial points (cell_spec.load_monomial()).  Zero coefficients are skipped, so sparse and
    low-degree blobs are cheap."""
    f = cs.blob_coefficients(blob)
    return [sparse_lincomb(o, mono[:N_FE - CELL_FE * (e + 1)], f[CELL_FE * (e + 1):]) for e in range(CELL_FE - 1)]


def proofs_from_h(o, H, cells=range(cs.CELLS_PER_EXT_BLOB)):
    return [sparse_lincomb(o, H, [pow(a_k(k), e, R) for e in range(len(H))]) for k in cells]
