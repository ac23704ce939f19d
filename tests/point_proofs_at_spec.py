"""CPU restatement of compute_kzg_proofs_at's route (k_point_quotient.hip), the opening of a blob at one point as the commitment to its own
quotient, in Python integers.

  * f_0 .. f_(n-1): the blob polynomial's coefficients (cell_spec.blob_coefficients; n = 4096).
  * q = (p - p(z)) / (X - z) has n - 1 coefficients: q[n-1] = 0, q[j] = f[j+1] + z q[j+1], and y = p(z) = f[0] + z q[0], for every z -- no
    inversion, and nothing special about a z inside the domain: synthetic_division, the plain chain.
  * blocked_division: the same values the way the kernel's n / 8 threads find them.  With Q[j] = q[j-1] (Q[0] = y): thread t runs the chain
    over its own 8 coefficients with zero carry-in (its segment value S_t), a suffix scan over the S_t with the powers z^8, z^16, .. takes
    log2(n / 8) doubling rounds and leaves Q[8t] at thread t, and a second pass of 8 steps starts from the carry Q[8(t+1)].
  * One forward transform of size 4096 (fk20_spec.dif at W4096: natural order in, bit-reversed order out) leaves q(w4096^rev12(i)) at
    position i.  That is the order of a blob and of the Lagrange setup points, so sum_i s_i [L_i(tau)]_1 = [q(tau)]_1: quotient_scalars."""
from oracle.pyref import R

import fk20_spec as fk

SEG = 8


def synthetic_division(f, z):
    """(q, y): the n values the kernel holds before its transform (q's n - 1 coefficients, then a zero) and p(z)"""
    n = len(f)
    q = [0] * n
    for j in range(n - 2, -1, -1):
        q[j] = (f[j + 1] + z * q[j + 1]) % R
    return q, (f[0] + z * q[0]) % R


def blocked_division(f, z):
    """the same (q, y) by segments of 8, doubling rounds and a second pass"""
    n = len(f)
    threads = n // SEG
    assert threads * SEG == n and threads & (threads - 1) == 0
    # first pass: zero carry-in
    acc = []
    for t in range(threads):
        a = f[SEG * t + SEG - 1]
        for i in range(SEG - 2, -1, -1):
            a = (a * z + f[SEG * t + i]) % R
        acc.append(a)
    # suffix scan: round d adds z^(8 d) times the value d threads up
    zp, d, rounds = pow(z, SEG, R), 1, 0
    while d < threads:
        acc = [(acc[t] + zp * acc[t + d]) % R if t + d < threads else acc[t] for t in range(threads)]
        zp, d, rounds = zp * zp % R, 2 * d, rounds + 1
    assert rounds == threads.bit_length() - 1
    # second pass: from the carry Q[8(t+1)] down, Q[8t+i] = q[8t+i-1]
    q = [0] * n
    for t in range(threads):
        a = acc[t + 1] if t + 1 < threads else 0
        for i in range(SEG - 1, -1, -1):
            a = (a * z + f[SEG * t + i]) % R
            if SEG * t + i > 0:
                q[SEG * t + i - 1] = a
    return q, acc[0]


def quotient_scalars(f, z):
    """the MSM's scalars: q in evaluation form on the blob's own domain, in blob order"""
    return fk.dif(blocked_division(f, z)[0], fk.W4096)
