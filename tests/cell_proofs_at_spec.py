"""CPU restatement of compute_cell_kzg_proofs_at's route (k_cell_quotient.hip), the proof of one chosen cell as the commitment to its own
quotient, in Python integers.

  * f_0 .. f_4095: the blob polynomial's coefficients (cell_spec.blob_coefficients); a_k = w128^rev7(k) (fk20_spec.a_k).
  * q_k = p div (X^64 - a_k) has 4032 coefficients and, column by column (r < 64), q[64u + r] = f[64(u+1) + r] + a_k q[64(u+1) + r] for
    u = 62 .. 0, from q[64 * 63 + r] = 0: quotient_coefficients, written the way the kernel's 64 lanes run it.
  * One forward transform of size 4096 (fk20_spec.dif at W4096: natural order in, bit-reversed order out) leaves q_k(w4096^rev12(i)) at
    position i.  That is the order of a blob and of the Lagrange setup points, so sum_i s_i [L_i(tau)]_1 = [q_k(tau)]_1: quotient_scalars.
  * lagrange_at(t): the values L_i(t) of the Lagrange basis in that same order -- the stand-in of the setup points over Fr."""
from oracle.pyref import R

import cell_spec as cs
import fk20_spec as fk

N_FE = cs.N_FE
CELL_FE = cs.CELL_FE


def quotient_coefficients(f, k):
    """the 4096 values the kernel holds before its transform: q_k's 4032 coefficients, then 64 zeros"""
    a = fk.a_k(k)
    q = [0] * N_FE
    for r in range(CELL_FE):
        acc = 0
        for u in range(CELL_FE - 2, -1, -1):
            acc = (acc * a + f[CELL_FE * (u + 1) + r]) % R
            q[CELL_FE * u + r] = acc
    return q


def quotient_scalars(f, k):
    """the MSM's scalars: q_k in evaluation form on the blob's own domain, in blob order"""
    return fk.dif(quotient_coefficients(f, k), fk.W4096)


def lagrange_at(t):
    """L_i(t) for the domain point w4096^rev12(i), i < 4096: (t^4096 - 1) x_i / (4096 (t - x_i)); t must lie outside the domain"""
    z = (pow(t, N_FE, R) - 1) * pow(N_FE, -1, R) % R
    xs = [pow(fk.W4096, cs.rev(i, 12), R) for i in range(N_FE)]
    return [z * x % R * pow(t - x, -1, R) % R for x in xs]
