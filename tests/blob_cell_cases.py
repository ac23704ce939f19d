"""What verify_blob_cell_proofs_batch must answer, from tests/cell_spec.py alone (nothing here calls the library under test).

A group is n blobs with their n commitments and 128 n cell proofs.  By definition its answer is verify_cell_kzg_proof_batch on 128 n cells, the cell
at position 128 b + k carrying commitment b, cell index k, cell k of blob b's extension and proof 128 b + k: group_args() builds those four arrays
and expected() the 176 bytes r | [I(tau)]_1 | LL | RL and the verdict.

The device does not interpolate cell by cell.  With f_b the monomial coefficients of blob b and a_k = h_k^64 = w128^rev7(k),
    I[t] = sum_{u<64} W[u] * ( sum_b r^(128 b) f_{b,64u+t} ),    W[u] = sum_{k<128} r^k a_k^u
(weights(), interpolant_from_coefficients()); interpolant_by_cells() is the definition, sum over the cells of r^(128 b + k) times
cell_spec.cell_interpolant.  tests/test_blob_cell_spec.py holds the two against each other."""
import cell_spec as cs

R = cs.R
N = cs.CELLS_PER_EXT_BLOB
INF = b"\xc0" + bytes(47)


def group_args(cells_per_blob, commitments, cell_proofs):
    """(commitments, cell_indices, cells, proofs) of verify_cell_kzg_proof_batch for one group of blobs; cells_per_blob[b] = the 128 cells of blob b"""
    n = len(commitments)
    assert len(cells_per_blob) == n and all(len(row) == N for row in cells_per_blob) and len(cell_proofs) == N * n
    return ([commitments[b] for b in range(n) for _ in range(N)], [k for _ in range(n) for k in range(N)],
            [cells_per_blob[b][k] for b in range(n) for k in range(N)], list(cell_proofs))


def expected(o, cells_per_blob, commitments, cell_proofs, mono=None, g2=None):
    """(176 bytes, verdict) of a group with at least one blob; cell_spec.BadArgs as the spec raises it"""
    ok, parts = cs.verify_cell_kzg_proof_batch(o, *group_args(cells_per_blob, commitments, cell_proofs), mono=mono, g2=g2, intermediates=True)
    return parts["r"] + parts["itau"] + parts["ll"] + parts["rl"], ok


def weights(r):
    """W[u] = sum_k r^k a_k^u, u < 64"""
    a = [pow(cs.coset_shift(k), cs.CELL_FE, R) for k in range(N)]
    rp = [pow(r, k, R) for k in range(N)]
    return [sum(rp[k] * pow(a[k], u, R) for k in range(N)) % R for u in range(cs.CELL_FE)]


def interpolant_from_coefficients(r, coeffs):
    """coeffs[b]: the 4096 monomial coefficients of blob b"""
    W, rb = weights(r), [pow(r, N * b, R) for b in range(len(coeffs))]
    return [sum(W[u] * sum(rb[b] * f[cs.CELL_FE * u + t] for b, f in enumerate(coeffs)) for u in range(cs.CELL_FE)) % R for t in range(cs.CELL_FE)]


def interpolant_by_cells(r, cells_per_blob):
    I = [0] * cs.CELL_FE
    for b, row in enumerate(cells_per_blob):
        for k, cell in enumerate(row):
            wt = pow(r, N * b + k, R)
            for t, v in enumerate(cs.cell_interpolant(cs.cell_values(cell), k)):
                I[t] = (I[t] + wt * v) % R
    return I
