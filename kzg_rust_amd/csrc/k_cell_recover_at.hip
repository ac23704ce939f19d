// k_cell_recover_at.hip -- recover_cells_and_kzg_proofs_at on the device: the chosen cells of recovered blobs.  The
// erasure decoding is that of k_cell_recover.hip (k_rc_vanish, k_rc_interp, k_rc_columns), unchanged, and the proofs are those of
// k_cell_quotient.hip (k_cq_quotient on the coefficients k_rc_columns leaves) with the fixed-base MSM behind it.  What is new here is the cell
// stage driven by the chunk's pair list: k_rc_cells writes all 128 cells of every blob, 256 KiB each; this one writes the pairs asked for.
#define KZG_FP_MUL_NOINLINE 1
#include "kernels.h"
#include "cell_domain.h"

namespace kzg {

// workgroup = pair (blob, cell k, slot): the arithmetic of k_rc_cells on u[blob][k][r] = P_r(a_k) -- coefficient r times h_k^r, dif64 (root w64)
// -> the cell's 64 elements in their order -- into slot pr.slot of `out`; nothing for a refused blob (the host gives it no pair; the test on its
// descriptor keeps the kernel right on its own)
__global__ void __launch_bounds__(CELL_FE) k_rc_cells_at(const Fr *u, const RecoverBlob *blobs, const CqPair *pairs, const CellComputeConsts *cc,
                                                         uint8_t *out) {
    __shared__ Fr a[CELL_FE];
    const CqPair pr = pairs[blockIdx.x];
    const int r = threadIdx.x;
    if (blobs[pr.blob].set < 0) return;
    Fr v = u[((size_t)pr.blob * CELLS_PER_EXT_BLOB + pr.cell) * CELL_FE + r];
    const uint32_t e = rev<7>(pr.cell) * (uint32_t)r;              // h_k^r = w^e, e <= 127 * 63
    if (e) { const Fr hp = cell_wpow(cc, e); fr_mul(v, v, hp); }
    a[r] = v;
    __syncthreads();
    fr_dif<CELL_FE, CELL_FE>(a, cc, r);
    fr_to_be32(out + (size_t)CELL_BYTES * pr.slot + 32 * r, a[r]);
}

void launch_rc_cells_at(const Fr *d_u, const RecoverBlob *d_blobs, const CqPair *d_pairs, int pairs, const CellComputeConsts *d_cc, uint8_t *d_out,
                        hipStream_t st) {
    if (pairs > 0) hipLaunchKernelGGL(k_rc_cells_at, dim3(pairs), dim3(CELL_FE), 0, st, d_u, d_blobs, d_pairs, d_cc, d_out);
}

}  // namespace kzg
