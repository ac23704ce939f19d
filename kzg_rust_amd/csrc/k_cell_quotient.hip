// k_cell_quotient.hip -- compute_cell_kzg_proofs_at on the device: the proofs of chosen cells of a blob, each as the commitment to its own
// quotient.  The FK20 chain of k_cell_compute.hip costs the same whatever is wanted of its 128 proofs; here a pair
// (blob, cell k) costs one field kernel and one fixed-base MSM over the handle's Lagrange points.
//
// Blob polynomial p = sum_m f_m X^m (m < 4096), a_k = w128^rev7(k).  The proof of cell k is [q_k(tau)]_1 with q_k = (p - I_k) / (X^64 - a_k),
// I_k of degree < 64: q_k has 4032 coefficients and, column by column (r < 64), obeys q[64u + r] = f[64(u+1) + r] + a_k q[64(u+1) + r] for
// u = 62 .. 0, starting from q[64 * 63 + r] = 0.  One forward transform of size 4096 (dif: natural order in, bit-reversed order out) leaves
// q_k(w4096^rev12(i)) at position i, which is the order of a blob and of the Lagrange points, so the MSM that commits to blobs commits to it.
// tests/cell_proofs_at_spec.py restates this route over Python integers.
#define KZG_FP_MUL_NOINLINE 1
#include "kernels.h"
#include "cell_domain.h"

namespace kzg {

constexpr int CQ_THREADS = 512;
// workgroup = pair: coefficients of the pair's blob (as k_cc_field leaves them) -> the 4096 evaluation-form scalars of its quotient, Montgomery,
// in the pair's row of `scal`.  A pair of a blob whose error word is set (k_cc_field has run: its coefficients come from elements >= r) takes the
// zero polynomial instead, so that the MSM behind it recodes reduced scalars whatever the blob held; nobody reads that row's result.
__global__ void __launch_bounds__(CQ_THREADS) k_cq_quotient(const Fr *coef, const CqPair *pairs, const int *err, const CellComputeConsts *cc, Fr *scal) {
    __shared__ Fr a[N_FE];
    const int tid = threadIdx.x;
    const CqPair pr = pairs[blockIdx.x];
    const Fr *f = coef + (size_t)N_FE * pr.blob;
    if (tid < CELL_FE) {
        const Fr ak = cc->w4096[(N_FE / CC_FFT) * rev<7>(pr.cell)];
        const bool dead = err[pr.blob] != 0;
        Fr acc = fr_zero();
        a[CELL_FE * (CELL_FE - 1) + tid] = acc;
#pragma unroll 1
        for (int u = CELL_FE - 2; u >= 0; u--) {
            fr_mul(acc, acc, ak);
            if (!dead) fr_add(acc, acc, f[CELL_FE * (u + 1) + tid]);
            a[CELL_FE * u + tid] = acc;
        }
    }
    __syncthreads();
    fr_dif<N_FE, CQ_THREADS>(a, cc, tid);
    Fr *out = scal + (size_t)N_FE * blockIdx.x;
    for (int i = tid; i < N_FE; i += CQ_THREADS) out[i] = a[i];
}

// workgroup = pair: cell pr.cell of blob pr.blob of the chunk's cell buffer -> slot pr.slot of `out`, 128 lanes of 16 bytes
__global__ void __launch_bounds__(CELL_BYTES / 16) k_cq_gather(const uint8_t *cells, const CqPair *pairs, uint8_t *out) {
    const CqPair pr = pairs[blockIdx.x];
    const uint4 *src = reinterpret_cast<const uint4 *>(cells + ((size_t)CELLS_PER_EXT_BLOB * pr.blob + pr.cell) * CELL_BYTES);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)CELL_BYTES * pr.slot);
    dst[threadIdx.x] = src[threadIdx.x];
}

void launch_cq_quotient(const Fr *d_coef, const CqPair *d_pairs, int pairs, const int *d_err, const CellComputeConsts *d_cc, Fr *d_scal, hipStream_t st) {
    if (pairs > 0) hipLaunchKernelGGL(k_cq_quotient, dim3(pairs), dim3(CQ_THREADS), 0, st, d_coef, d_pairs, d_err, d_cc, d_scal);
}
void launch_cq_gather(const uint8_t *d_cells, const CqPair *d_pairs, int pairs, uint8_t *d_out, hipStream_t st) {
    if (pairs > 0) hipLaunchKernelGGL(k_cq_gather, dim3(pairs), dim3(CELL_BYTES / 16), 0, st, d_cells, d_pairs, d_out);
}

}  // namespace kzg
