// k_point_quotient.hip -- compute_kzg_proofs_at on the device: openings of a blob at chosen points, each proof as the commitment to its own
// quotient.  A pair (blob, z) costs one field kernel and one fixed-base MSM over the handle's Lagrange points, whatever
// z is: no inversion, and a z inside the domain takes the same route as any other.
//
// Blob polynomial p = sum_m f_m X^m (m < 4096).  The quotient q = (p - p(z)) / (X - z) has 4095 coefficients and obeys q[j] = f[j+1] + z q[j+1]
// from q[4095] = 0 downwards, and y = p(z) = f[0] + z q[0]: with Q[j] = sum_(m >= j) f[m] z^(m-j), q[j] = Q[j+1] and y = Q[0].  The chain of
// 4096 steps is cut into 512 segments of 8: thread t takes Q of its own coefficients alone (segment value S_t = sum_(i < 8) f[8t+i] z^i), a
// suffix scan with the powers z^8, z^16, .. turns the S_t into Q[8t] in 9 doubling rounds, and a second pass of 8 steps starts from the carry
// Q[8(t+1)].  One forward transform of size 4096 (dif: natural order in, bit-reversed order out) leaves q(w4096^rev12(i)) at position i, which
// is the order of a blob and of the Lagrange points, so the MSM that commits to blobs commits to it.  tests/point_proofs_at_spec.py restates
// this route over Python integers.
#define KZG_FP_MUL_NOINLINE 1
#include "kernels.h"
#include "cell_domain.h"

namespace kzg {

constexpr int PQ_THREADS = 512, PQ_SEG = N_FE / PQ_THREADS;
// workgroup = pair: coefficients of the pair's blob (as k_cc_field leaves them) and the pair's point (Montgomery) -> y as 32 canonical bytes in
// slot pr.slot of `ys` (when wanted) and the 4096 evaluation-form scalars of the quotient, Montgomery, in the pair's row of `scal` (when
// wanted; without it neither the second pass nor the transform runs).  The scan's exchange lives in a[0 .. 1023], two rows that the rounds
// write in turn, before q is written over them: a[] alone takes 147,456 of the 163,840 bytes.  A pair of a blob whose error word is set
// (k_cc_field has run, or the host refused the blob) takes the zero polynomial instead, so that the MSM behind it recodes reduced scalars
// whatever the blob held; nobody reads that pair's results.
__global__ void __launch_bounds__(PQ_THREADS) k_pq_quotient(const Fr *coef, const PqPair *pairs, const Fr *zs, const int *err, const CellComputeConsts *cc,
                                                            Fr *scal, uint8_t *ys) {
    __shared__ Fr a[N_FE];
    const int tid = threadIdx.x;
    const PqPair pr = pairs[blockIdx.x];
    const Fr z = zs[blockIdx.x];
    const bool dead = err[pr.blob] != 0;
    const Fr *src = coef + (size_t)N_FE * pr.blob + PQ_SEG * tid;
    // first pass: zero carry-in (the coefficients are read again by the second pass rather than held: 72 registers a thread)
    Fr acc = fr_zero();
#pragma unroll 1
    for (int i = PQ_SEG - 1; i >= 0; i--) {
        fr_mul(acc, acc, z);
        if (!dead) fr_add(acc, acc, src[i]);
    }
    Fr zp = z;                                                        // z^(8 d) of round d
#pragma unroll
    for (int i = 1; i < PQ_SEG; i <<= 1) fr_sqr(zp, zp);
    Fr *cur = a, *nxt = a + PQ_THREADS;
    cur[tid] = acc;
    __syncthreads();
    // suffix scan: after round d, acc = sum of S_u z^(8(u-t)) over t <= u < t + 2d
#pragma unroll 1
    for (int d = 1; d < PQ_THREADS; d <<= 1) {
        if (tid + d < PQ_THREADS) {
            Fr t; fr_mul(t, cur[tid + d], zp);
            fr_add(acc, acc, t);
        }
        nxt[tid] = acc;
        __syncthreads();
        Fr *swap = cur; cur = nxt; nxt = swap;
        fr_sqr(zp, zp);
    }
    if (tid == 0 && ys) fr_to_be32(ys + 32 * pr.slot, acc);           // Q[0] = p(z)
    if (!scal) return;
    acc = tid + 1 < PQ_THREADS ? cur[tid + 1] : fr_zero();            // the carry Q[8(t+1)]
    __syncthreads();
    // second pass: Q[8t+i] = q[8t+i-1]
    if (tid == PQ_THREADS - 1) a[N_FE - 1] = fr_zero();
#pragma unroll 1
    for (int i = PQ_SEG - 1; i >= 0; i--) {
        fr_mul(acc, acc, z);
        if (!dead) fr_add(acc, acc, src[i]);
        if (PQ_SEG * tid + i > 0) a[PQ_SEG * tid + i - 1] = acc;
    }
    __syncthreads();
    fr_dif<N_FE, PQ_THREADS>(a, cc, tid);
    Fr *out = scal + (size_t)N_FE * blockIdx.x;
    for (int i = tid; i < N_FE; i += PQ_THREADS) out[i] = a[i];
}

void launch_pq_quotient(const Fr *d_coef, const PqPair *d_pairs, const Fr *d_zs, int pairs, const int *d_err, const CellComputeConsts *d_cc, Fr *d_scal,
                        uint8_t *d_ys, hipStream_t st) {
    if (pairs > 0) hipLaunchKernelGGL(k_pq_quotient, dim3(pairs), dim3(PQ_THREADS), 0, st, d_coef, d_pairs, d_zs, d_err, d_cc, d_scal, d_ys);
}

}  // namespace kzg
