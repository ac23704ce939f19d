// k_cell_recover.hip -- the field stage of recover_cells_and_kzg_proofs (EIP-7594 / PeerDAS, consensus specs
// fulu/polynomial-commitments-sampling.md) on the device: from 64..128 known cells of a blob's 2x extension to the blob polynomial's
// coefficients and all 128 cells.  The proofs then come from the FK20 chain of k_cell_compute.hip (k_cc_columns, k_cc_msm, k_cc_proofs).
//
// The spec states recovery with 8192-point transforms; the cell structure makes every transform here one of 64 or 128 points.  Write
// p(x) = sum_{r<64} x^r P_r(x^64), deg P_r < 64.  The 64 points of cell k share x^64 = a_k = w128^rev7(k) (w128 = w^64, w = 7^((r-1)/8192)),
// so the degree < 64 interpolant of cell k on its coset h_k <w64> has the coefficients u_r(k) = P_r(a_k): 64 independent erasure-decoding
// problems of length 128, one per column r, all with the same known positions.  (Blobs of one call may be known at different index sets: each
// reads the tables of its own set through its descriptor, RecoverBlob.)  With M the missing cells and S(y) = prod_{m in M} (y - a_m):
//   (k_rc_interp)  per known cell: dit64 of its elements (root w64^-1), coefficient t times h_k^-t  -> u_t(k)
//   (k_rc_vanish)  once per index set: S(a_k) on the domain and 1 / S(g a_k) on the coset g <w128>, g = w (g^128 = w64 != 1)
//   (k_rc_columns) per (blob, column r): E_r(a_k) S(a_k) (0 at the missing k) = (P_r S)(a_k), deg P_r S < 128: dit128 -> its coefficients c_i;
//                  dif128 of c_i g^i -> (P_r S)(g a_k); times 1 / S(g a_k); dit128, times g^-i -> P_r.  f_(64u+r) = P_r[u] for u < 64 are the
//                  blob's coefficients (columns are what k_cc_columns reads); dif128 of (P_r[0..63], 0^64) -> P_r(a_k) for all 128 cells
//   (k_rc_cells)   per cell: coefficient r times h_k^r, dif64 (root w64) -> the cell's 64 elements in their order
// Orders as in k_cell_compute.hip: "dif" natural in, bit-reversed out; "dit" bit-reversed in, natural out.  Cell order is the bit-reversed
// order of the 128-point domain and element order that of the 64-point coset, so no permutation runs anywhere.  The factors 1/64 (dit64) and
// 1/128 (each dit128) ride in the two tables of k_rc_vanish.  Coefficients 64..127 of P_r are zero exactly when the known cells lie on one
// polynomial of degree < 4096; they are dropped, as the spec drops the upper half of its quotient.  tests/recover_spec.py restates the route.
#define KZG_FP_MUL_NOINLINE 1
#include "kernels.h"
#include "cell_domain.h"

namespace kzg {

// workgroup per index set of the chunk, thread k < 128: pos[k] from the set's mask (< 0 marks the missing cells), sd[k] = S(a_k) / (64 * 128),
// sci[k] = 1 / (128 S(g a_k))
__global__ void __launch_bounds__(CELLS_PER_EXT_BLOB) k_rc_vanish(const CellComputeConsts *cc, const uint64_t *masks, RecoverTables *rts) {
    __shared__ Fr a[CELLS_PER_EXT_BLOB];
    __shared__ int missing[CELLS_PER_EXT_BLOB];
    const int k = threadIdx.x;
    RecoverTables *rt = rts + blockIdx.x;
    const uint64_t lo = masks[2 * blockIdx.x], hi = masks[2 * blockIdx.x + 1];
    const uint64_t half = k < 64 ? lo : hi, bit = (uint64_t)1 << (k & 63);
    const int known = (half & bit) != 0;
    rt->pos[k] = known ? __popcll(half & (bit - 1)) + (k < 64 ? 0 : __popcll(lo)) : -1;
    a[k] = cc->w4096[(N_FE / CC_FFT) * rev<7>((uint32_t)k)];
    missing[k] = !known;
    __syncthreads();
    Fr ga; fr_mul(ga, a[k], cc->w8192);
    Fr sd = fr_one(), sc = fr_one();
    for (int m = 0; m < CELLS_PER_EXT_BLOB; m++) {
        if (!missing[m]) continue;
        Fr d;
        fr_sub(d, a[k], a[m]); fr_mul(sd, sd, d);
        fr_sub(d, ga, a[m]); fr_mul(sc, sc, d);                    // never zero: g a_k is outside <w128>
    }
    Fr inv64; fr_add(inv64, cc->inv128, cc->inv128);
    fr_mul(sd, sd, inv64); fr_mul(sd, sd, cc->inv128);
    rt->sd[k] = sd;
    Fr sci; fr_inv(sci, sc);
    fr_mul(sci, sci, cc->inv128);
    rt->sci[k] = sci;
}
// workgroup (blob, cell k): the 64 coefficients of the cell's interpolant, times 64, at u[blob][k][t]; nothing for a missing cell or a refused blob.
// The blob's descriptor is the same for the whole workgroup: one scalar load.
__global__ void __launch_bounds__(CELL_FE) k_rc_interp(const uint8_t *cells, const RecoverBlob *blobs, const CellComputeConsts *cc, const RecoverTables *rts,
                                                       Fr *u, int *err) {
    __shared__ Fr a[CELL_FE];
    const int b = blockIdx.x / CELLS_PER_EXT_BLOB, k = blockIdx.x % CELLS_PER_EXT_BLOB, t = threadIdx.x;
    const RecoverBlob d = blobs[b];
    if (d.set < 0) return;
    const int p = rts[d.set].pos[k];
    if (p < 0) return;
    Fr v;
    if (!fr_from_be32_checked(v, cells + (d.first + (uint64_t)p) * CELL_BYTES + 32 * t)) atomicOr(&err[b], ERR_NONCANONICAL_FR);
    a[t] = v;                                                       // p(h_k w64^rev6(t)): bit-reversed order, as dit wants it
    __syncthreads();
    fr_dit_inv<CELL_FE, CELL_FE>(a, cc, t);
    const uint32_t e = (rev<7>((uint32_t)k) * (uint32_t)t) & 8191u;   // h_k^-t = w^(8192 - e)
    v = a[t];
    if (e) { const Fr hp = cell_wpow(cc, 8192u - e); fr_mul(v, v, hp); }
    u[((size_t)b * CELLS_PER_EXT_BLOB + k) * CELL_FE + t] = v;
}
// workgroup (blob, column r): see the head of the file.  u is read at [blob][k][r] for the known k and, when cells are wanted, written there
// for all k; coef (or null) receives f_(64 i + r) for i < 64.  A refused blob gets zero coefficients (what the FK20 chain behind reads must be
// field elements) and nothing else.
__global__ void __launch_bounds__(CELL_FE) k_rc_columns(Fr *u, const RecoverBlob *blobs, const CellComputeConsts *cc, const RecoverTables *rts, Fr *coef,
                                                        int want_cells) {
    __shared__ Fr a[CC_FFT];
    const int b = blockIdx.x / CELL_FE, r = blockIdx.x % CELL_FE, L = threadIdx.x;
    const int set = blobs[b].set;
    if (set < 0) {
        if (coef) coef[(size_t)N_FE * b + CELL_FE * L + r] = fr_zero();
        return;
    }
    const RecoverTables *rt = rts + set;
    Fr *col = u + (size_t)b * CELLS_PER_EXT_BLOB * CELL_FE + r;
    for (int k = L; k < CC_FFT; k += CC_FFT / 2) {
        Fr v = fr_zero();
        if (rt->pos[k] >= 0) fr_mul(v, col[(size_t)k * CELL_FE], rt->sd[k]);
        a[k] = v;
    }
    __syncthreads();
    fr_dit_inv<CC_FFT, CC_FFT / 2>(a, cc, L);                                   // coefficients of P_r S
    for (int i = L; i < CC_FFT; i += CC_FFT / 2)
        if (i) { Fr v; const Fr g = cell_wpow(cc, (uint32_t)i); fr_mul(v, a[i], g); a[i] = v; }
    __syncthreads();
    fr_dif<CC_FFT, CC_FFT / 2>(a, cc, L);                                       // (P_r S)(g a_k)
    for (int k = L; k < CC_FFT; k += CC_FFT / 2) { Fr v; fr_mul(v, a[k], rt->sci[k]); a[k] = v; }
    __syncthreads();
    fr_dit_inv<CC_FFT, CC_FFT / 2>(a, cc, L);                                   // P_r[i] g^i
    Fr f = a[L];
    if (L) { const Fr g = cell_wpow(cc, 8192u - (uint32_t)L); fr_mul(f, f, g); }
    if (coef) coef[(size_t)N_FE * b + CELL_FE * L + r] = f;
    if (!want_cells) return;
    __syncthreads();
    a[L] = f;
    a[L + CC_FFT / 2] = fr_zero();
    __syncthreads();
    fr_dif<CC_FFT, CC_FFT / 2>(a, cc, L);                                       // P_r(a_k), k in cell order
    for (int k = L; k < CC_FFT; k += CC_FFT / 2) col[(size_t)k * CELL_FE] = a[k];
}
// workgroup (blob, cell k): the cell's elements from u[blob][k][r] = P_r(a_k); nothing for a refused blob
__global__ void __launch_bounds__(CELL_FE) k_rc_cells(const Fr *u, const RecoverBlob *blobs, const CellComputeConsts *cc, uint8_t *cells) {
    __shared__ Fr a[CELL_FE];
    const int k = blockIdx.x % CELLS_PER_EXT_BLOB, r = threadIdx.x;
    if (blobs[blockIdx.x / CELLS_PER_EXT_BLOB].set < 0) return;
    Fr v = u[(size_t)blockIdx.x * CELL_FE + r];
    const uint32_t e = rev<7>((uint32_t)k) * (uint32_t)r;          // h_k^r = w^e, e <= 127 * 63
    if (e) { const Fr hp = cell_wpow(cc, e); fr_mul(v, v, hp); }
    a[r] = v;
    __syncthreads();
    fr_dif<CELL_FE, CELL_FE>(a, cc, r);
    fr_to_be32(cells + (size_t)blockIdx.x * CELL_BYTES + 32 * r, a[r]);
}

// ---- launchers
void launch_rc_vanish(const CellComputeConsts *d_cc, const uint64_t *d_masks, int sets, RecoverTables *d_rt, hipStream_t st) {
    if (sets > 0) hipLaunchKernelGGL(k_rc_vanish, dim3(sets), dim3(CELLS_PER_EXT_BLOB), 0, st, d_cc, d_masks, d_rt);
}
void launch_rc_interp(const uint8_t *d_cells, const RecoverBlob *d_blobs, int m, const CellComputeConsts *d_cc, const RecoverTables *d_rt, Fr *d_u,
                      int *d_err, hipStream_t st) {
    if (m > 0) hipLaunchKernelGGL(k_rc_interp, dim3(m * CELLS_PER_EXT_BLOB), dim3(CELL_FE), 0, st, d_cells, d_blobs, d_cc, d_rt, d_u, d_err);
}
void launch_rc_columns(Fr *d_u, const RecoverBlob *d_blobs, int m, const CellComputeConsts *d_cc, const RecoverTables *d_rt, Fr *d_coef,
                       bool want_cells, hipStream_t st) {
    if (m > 0) hipLaunchKernelGGL(k_rc_columns, dim3(m * CELL_FE), dim3(CELL_FE), 0, st, d_u, d_blobs, d_cc, d_rt, d_coef, want_cells ? 1 : 0);
}
void launch_rc_cells(const Fr *d_u, const RecoverBlob *d_blobs, int m, const CellComputeConsts *d_cc, uint8_t *d_cells, hipStream_t st) {
    if (m > 0) hipLaunchKernelGGL(k_rc_cells, dim3(m * CELLS_PER_EXT_BLOB), dim3(CELL_FE), 0, st, d_u, d_blobs, d_cc, d_cells);
}

}  // namespace kzg
