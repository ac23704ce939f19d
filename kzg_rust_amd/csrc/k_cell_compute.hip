// k_cell_compute.hip -- compute_cells_and_kzg_proofs (EIP-7594 / PeerDAS, consensus specs fulu/polynomial-commitments-sampling.md) on the
// device: the 128 cells of a blob's 2x extension and their 128 proofs by FK20 (Feist-Khovratovich, "Fast amortized KZG proofs").
//
// Blob polynomial p = sum_m f_m X^m (m < 4096); a_k = h_k^64 = w128^rev7(k), w128 = w^64, w = 7^((r-1)/8192).  The proof of cell k is the
// quotient of p by X^64 - a_k at tau, pi_k = sum_{e<63} a_k^e H_e with H_e = sum_{m >= 64(e+1)} f_m [tau^(m - 64(e+1))]_1.  With
// g_r[u] = f_(64u+r), x_r[v] = [tau^(64v+r)]_1 and c_r[d] = g_r[63-d] / 128 (d < 64; 0 above), H_(62-n) = sum_r (c_r (*) x_r)[n] for n < 63,
// (*) the 128-point cyclic convolution.  So, per blob:
//   field stage  (k_cc_field)   canonical check, inverse NTT 4096 -> f, coset NTT 4096 of f_m w^m -> cells 64..127;
//                (k_cc_columns) C_r = NTT128(c_r) for the 64 columns r;
//   fixed-base   (k_cc_msm)     Z[i] = sum_r C_r[i] X_r[i], X_r = NTT128(x_r) built once per handle (k_cc_table: signed 4-bit comb table);
//   G1 FFT       (k_cc_proofs)  conv = iNTT128(Z); h_e = conv[62-e] (e < 63), 0 above; pi = NTT128(h); compressed.  conv[63] = sum_r sum_d
//                               c_r[d] x_r[63-d] = sum_m f_m [tau^m]_1 is the blob's commitment (no index wraps), written out when asked for.
// Every transform of size 2^k is radix 2 in one of two orders: "dif" takes natural order and leaves the outputs bit-reversed, "dit" takes
// bit-reversed order and leaves them natural.  Forward transforms are dif, inverse ones dit, so no permutation runs anywhere: the blob is
// already in bit-reversed order, cells 64..127 are the coset evaluations in 12-bit bit-reversed order, Z is bit-reversed on both factors, and
// the proofs come out of the last dif in cell order.  tests/fk20_spec.py restates this route over Fr.
#define KZG_FP_MUL_NOINLINE 1
#include "kernels.h"
#include "cell_domain.h"

namespace kzg {

// ---- setup: constants
// thread e < 4096: w4096^e from the handle's bit-reversed root table; threads e < 128 also the GLV halves of w128^e; thread 0 the scalars
__global__ void __launch_bounds__(256) k_cc_consts(const Fr *roots, CellComputeConsts *cc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N_FE) return;
    const Fr v = roots[rev<12>((uint32_t)e)];                      // roots[brp12(i)] = w4096^i
    cc->w4096[e] = v;
    if (e % (N_FE / CC_FFT) == 0) {
        uint32_t k[8]; fr_to_words(k, v);
        const int t = e / (N_FE / CC_FFT);
        glv_split_fast(cc->tw_a[t], cc->tw_b[t], k);
    }
    if (e == 0) {
        const uint32_t wc[8] = FR_W8192_INIT;
        fr_from_words(cc->w8192, wc);
        Fr n = fr_zero(); const Fr one = fr_one();
        for (int i = 0; i < CC_FFT; i++) fr_add(n, n, one);
        fr_inv_fermat(cc->inv128, n);
        Fr n4096 = n;
        for (int i = 0; i < 5; i++) fr_add(n4096, n4096, n4096);
        fr_inv_fermat(cc->inv4096, n4096);
    }
}
// scalars w_i^t (t = t0 .. t0 + CELL_FE - 1) of the "blobs" whose commitments are the monomial points [tau^t]_1
__global__ void __launch_bounds__(256) k_cc_mono_scalars(const Fr *roots, int t0, Fr *out) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= CELL_FE * N_FE) return;
    const uint32_t e = (uint32_t)(t0 + gid / N_FE);
    Fr acc = fr_one(), b = roots[gid % N_FE];
    for (int bit = 11; bit >= 0; bit--) { fr_sqr(acc, acc); if ((e >> bit) & 1u) fr_mul(acc, acc, b); }
    out[gid] = acc;
}
__global__ void __launch_bounds__(64) k_cc_decode(const uint8_t *in48, int n, G1Affine *out, int *err) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint8_t b[48];
    for (int k = 0; k < 48; k++) b[k] = in48[48 * (size_t)t + k];
    G1Affine p;
    if (g1_decompress(p, b) != 0) { atomicOr(err, ERR_SETUP_POINT); p = g1a_inf(); }
    out[t] = p;
}

// ---- G1 transforms of 128 points: one wave, lane L one butterfly per stage, the points in LDS
// [w128^e] P through the precomputed GLV halves: [a] P + [b] (-phi P), joint double-and-add on Jacobian points (complete additions:
// P or the result may be the point at infinity)
__device__ void cc_mul_tw(G1Jac &r, const G1Jac &p, const CellComputeConsts *cc, int e) {
    const uint32_t *a = cc->tw_a[e], *b = cc->tw_b[e];
    const uint32_t bc[NFP] = FP_BETA_INIT;
    Fp beta; for (int i = 0; i < NFP; i++) beta.l[i] = bc[i];
    G1Jac q; fp_mul(q.x, p.x, beta); fp_neg(q.y, p.y); q.z = p.z;            // -phi(P) = (beta X, -Y, Z)
    G1Jac pq; g1_add(pq, p, q);
    G1Jac acc = g1_inf();
#pragma unroll 1
    for (int i = 127; i >= 0; i--) {
        g1_dbl(acc, acc);
        const int sel = (int)((a[i >> 5] >> (i & 31)) & 1u) | (int)(((b[i >> 5] >> (i & 31)) & 1u) << 1);
        if (sel) { const G1Jac &t = sel == 1 ? p : sel == 2 ? q : pq; g1_add(acc, acc, t); }
    }
    r = acc;
}
__device__ __forceinline__ void cc_sub(G1Jac &r, const G1Jac &u, const G1Jac &v) { G1Jac nv; g1_neg(nv, v); g1_add(r, u, nv); }
// forward (root w128), natural in, bit-reversed out
__device__ void cc_g1_dif(G1Jac *a, const CellComputeConsts *cc, int L) {
    for (int h = CC_FFT / 2; h >= 1; h >>= 1) {
        const int j = L % h, s = (L / h) * 2 * h, e = j * (CC_FFT / 2 / h);
        const G1Jac u = a[s + j], v = a[s + j + h];
        G1Jac x, y;
        g1_add(x, u, v);
        cc_sub(y, u, v);
        if (e) cc_mul_tw(y, y, cc, e);
        __syncthreads();
        a[s + j] = x; a[s + j + h] = y;
        __syncthreads();
    }
}
// inverse (root w128^-1, no 1/128: the field stage scales the columns), bit-reversed in, natural out
__device__ void cc_g1_dit_inv(G1Jac *a, const CellComputeConsts *cc, int L) {
    for (int h = 1; h < CC_FFT; h <<= 1) {
        const int j = L % h, s = (L / h) * 2 * h, e = j * (CC_FFT / 2 / h);
        const G1Jac u = a[s + j];
        G1Jac v = a[s + j + h];
        if (e) cc_mul_tw(v, v, cc, CC_FFT - e);
        G1Jac x, y;
        g1_add(x, u, v);
        cc_sub(y, u, v);
        __syncthreads();
        a[s + j] = x; a[s + j + h] = y;
        __syncthreads();
    }
}
// setup: block r transforms x_r = ([tau^(64v+r)]_1 for v < 64, then 64 points at infinity) -> X[r][i] (bit-reversed order)
__global__ void __launch_bounds__(64) k_cc_setup_fft(const G1Affine *mono, const CellComputeConsts *cc, G1Jac *X) {
    __shared__ G1Jac a[CC_FFT];
    const int r = blockIdx.x, L = threadIdx.x;
    g1_from_affine(a[L], mono[CELL_FE * L + r]);
    a[L + CC_FFT / 2] = g1_inf();
    __syncthreads();
    cc_g1_dif(a, cc, L);
    X[(size_t)r * CC_FFT + L] = a[L];
    X[(size_t)r * CC_FFT + L + CC_FFT / 2] = a[L + CC_FFT / 2];
}
// setup: thread (point P, window w): m [16^w] X_P for m = 1..8, affine, at tab[(P * 64 + w) * 8 + m - 1]
__global__ void __launch_bounds__(64) k_cc_table(const G1Jac *X, G1Affine *tab) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)CC_POINTS * CC_WINDOWS) return;
    const int P = (int)(gid / CC_WINDOWS), w = (int)(gid % CC_WINDOWS);
    G1Jac base = X[P];
#pragma unroll 1
    for (int i = 0; i < 4 * w; i++) g1_dbl(base, base);
    G1Jac m = base;
    G1Affine *o = tab + gid * CC_DIGITS;
#pragma unroll 1
    for (int k = 0; k < CC_DIGITS; k++) {
        if (k) g1_add(m, m, base);
        G1Affine p; g1_to_affine(p, m);
        o[k] = p;
    }
}

// ---- per call: field stage.  One workgroup per blob, the 4096 values in LDS (147,456 bytes).
constexpr int CC_FIELD_THREADS = 512;
__global__ void __launch_bounds__(CC_FIELD_THREADS) k_cc_field(const uint8_t *blobs, const CellComputeConsts *cc, Fr *coef /* [n][4096] or null */,
                                                              uint8_t *cells /* [n][128][2048] or null */, int *err) {
    __shared__ Fr a[N_FE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t *blob = blobs + (size_t)BLOB_BYTES * b;
    bool bad = false;
    for (int i = tid; i < N_FE; i += CC_FIELD_THREADS) {
        Fr v;
        bad |= !fr_from_be32_checked(v, blob + 32 * i);
        a[i] = v;                                                     // p(w4096^rev12(i)): bit-reversed order, as dit wants it
    }
    if (bad) atomicOr(&err[b], ERR_NONCANONICAL_FR);
    __syncthreads();
    // inverse NTT (dit, root w4096^-1): natural-order coefficients times 4096
    fr_dit_inv<N_FE, CC_FIELD_THREADS>(a, cc, tid);
    for (int m = tid; m < N_FE; m += CC_FIELD_THREADS) {
        Fr f; fr_mul(f, a[m], cc->inv4096);
        if (coef) coef[(size_t)N_FE * b + m] = f;
        if (cells) { Fr t; fr_mul(t, f, cell_wpow(cc, (uint32_t)m)); a[m] = t; }    // f_m w^m
    }
    if (!cells) return;
    __syncthreads();
    // coset NTT (dif, root w4096): position i holds p(w w4096^rev12(i)), i.e. element i of cells 64..127 read as one array
    fr_dif<N_FE, CC_FIELD_THREADS>(a, cc, tid);
    uint8_t *out = cells + (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES * b;
    const uint4 *src = reinterpret_cast<const uint4 *>(blob);         // cells 0..63: the blob itself
    uint4 *dst = reinterpret_cast<uint4 *>(out);
    for (int i = tid; i < BLOB_BYTES / 16; i += CC_FIELD_THREADS) dst[i] = src[i];
    for (int i = tid; i < N_FE; i += CC_FIELD_THREADS) fr_to_be32(out + BLOB_BYTES + 32 * i, a[i]);
}
// workgroup (blob, column r): C_r = dif128(c_r), c_r[d] = f_(64(63-d)+r) / 128 for d < 64, 0 above; scal[blob][i][r] = C_r[i] as 8 words
__global__ void __launch_bounds__(64) k_cc_columns(const Fr *coef, const CellComputeConsts *cc, uint32_t *scal) {
    __shared__ Fr a[CC_FFT];
    const int b = blockIdx.x / CELL_FE, r = blockIdx.x % CELL_FE, L = threadIdx.x;
    Fr v; fr_mul(v, coef[(size_t)N_FE * b + CELL_FE * (CELL_FE - 1 - L) + r], cc->inv128);
    a[L] = v;
    a[L + CC_FFT / 2] = fr_zero();
    __syncthreads();
    fr_dif<CC_FFT, CC_FFT / 2>(a, cc, L);
    for (int i = L; i < CC_FFT; i += CC_FFT / 2) fr_store_words(scal + 8 * (((size_t)b * CC_FFT + i) * CELL_FE + r), a[i]);
}
// workgroup (blob, i), lane r: [C_r[i]] X_r[i] from the comb table (64 signed 4-bit digits in [-8, 7], one mixed addition each), then the
// 64 lanes' sum -> Z[blob][i]
__global__ void __launch_bounds__(64) k_cc_msm(const uint32_t *scal, const G1Affine *tab, G1Jac *Z) {
    __shared__ G1Jac red[CELL_FE];
    const int bi = blockIdx.x, i = bi % CC_FFT, r = threadIdx.x;
    const uint32_t *k = scal + 8 * ((size_t)bi * CELL_FE + r);
    uint32_t e[8];
    uint64_t c = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) { c += (uint64_t)k[q] + 0x88888888u; e[q] = (uint32_t)c; c >>= 32; }   // k < r: no carry leaves the top word
    const G1Affine *pt = tab + (size_t)(r * CC_FFT + i) * CC_WINDOWS * CC_DIGITS;
    G1X acc = g1x_inf();
    bool started = false;
#pragma unroll 1
    for (int w = 0; w < CC_WINDOWS; w++) {
        const int d = (int)((e[w >> 3] >> (4 * (w & 7))) & 15u) - 8;
        if (!d) continue;
        G1Affine p = pt[w * CC_DIGITS + (d < 0 ? -d : d) - 1];
        if (d < 0) g1a_neg(p, p);
        g1x_add_mixed_lazy(acc, started, p);
    }
    G1X x; g1x_from_lazy(x, acc, started);
    G1Jac j; g1x_to_jac(j, x);
    red[r] = j;
    __syncthreads();
    for (int s = CELL_FE / 2; s > 0; s >>= 1) {
        if (r < s) { G1Jac u = red[r], v = red[r + s]; g1_add(u, u, v); red[r] = u; }
        __syncthreads();
    }
    if (r == 0) Z[bi] = red[0];
}
// workgroup blob: conv = dit_inv(Z); h_e = conv[62 - e] (e < 63), infinity above; pi = dif(h), compressed in cell order.  h_dbg (or null):
// H_0 .. H_63 compressed (H_63 = infinity).  commit48 (or null): conv[63] = sum_m f_m [tau^m]_1, the blob's commitment, compressed; the lane
// that holds no h takes it.  With neither proofs48 nor h_dbg the kernel ends there (the whole workgroup: no barrier follows a divergent return).
__global__ void __launch_bounds__(64) k_cc_proofs(const G1Jac *Z, const CellComputeConsts *cc, uint8_t *proofs48, uint8_t *h_dbg, uint8_t *commit48) {
    __shared__ G1Jac a[CC_FFT];
    const int b = blockIdx.x, L = threadIdx.x;
    a[L] = Z[(size_t)b * CC_FFT + L];
    a[L + CC_FFT / 2] = Z[(size_t)b * CC_FFT + L + CC_FFT / 2];
    __syncthreads();
    cc_g1_dit_inv(a, cc, L);
    const G1Jac h = L < CELL_FE - 1 ? a[CELL_FE - 2 - L] : g1_inf();
    if (commit48 && L == CELL_FE - 1) {
        G1Affine p; g1_to_affine(p, a[CELL_FE - 1]);
        g1_compress_affine(commit48 + 48 * (size_t)b, p);
    }
    if (!proofs48 && !h_dbg) return;
    __syncthreads();
    a[L] = h;
    a[L + CC_FFT / 2] = g1_inf();
    __syncthreads();
    if (h_dbg) {
        G1Affine p; g1_to_affine(p, h);
        g1_compress_affine(h_dbg + 48 * ((size_t)b * CELL_FE + L), p);
    }
    cc_g1_dif(a, cc, L);
    for (int k = L; k < CC_FFT; k += CC_FFT / 2) {
        G1Affine p; g1_to_affine(p, a[k]);
        g1_compress_affine(proofs48 + 48 * ((size_t)b * CC_FFT + k), p);
    }
}

// ---- launchers
void launch_cc_consts(const Fr *d_roots, CellComputeConsts *d_cc, hipStream_t st) {
    hipLaunchKernelGGL(k_cc_consts, dim3(N_FE / 256), dim3(256), 0, st, d_roots, d_cc);
}
void launch_monomial_chunk(DeviceTables t, int t0, Fr *d_scal, uint8_t *d_digits, G1Jac *d_partials, uint8_t *d_out48, hipStream_t st) {
    hipLaunchKernelGGL(k_cc_mono_scalars, dim3(CELL_FE * N_FE / 256), dim3(256), 0, st, t.roots, t0, d_scal);
    launch_digits_from_fr(d_scal, CELL_FE, d_digits, st);
    launch_msm_bucket(d_digits, t, CELL_FE, d_partials, st);
    launch_msm_finalize(d_partials, CELL_FE, d_out48 + 48 * (size_t)t0, st);
}
void launch_monomial_decode(const uint8_t *d_mono48, int count, G1Affine *d_mono, int *d_err, hipStream_t st) {
    hipLaunchKernelGGL(k_cc_decode, dim3((count + 63) / 64), dim3(64), 0, st, d_mono48, count, d_mono, d_err);
}
void launch_cc_setup_points(const G1Affine *d_mono, const CellComputeConsts *d_cc, G1Jac *d_X, G1Affine *d_tab, hipStream_t st) {
    hipLaunchKernelGGL(k_cc_setup_fft, dim3(CELL_FE), dim3(64), 0, st, d_mono, d_cc, d_X);
    hipLaunchKernelGGL(k_cc_table, dim3(CC_POINTS * CC_WINDOWS / 64), dim3(64), 0, st, d_X, d_tab);
}
void launch_cc_field(const uint8_t *d_blobs, int n, const CellComputeConsts *d_cc, Fr *d_coef, uint8_t *d_cells, int *d_err, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_cc_field, dim3(n), dim3(CC_FIELD_THREADS), 0, st, d_blobs, d_cc, d_coef, d_cells, d_err);
}
void launch_cc_columns(const Fr *d_coef, int n, const CellComputeConsts *d_cc, uint32_t *d_scal, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_cc_columns, dim3(n * CELL_FE), dim3(64), 0, st, d_coef, d_cc, d_scal);
}
void launch_cc_msm(const uint32_t *d_scal, int n, const G1Affine *d_tab, G1Jac *d_Z, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_cc_msm, dim3(n * CC_FFT), dim3(64), 0, st, d_scal, d_tab, d_Z);
}
void launch_cc_proofs(const G1Jac *d_Z, int n, const CellComputeConsts *d_cc, uint8_t *d_proofs48, uint8_t *d_h_dbg, uint8_t *d_commit48, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_cc_proofs, dim3(n), dim3(64), 0, st, d_Z, d_cc, d_proofs48, d_h_dbg, d_commit48);
}

}  // namespace kzg
