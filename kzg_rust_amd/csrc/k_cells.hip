// k_cells.hip -- verify_cell_kzg_proof_batch (EIP-7594 / PeerDAS, consensus specs fulu/polynomial-commitments-sampling.md) on the device.
//
// A cell is 64 field elements of a blob's 2x Reed-Solomon extension (8192 points).  With w = 7^((r-1)/8192) and brp the 13-bit bit-reversal
// permutation of [w^0 .. w^8191], cell k holds the blob polynomial at brp[64k .. 64k+63]: element j sits at h_k * w64^rev6(j), where the coset
// shift is h_k = w^rev7(k) and w64 = w^128.  The batch check of n cells with weights r^0 .. r^(n-1) (r from a host-hashed transcript) is
//     e(LL, [tau^64]_2) == e(RL, G2),   LL = sum_k r^k pi_k,   RL = sum_i w_i C_i - [I(tau)]_1 + sum_k r^k h_k^64 pi_k,
// I = sum_k r^k I_k with I_k the degree < 64 interpolant of cell k on its coset, computed per column c (cell index): the weighted cells of the
// column are summed, the bit reversal undone, a 64-point inverse DFT taken and coefficient t multiplied by h_c^-t.
//
// Launch order of one call (cells.hip): decode + subgroup (k_g1.hip) | k_cell_rpowers -> k_cell_weights, k_cell_columns -> k_cell_interp ->
// k_cell_terms -> k_cell_sum -> k_cell_finish -> launch_pairing with the [tau^64]_2 line set.  The lincomb is one double-and-add scalar
// multiplication per term (255-bit scalars) and a tree per group and side: the 4844 lincomb families have their scalar layout baked in.
//
// A group cut over the devices of a multi-device handle (cells.hip: cell_multi_sharded): the check is linear in the cells once r is known, so a
// contiguous block of cells [k0, k0 + cnt) runs the same chain with weights r^(k0 + k) and stops after k_cell_sum; k_cell_merge adds the
// blocks' three sums on the group's stage-2 device and ends as k_cell_finish does.
// The G1 routines and the field products are inlined here (the out-of-line forms of g1.h / field.h take their operands by address, which puts
// every point a kernel holds into private memory): no kernel of this file uses scratch.
#define KZG_MID_INLINE 1
#include "kernels.h"
#include "cell_domain.h"
#include "group_geo.h"

namespace kzg {

__device__ __forceinline__ Fr fr_pow_small(const Fr &base, uint32_t e) {
    Fr acc = fr_one();
    for (int b = 31; b >= 0; b--) {
        fr_sqr(acc, acc);
        if ((e >> b) & 1u) fr_mul(acc, acc, base);
    }
    return acc;
}

// ---- setup (once per handle, on the first cell call)
// thread c < 128: h_c^64 and the shifts h_c^-t / 64; threads < 64 also the inverse-DFT twiddles w64^-j
__global__ void __launch_bounds__(128) k_cell_consts(CellConsts *cc) {
    const int c = threadIdx.x;
    const uint32_t wc[8] = FR_W8192_INIT;
    Fr w; fr_from_words(w, wc);
    const Fr h = fr_pow_small(w, rev<7>((uint32_t)c));
    Fr h64 = h;
    for (int i = 0; i < 6; i++) fr_sqr(h64, h64);
    cc->h64[c] = h64;
    Fr hinv, s, n64 = fr_zero();
    fr_inv_fermat(hinv, h);
    const Fr one = fr_one();
    for (int i = 0; i < 64; i++) fr_add(n64, n64, one);
    fr_inv_fermat(s, n64);
    for (int t = 0; t < CELL_FE; t++) { cc->shift[c][t] = s; fr_mul(s, s, hinv); }
    if (c < CELL_FE) {
        Fr w64 = w;
        for (int i = 0; i < 7; i++) fr_sqr(w64, w64);
        Fr w64inv; fr_inv_fermat(w64inv, w64);
        cc->tw[c] = fr_pow_small(w64inv, (uint32_t)c);
    }
}
// Miller-loop lines of setup g2[64] = [tau^64]_2 into slot 2 of a three-slot line table (the slot the pairing kernels pair the first point with)
__global__ void __launch_bounds__(64) k_cell_lines(const uint8_t *g2_bytes, LineCoeff *lines, int *lines_inf, int *err) {
    if (threadIdx.x != 0) return;
    uint8_t b[96];
    for (int k = 0; k < 96; k++) b[k] = g2_bytes[k];
    G2Affine q;
    if (g2_decompress(q, b) != 0) { atomicOr(err, ERR_SETUP_POINT); q.x = fp2_zero(); q.y = fp2_zero(); }
    const bool inf = g2a_is_inf(q);
    lines_inf[2] = inf ? 1 : 0;
    if (!inf) precompute_lines(lines + 2 * N_LINES, q);
}

// ---- per call
// Every kernel that needs to know where a group lies has ONE body, written against the geometry of group_geo.h, and two entries: the uniform
// one (every group npg cells; its name and arguments as they always were) and the `_sets` one (every group its own count).  k_cell_columns,
// k_cell_finish and k_cell_merge work on global cell numbers and per-group slots and have one form.
// thread (g, k): r of group g from its digest, r^(k0 + k), and the two proof scalars: r^(k0 + k) (LL) and r^(k0 + k) h_k^64 (RL).  k0: the
// position in its group of the first cell handed to this launch (0 unless the group is cut into blocks)
template <class GEO>
__device__ __forceinline__ void cell_rpowers_body(const GEO geo, const uint8_t *digests, const int *cell_idx, int n_cells, int k0, const CellConsts *cc,
                                                  Fr *rpow, uint32_t *scal, uint8_t *r_out) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_cells) return;
    const int g = geo.group_of_cell(gid), k = geo.cell_in_group(gid, g), n = geo.count(g);
    const size_t t0 = geo.term0(g);
    uint32_t w[8]; be32_to_words(w, digests + 32 * (size_t)g);
    Fr r; fr_from_words(r, w);                                    // int(digest) mod r_BLS
    if (k == 0) fr_to_be32(r_out + 32 * (size_t)g, r);
    const Fr p = fr_pow_small(r, (uint32_t)k0 + (uint32_t)k);
    rpow[gid] = p;
    Fr q; fr_mul(q, p, cc->h64[cell_idx[gid]]);
    fr_store_words(scal + 8 * (t0 + n + k), q);
    fr_store_words(scal + 8 * (t0 + 2 * n + CELL_FE + k), p);
}
__global__ void __launch_bounds__(256) k_cell_rpowers(const uint8_t *digests, const int *cell_idx, int npg, int groups, int k0, const CellConsts *cc,
                                                      Fr *rpow, uint32_t *scal, uint8_t *r_out) {
    cell_rpowers_body(GroupGeoUniform{npg}, digests, cell_idx, npg * groups, k0, cc, rpow, scal, r_out);
}
__global__ void __launch_bounds__(256) k_cell_rpowers_sets(const uint8_t *digests, const int *cell_idx, const int *goff, const int *cgrp, int n_cells,
                                                           const CellConsts *cc, Fr *rpow, uint32_t *scal, uint8_t *r_out) {
    cell_rpowers_body(GroupGeoSets{goff, cgrp}, digests, cell_idx, n_cells, 0, cc, rpow, scal, r_out);
}
// thread (g, i): weight of unique commitment i = sum of r^k over the cells that carry it (0 for the padding slots)
template <class GEO> __device__ __forceinline__ void cell_weights_body(const GEO geo, const int *cidx, const Fr *rpow, int n_cells, uint32_t *scal) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_cells) return;
    const int g = geo.group_of_cell(gid), i = geo.cell_in_group(gid, g), n = geo.count(g);
    const int *ci = cidx + (size_t)geo.first(g);
    const Fr *rp = rpow + (size_t)geo.first(g);
    Fr acc = fr_zero();
    for (int k = 0; k < n; k++) if (ci[k] == i) fr_add(acc, acc, rp[k]);
    fr_store_words(scal + 8 * (geo.term0(g) + i), acc);
}
__global__ void __launch_bounds__(256) k_cell_weights(const int *cidx, const Fr *rpow, int npg, int groups, uint32_t *scal) {
    cell_weights_body(GroupGeoUniform{npg}, cidx, rpow, npg * groups, scal);
}
__global__ void __launch_bounds__(256) k_cell_weights_sets(const int *cidx, const Fr *rpow, const int *goff, const int *cgrp, int n_cells, uint32_t *scal) {
    cell_weights_body(GroupGeoSets{goff, cgrp}, cidx, rpow, n_cells, scal);
}
// One workgroup per (group, column) segment: lane j sums r^k cell_k[j] over the segment's cells (bytes_to_bls_field on every element read,
// error into the group's word), the sum goes to LDS at rev6(j) (undoing the bit reversal), then lane t takes coefficient t of the inverse DFT
// (64 products against the twiddle table) times h_c^-t / 64.
__global__ void __launch_bounds__(CELL_FE) k_cell_columns(const uint8_t *cells, const int *perm, const int4 *segs, const Fr *rpow, const CellConsts *cc,
                                                          Fr *coef, int *err) {
    __shared__ Fr u[CELL_FE], tw[CELL_FE];
    const int4 sg = segs[blockIdx.x];                             // group, column, start, count
    const int j = threadIdx.x;
    tw[j] = cc->tw[j];
    Fr acc = fr_zero();
    bool bad = false;
    for (int m = 0; m < sg.w; m++) {
        const int k = perm[sg.z + m];                             // global cell number
        Fr v;
        bad |= !fr_from_be32_checked(v, cells + (size_t)CELL_BYTES * k + 32 * j);
        fr_mul(v, v, rpow[k]);
        fr_add(acc, acc, v);
    }
    if (bad) atomicOr(&err[sg.x], ERR_NONCANONICAL_FR);
    u[rev<6>((uint32_t)j)] = acc;
    __syncthreads();
    Fr q = fr_zero();
    for (int i = 0; i < CELL_FE; i++) { Fr t; fr_mul(t, u[i], tw[(i * j) & (CELL_FE - 1)]); fr_add(q, q, t); }
    fr_mul(q, q, cc->shift[sg.y][j]);
    coef[(size_t)blockIdx.x * CELL_FE + j] = q;
}
// one workgroup per group: I_t = sum over the group's segments; the scalar of monomial point t is -I_t
template <class GEO> __device__ __forceinline__ void cell_interp_body(const GEO geo, const Fr *coef, const int *gseg, uint32_t *scal) {
    const int g = blockIdx.x, t = threadIdx.x;
    Fr acc = fr_zero();
    for (int s = gseg[g]; s < gseg[g + 1]; s++) fr_add(acc, acc, coef[(size_t)s * CELL_FE + t]);
    Fr neg; fr_sub(neg, fr_zero(), acc);
    fr_store_words(scal + 8 * (geo.term0(g) + 2 * geo.count(g) + t), neg);
}
__global__ void __launch_bounds__(CELL_FE) k_cell_interp(const Fr *coef, const int *gseg, int npg, uint32_t *scal) {
    cell_interp_body(GroupGeoUniform{npg}, coef, gseg, scal);
}
__global__ void __launch_bounds__(CELL_FE) k_cell_interp_sets(const Fr *coef, const int *gseg, const int *goff, uint32_t *scal) {
    cell_interp_body(GroupGeoSets{goff, nullptr}, coef, gseg, scal);
}
// thread (g, term): [scalar] point.  Terms of a group: [0, n) unique commitments, [n, 2n) proofs (RL), [2n, 2n + 64) monomial points,
// [2n + 64, 3n + 64) proofs (LL).  pts is [group][commitments | proofs] as launch_decompress_points writes it.
template <class GEO>
__device__ __forceinline__ void cell_terms_body(const GEO geo, const G1Affine *pts, const G1Affine *mono, const uint32_t *scal, size_t n_terms, int groups,
                                                G1Jac *partials) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_terms) return;
    const int g = geo.group_of_term(gid, groups), e = (int)(gid - geo.term0(g)), n = geo.count(g);
    const G1Affine *gp = pts + geo.pts0(g);
    const G1Affine p = e < 2 * n ? gp[e] : e < 2 * n + CELL_FE ? mono[e - 2 * n] : gp[n + (e - 2 * n - CELL_FE)];
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = scal[8 * gid + i];
    G1Jac r; g1_mul_words(r, p, k, 8);
    partials[gid] = r;
}
__global__ void __launch_bounds__(64) k_cell_terms(const G1Affine *pts, const G1Affine *mono, const uint32_t *scal, int npg, int groups, G1Jac *partials) {
    cell_terms_body(GroupGeoUniform{npg}, pts, mono, scal, (size_t)cell_terms(npg) * groups, groups, partials);
}
__global__ void __launch_bounds__(64) k_cell_terms_sets(const G1Affine *pts, const G1Affine *mono, const uint32_t *scal, const int *goff, int n_terms,
                                                        int groups, G1Jac *partials) {
    cell_terms_body(GroupGeoSets{goff, nullptr}, pts, mono, scal, (size_t)n_terms, groups, partials);
}
// workgroup (g, side): side 0 = terms [0, 2n) (commitments, RL proofs), 1 = [2n, 2n + 64) (= -[I(tau)]), 2 = [2n + 64, 3n + 64) (LL)
constexpr int CELL_SUM_THREADS = 256;
template <class GEO> __device__ __forceinline__ void cell_sum_body(const GEO geo, const G1Jac *partials, G1Jac *sums) {
    __shared__ G1Jac red[CELL_SUM_THREADS];
    const int g = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    const int n = geo.count(g);
    const G1Jac *gt = partials + geo.term0(g);
    const int lo = side == 0 ? 0 : side == 1 ? 2 * n : 2 * n + CELL_FE;
    const int hi = side == 0 ? 2 * n : side == 1 ? 2 * n + CELL_FE : cell_terms(n);
    G1Jac acc = g1_inf();
    for (int e = lo + tid; e < hi; e += CELL_SUM_THREADS) g1_add(acc, acc, gt[e]);
    red[tid] = acc;
    __syncthreads();
    for (int s = CELL_SUM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { G1Jac a = red[tid], b = red[tid + s]; g1_add(a, a, b); red[tid] = a; }
        __syncthreads();
    }
    if (tid == 0) sums[3 * (size_t)g + side] = red[0];
}
__global__ void __launch_bounds__(CELL_SUM_THREADS) k_cell_sum(const G1Jac *partials, int npg, G1Jac *sums) {
    cell_sum_body(GroupGeoUniform{npg}, partials, sums);
}
__global__ void __launch_bounds__(CELL_SUM_THREADS) k_cell_sum_sets(const G1Jac *partials, const int *goff, G1Jac *sums) {
    cell_sum_body(GroupGeoSets{goff, nullptr}, partials, sums);
}
// The end of a group's check from its three sums a (commitments + RL proofs), b (= -[I(tau)]_1) and ll: the pairing arguments (-LL, RL) and, with
// o, r | [I(tau)]_1 | LL | RL compressed (CELL_DEBUG_BYTES)
__device__ __forceinline__ void cell_finish_group(const G1Jac &a, const G1Jac &b, const G1Jac &ll, const uint8_t *r_be, PairPt *pp, uint8_t *o) {
    G1Jac rl; g1_add(rl, a, b);
    pairpt_from_jac(pp[0], ll, true);
    pairpt_from_jac(pp[1], rl, false);
    if (!o) return;
    for (int i = 0; i < 32; i++) o[i] = r_be[i];
    G1Jac itau; g1_neg(itau, b);
#pragma unroll 1
    for (int q = 0; q < 3; q++) {
        const G1Jac p = q == 0 ? itau : q == 1 ? ll : rl;        // by value: a table of addresses would put the three points into private memory
        G1Affine af; g1_to_affine(af, p);
        g1_compress_affine(o + 32 + 48 * q, af);
    }
}
// thread g: the end of group g's check from sums[3 g ..]
__global__ void __launch_bounds__(64) k_cell_finish(const G1Jac *sums, int groups, const uint8_t *r_be, PairPt *pair_pts, uint8_t *dbg) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    cell_finish_group(sums[3 * (size_t)g], sums[3 * (size_t)g + 1], sums[3 * (size_t)g + 2], r_be + 32 * (size_t)g, pair_pts + 2 * (size_t)g,
                      dbg ? dbg + (size_t)CELL_DEBUG_BYTES * g : nullptr);
}
// One wave per group j of a stage-2 device: parts is [j][block][side], the three sums of every block of the group's cells.  Per side lane d
// takes block d's sum and a tree over the wave adds them; lane 0 then ends the check as k_cell_finish does.  r of group j is at
// r_be + 32 (r_first + j r_stride): every device derived the r of every group in stage 1.
__global__ void __launch_bounds__(CELL_MERGE_MAX_BLOCKS) k_cell_merge(const G1Jac *parts, int blocks, int groups, const uint8_t *r_be, int r_first,
                                                                      int r_stride, PairPt *pair_pts, uint8_t *dbg) {
    __shared__ G1Jac red[CELL_MERGE_MAX_BLOCKS], sum[3];
    const int j = blockIdx.x, d = threadIdx.x;
    if (j >= groups) return;
    int top = 1;                                                  // the tree starts at the power of two at or above `blocks`
    while (top < blocks) top <<= 1;
    for (int side = 0; side < 3; side++) {
        red[d] = d < blocks ? parts[((size_t)j * blocks + d) * 3 + side] : g1_inf();
        __syncthreads();
        for (int s = top / 2; s > 0; s >>= 1) {
            if (d < s) { G1Jac a = red[d], b = red[d + s]; g1_add(a, a, b); red[d] = a; }
            __syncthreads();
        }
        if (d == 0) sum[side] = red[0];
        __syncthreads();
    }
    if (d != 0) return;
    cell_finish_group(sum[0], sum[1], sum[2], r_be + 32 * ((size_t)r_first + (size_t)j * r_stride), pair_pts + 2 * (size_t)j,
                      dbg ? dbg + (size_t)CELL_DEBUG_BYTES * j : nullptr);
}

// ---- launchers
void launch_cell_setup(const uint8_t *d_g2_tau64, CellConsts *d_cc, LineCoeff *d_lines, int *d_lines_inf, int *d_err, hipStream_t st) {
    hipLaunchKernelGGL(k_cell_consts, dim3(1), dim3(CELLS_PER_EXT_BLOB), 0, st, d_cc);
    hipLaunchKernelGGL(k_cell_lines, dim3(1), dim3(64), 0, st, d_g2_tau64, d_lines, d_lines_inf, d_err);
}
void launch_cell_scalars(const uint8_t *d_digests, const int *d_cell_idx, const int *d_cidx, int npg, int groups, int k0, const CellConsts *d_cc,
                         Fr *d_rpow, uint32_t *d_scal, uint8_t *d_r_be, hipStream_t st) {
    const int n = npg * groups;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_cell_rpowers, dim3((n + 255) / 256), dim3(256), 0, st, d_digests, d_cell_idx, npg, groups, k0, d_cc, d_rpow, d_scal, d_r_be);
    hipLaunchKernelGGL(k_cell_weights, dim3((n + 255) / 256), dim3(256), 0, st, d_cidx, d_rpow, npg, groups, d_scal);
}
void launch_cell_scalars_sets(const uint8_t *d_digests, const int *d_cell_idx, const int *d_cidx, const int *d_goff, const int *d_cgrp, int n_cells,
                              const CellConsts *d_cc, Fr *d_rpow, uint32_t *d_scal, uint8_t *d_r_be, hipStream_t st) {
    if (n_cells <= 0) return;
    hipLaunchKernelGGL(k_cell_rpowers_sets, dim3((n_cells + 255) / 256), dim3(256), 0, st, d_digests, d_cell_idx, d_goff, d_cgrp, n_cells, d_cc, d_rpow, d_scal,
                       d_r_be);
    hipLaunchKernelGGL(k_cell_weights_sets, dim3((n_cells + 255) / 256), dim3(256), 0, st, d_cidx, d_rpow, d_goff, d_cgrp, n_cells, d_scal);
}
void launch_cell_interp(const uint8_t *d_cells, const int *d_perm, const int4 *d_segs, int n_segs, const int *d_gseg, const Fr *d_rpow, const CellConsts *d_cc,
                        int npg, int groups, Fr *d_coef, uint32_t *d_scal, int *d_err, hipStream_t st) {
    if (groups <= 0) return;
    if (n_segs > 0) hipLaunchKernelGGL(k_cell_columns, dim3(n_segs), dim3(CELL_FE), 0, st, d_cells, d_perm, d_segs, d_rpow, d_cc, d_coef, d_err);
    hipLaunchKernelGGL(k_cell_interp, dim3(groups), dim3(CELL_FE), 0, st, d_coef, d_gseg, npg, d_scal);
}
void launch_cell_interp_sets(const uint8_t *d_cells, const int *d_perm, const int4 *d_segs, int n_segs, const int *d_gseg, const Fr *d_rpow,
                             const CellConsts *d_cc, const int *d_goff, int groups, Fr *d_coef, uint32_t *d_scal, int *d_err, hipStream_t st) {
    if (groups <= 0) return;
    if (n_segs > 0) hipLaunchKernelGGL(k_cell_columns, dim3(n_segs), dim3(CELL_FE), 0, st, d_cells, d_perm, d_segs, d_rpow, d_cc, d_coef, d_err);
    hipLaunchKernelGGL(k_cell_interp_sets, dim3(groups), dim3(CELL_FE), 0, st, d_coef, d_gseg, d_goff, d_scal);
}
void launch_cell_sums(const G1Affine *d_pts, const G1Affine *d_mono, const uint32_t *d_scal, int npg, int groups, G1Jac *d_partials, G1Jac *d_sums,
                      hipStream_t st) {
    if (groups <= 0) return;
    const size_t terms = (size_t)cell_terms(npg) * groups;
    hipLaunchKernelGGL(k_cell_terms, dim3((unsigned)((terms + 63) / 64)), dim3(64), 0, st, d_pts, d_mono, d_scal, npg, groups, d_partials);
    hipLaunchKernelGGL(k_cell_sum, dim3(groups, 3), dim3(CELL_SUM_THREADS), 0, st, d_partials, npg, d_sums);
}
void launch_cell_lincomb(const G1Affine *d_pts, const G1Affine *d_mono, const uint32_t *d_scal, int npg, int groups, G1Jac *d_partials, G1Jac *d_sums,
                         const uint8_t *d_r_be, PairPt *d_pair_pts, uint8_t *d_dbg, hipStream_t st) {
    if (groups <= 0) return;
    launch_cell_sums(d_pts, d_mono, d_scal, npg, groups, d_partials, d_sums, st);
    hipLaunchKernelGGL(k_cell_finish, dim3((groups + 63) / 64), dim3(64), 0, st, d_sums, groups, d_r_be, d_pair_pts, d_dbg);
}
void launch_cell_lincomb_sets(const G1Affine *d_pts, const G1Affine *d_mono, const uint32_t *d_scal, const int *d_goff, int n_cells, int groups,
                              G1Jac *d_partials, G1Jac *d_sums, const uint8_t *d_r_be, PairPt *d_pair_pts, uint8_t *d_dbg, hipStream_t st) {
    if (groups <= 0) return;
    const int terms = cell_terms_sets(n_cells, groups);
    hipLaunchKernelGGL(k_cell_terms_sets, dim3((unsigned)((terms + 63) / 64)), dim3(64), 0, st, d_pts, d_mono, d_scal, d_goff, terms, groups, d_partials);
    hipLaunchKernelGGL(k_cell_sum_sets, dim3(groups, 3), dim3(CELL_SUM_THREADS), 0, st, d_partials, d_goff, d_sums);
    hipLaunchKernelGGL(k_cell_finish, dim3((groups + 63) / 64), dim3(64), 0, st, d_sums, groups, d_r_be, d_pair_pts, d_dbg);
}
bool launch_cell_merge(const G1Jac *d_parts, int blocks, int groups, const uint8_t *d_r_be, int r_first, int r_stride, PairPt *d_pair_pts, uint8_t *d_dbg,
                       hipStream_t st) {
    if (blocks <= 0 || blocks > CELL_MERGE_MAX_BLOCKS) return false;
    if (groups > 0)
        hipLaunchKernelGGL(k_cell_merge, dim3(groups), dim3(CELL_MERGE_MAX_BLOCKS), 0, st, d_parts, blocks, groups, d_r_be, r_first, r_stride, d_pair_pts, d_dbg);
    return true;
}

}  // namespace kzg
