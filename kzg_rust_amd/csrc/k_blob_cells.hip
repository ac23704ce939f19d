// k_blob_cells.hip -- verify_blob_cell_proofs_batch on the device (blob_cells.hip): what a batch of ALL 128 cells of every blob, in cell order,
// adds to the kernels of k_cell_compute.hip (the extension) and k_cells.hip (the check).
//
// Blob b of a group has the monomial coefficients f_b (k_cc_field's inverse NTT) and sits at cells 128 b .. 128 b + 127 of its group, cell k with
// the weight r^(128 b + k).  The interpolant of cell k of blob b has the coefficients I_{b,k}[t] = P_{b,t}(a_k), P_{b,t}(y) = sum_u f_{b,64u+t} y^u,
// a_k = h_k^64 = w128^rev7(k), so the batch interpolant is
//     I[t] = sum_b sum_k r^(128 b + k) sum_u f_{b,64u+t} a_k^u = sum_{u<64} W[u] * ( sum_b r^(128 b) f_{b,64u+t} ),   W[u] = sum_{k<128} r^k a_k^u:
// 64 weights per group (k_blob_weights; a_k^u = w128^(rev7(k) u mod 128) is a lookup), one multiply-add per blob coefficient and one product with
// W[u] (k_blob_coef).  The products land in the segment layout of k_cell_columns, 64 "segments" u per group, so that k_cell_interp adds them up
// and the rest of the chain runs as it does for any cell batch.
// k_blob_meta writes what the host preparation of cells.hip would: every array follows from the position of each blob's commitment among its
// group's unique ones, with no sort.
// The field products are inlined here as in k_cells.hip: no kernel of this file uses scratch.
#define KZG_MID_INLINE 1
#include "kernels.h"
#include "cell_domain.h"

namespace kzg {

// Where the groups of a launch set lie, in blobs: the geometry of group_geo.h one level up.  Every group is whole blobs of 128 cells, so the cell
// offsets of the `_sets` chain (goff, cgrp) describe the blobs too -- goff[g] / 128 blobs lie before group g -- and no second offset array exists.
// Each kernel below has ONE body and two entries, as in k_cells.hip: the uniform one (n blobs per group; its name and arguments as they were) and
// the `_sets` one (kzg355_verify_blob_cell_proofs_batch_many_sets: every group its own blob count).
struct BlobGeoUniform {
    int n;
    __device__ __forceinline__ int group_of_cell(int c) const { return c / (CELLS_PER_EXT_BLOB * n); }
    __device__ __forceinline__ int first(int g) const { return g * (CELLS_PER_EXT_BLOB * n); }       // cells before group g
    __device__ __forceinline__ int first_blob(int g) const { return g * n; }                           // blobs before group g
    __device__ __forceinline__ int blobs(int) const { return n; }
};
struct BlobGeoSets {
    const int *goff, *cgrp;
    __device__ __forceinline__ int group_of_cell(int c) const { return cgrp[c]; }
    __device__ __forceinline__ int first(int g) const { return goff[g]; }
    __device__ __forceinline__ int first_blob(int g) const { return goff[g] / CELLS_PER_EXT_BLOB; }
    __device__ __forceinline__ int blobs(int g) const { return (goff[g + 1] - goff[g]) / CELLS_PER_EXT_BLOB; }
};

// thread i = cell i of the launch set, in group g = group_of_cell(i) of n blobs whose cells start at c0 = first(g) and whose blobs at b0 =
// first_blob(g) (uniform: c0 = g npg, b0 = g n, npg = 128 n): cell k = j mod 128 of blob b = j / 128, j = i - c0.  Cell index k, commitment position
// pos[b0 + b], the transcript's index array, slot j of the group's padded unique-commitment list, and -- segs set: the column form -- the column
// sort (column k of a group holds its n cells 128 b + k, b ascending) with one segment per column.  seg_cap segments per group (128 columns, or
// the 64 of k_blob_coef).  The first n threads of a group fold their blob's error word into the group's.
template <class GEO>
__device__ __forceinline__ void blob_meta_body(const GEO geo, const int *pos, const int *ucount, const uint8_t *uc_in, const int *blob_err, int n_cells,
                                               int groups, int seg_cap, int4 *segs, int *gseg, int *cell, int *cidx, int *perm, uint64_t *indices, uint8_t *uc,
                                               int *err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cells) return;
    const int g = geo.group_of_cell(i), c0 = geo.first(g), b0 = geo.first_blob(g), n = geo.blobs(g);
    const int j = i - c0, b = j / CELLS_PER_EXT_BLOB, k = j % CELLS_PER_EXT_BLOB;
    cell[i] = k;
    cidx[i] = pos[b0 + b];
    if (indices) indices[i] = (uint64_t)k;
    if (segs) {
        perm[c0 + k * n + b] = i;
        if (j < CELLS_PER_EXT_BLOB) segs[(size_t)g * seg_cap + j] = make_int4(g, j, c0 + j * n, n);
    }
    if (j == 0) { gseg[g] = g * seg_cap; if (g == groups - 1) gseg[groups] = groups * seg_cap; }
    uint4 *dst = reinterpret_cast<uint4 *>(uc + 48 * (size_t)i);
    if (j < ucount[g]) {
        const uint4 *src = reinterpret_cast<const uint4 *>(uc_in + 48 * ((size_t)b0 + j));
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    } else {                                                      // infinity, weight 0
        dst[0] = make_uint4(0xc0u, 0u, 0u, 0u); dst[1] = make_uint4(0u, 0u, 0u, 0u); dst[2] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (j < n && blob_err[b0 + j]) atomicOr(&err[g], blob_err[b0 + j]);
}
__global__ void __launch_bounds__(256) k_blob_meta(const int *pos, const int *ucount, const uint8_t *uc_in, const int *blob_err, int n, int groups, int seg_cap,
                                                   int4 *segs, int *gseg, int *cell, int *cidx, int *perm, uint64_t *indices, uint8_t *uc, int *err) {
    blob_meta_body(BlobGeoUniform{n}, pos, ucount, uc_in, blob_err, CELLS_PER_EXT_BLOB * n * groups, groups, seg_cap, segs, gseg, cell, cidx, perm, indices, uc,
                   err);
}
__global__ void __launch_bounds__(256) k_blob_meta_sets(const int *pos, const int *ucount, const uint8_t *uc_in, const int *blob_err, const int *goff,
                                                        const int *cgrp, int n_cells, int groups, int seg_cap, int4 *segs, int *gseg, int *cell, int *cidx,
                                                        int *perm, uint64_t *indices, uint8_t *uc, int *err) {
    blob_meta_body(BlobGeoSets{goff, cgrp}, pos, ucount, uc_in, blob_err, n_cells, groups, seg_cap, segs, gseg, cell, cidx, perm, indices, uc, err);
}

// one workgroup per group, lane u: W[u] = sum_k r^k w128^(rev7(k) u); rpow is [group][its cells], a group's first 128 entries r^0 .. r^127
template <class GEO> __device__ __forceinline__ void blob_weights_body(const GEO geo, const Fr *rpow, const CellComputeConsts *cc, Fr *W) {
    __shared__ Fr rp[CELLS_PER_EXT_BLOB];
    const int g = blockIdx.x, u = threadIdx.x;
    const Fr *src = rpow + (size_t)geo.first(g);
    rp[u] = src[u];
    rp[u + CELL_FE] = src[u + CELL_FE];
    __syncthreads();
    Fr acc = fr_zero();
    for (int k = 0; k < CELLS_PER_EXT_BLOB; k++) {
        const uint32_t e = (rev<7>((uint32_t)k) * (uint32_t)u) & (uint32_t)(CC_FFT - 1);
        Fr t; fr_mul(t, rp[k], cc->w4096[e * (N_FE / CC_FFT)]);
        fr_add(acc, acc, t);
    }
    W[(size_t)g * CELL_FE + u] = acc;
}
__global__ void __launch_bounds__(CELL_FE) k_blob_weights(const Fr *rpow, const CellComputeConsts *cc, int n, Fr *W) {
    blob_weights_body(BlobGeoUniform{n}, rpow, cc, W);
}
__global__ void __launch_bounds__(CELL_FE) k_blob_weights_sets(const Fr *rpow, const CellComputeConsts *cc, const int *goff, Fr *W) {
    blob_weights_body(BlobGeoSets{goff, nullptr}, rpow, cc, W);
}

// one workgroup per (group, u), lane t: W[u] * sum_b r^(128 b) f_b[64 u + t] -> coef[(64 g + u) * 64 + t], b over the group's own blobs (f holds
// the blobs of the launch set one after the other: the group's start at first_blob(g))
template <class GEO> __device__ __forceinline__ void blob_coef_body(const GEO geo, const Fr *f, const Fr *rpow, const Fr *W, Fr *coef) {
    const int g = blockIdx.x / CELL_FE, u = blockIdx.x % CELL_FE, t = threadIdx.x;
    const int n = geo.blobs(g);
    const Fr *fb = f + (size_t)geo.first_blob(g) * N_FE + CELL_FE * u + t;
    const Fr *rp = rpow + (size_t)geo.first(g);
    Fr acc = fb[0];                                               // r^0
    for (int b = 1; b < n; b++) {
        Fr v; fr_mul(v, fb[(size_t)b * N_FE], rp[(size_t)CELLS_PER_EXT_BLOB * b]);
        fr_add(acc, acc, v);
    }
    fr_mul(acc, acc, W[(size_t)g * CELL_FE + u]);
    coef[(size_t)blockIdx.x * CELL_FE + t] = acc;
}
__global__ void __launch_bounds__(CELL_FE) k_blob_coef(const Fr *f, const Fr *rpow, const Fr *W, int n, Fr *coef) {
    blob_coef_body(BlobGeoUniform{n}, f, rpow, W, coef);
}
__global__ void __launch_bounds__(CELL_FE) k_blob_coef_sets(const Fr *f, const Fr *rpow, const Fr *W, const int *goff, Fr *coef) {
    blob_coef_body(BlobGeoSets{goff, nullptr}, f, rpow, W, coef);
}

// ---- launchers
void launch_blob_cell_meta(const int *d_pos, const int *d_ucount, const uint8_t *d_uc_in, const int *d_blob_err, int n, int groups, bool columns, int4 *d_segs,
                           int *d_gseg, int *d_cell, int *d_cidx, int *d_perm, size_t *d_indices, uint8_t *d_uc, int *d_err, hipStream_t st) {
    if (groups <= 0 || n <= 0) return;
    static_assert(sizeof(size_t) == sizeof(uint64_t), "cell indices are 64-bit");
    const int N = CELLS_PER_EXT_BLOB * n * groups;
    hipLaunchKernelGGL(k_blob_meta, dim3((N + 255) / 256), dim3(256), 0, st, d_pos, d_ucount, d_uc_in, d_blob_err, n, groups,
                       columns ? CELLS_PER_EXT_BLOB : CELL_FE, columns ? d_segs : nullptr, d_gseg, d_cell, d_cidx, d_perm,
                       reinterpret_cast<uint64_t *>(d_indices), d_uc, d_err);
}
void launch_blob_cell_coefs(const Fr *d_f, const Fr *d_rpow, const CellComputeConsts *d_cc, int n, int groups, Fr *d_W, Fr *d_coef, hipStream_t st) {
    if (groups <= 0 || n <= 0) return;
    hipLaunchKernelGGL(k_blob_weights, dim3(groups), dim3(CELL_FE), 0, st, d_rpow, d_cc, n, d_W);
    hipLaunchKernelGGL(k_blob_coef, dim3(groups * CELL_FE), dim3(CELL_FE), 0, st, d_f, d_rpow, d_W, n, d_coef);
}
void launch_blob_cell_meta_sets(const int *d_pos, const int *d_ucount, const uint8_t *d_uc_in, const int *d_blob_err, const int *d_goff, const int *d_cgrp,
                                int n_cells, int groups, bool columns, int4 *d_segs, int *d_gseg, int *d_cell, int *d_cidx, int *d_perm, size_t *d_indices,
                                uint8_t *d_uc, int *d_err, hipStream_t st) {
    if (groups <= 0 || n_cells <= 0) return;
    hipLaunchKernelGGL(k_blob_meta_sets, dim3((n_cells + 255) / 256), dim3(256), 0, st, d_pos, d_ucount, d_uc_in, d_blob_err, d_goff, d_cgrp, n_cells, groups,
                       columns ? CELLS_PER_EXT_BLOB : CELL_FE, columns ? d_segs : nullptr, d_gseg, d_cell, d_cidx, d_perm,
                       reinterpret_cast<uint64_t *>(d_indices), d_uc, d_err);
}
void launch_blob_cell_coefs_sets(const Fr *d_f, const Fr *d_rpow, const CellComputeConsts *d_cc, const int *d_goff, int groups, Fr *d_W, Fr *d_coef,
                                 hipStream_t st) {
    if (groups <= 0) return;
    hipLaunchKernelGGL(k_blob_weights_sets, dim3(groups), dim3(CELL_FE), 0, st, d_rpow, d_cc, d_goff, d_W);
    hipLaunchKernelGGL(k_blob_coef_sets, dim3(groups * CELL_FE), dim3(CELL_FE), 0, st, d_f, d_rpow, d_W, d_goff, d_coef);
}

}  // namespace kzg
