// k_cell_points.hip -- validate_kzg_g1 on the points of a cell launch set whose groups have their own sizes
// (kzg355_verify_cell_kzg_proof_batch_many_sets): what k_decompress_points and k_subgroup_points / k_subgroup_points_quad (k_g1.hip) do for
// groups of one size, with a point's slot and its group's error word taken from the ragged geometry of group_geo.h.  The predicates are the
// shared ones (g1_decompress, g1_in_subgroup, g1_phi_matches; the quad ladder is the routines of g1_quad.h in k_g1.hip's order); only the
// placement differs.  These are kernels of their own, in a translation unit of their own, because k_g1.hip holds the kernels the blob
// benchmark times: its code object stays exactly what it was.
#define KZG_MID_INLINE 1
#include "kernels.h"
#include "g1_quad.h"
#include "group_geo.h"

namespace kzg {

// thread j < n_cells: unique-commitment slot j; j >= n_cells: proof j - n_cells.  48 bytes -> affine point into the group's
// [slots | proofs] (infinity where the decoding failed, ERR_BAD_POINT on the group)
__global__ void __launch_bounds__(64) k_decompress_points_sets(const uint8_t *commitments, const uint8_t *proofs, int n_cells, const int *goff, const int *cgrp,
                                                               G1Affine *pts, int *err) {
    const GroupGeoSets geo{goff, cgrp};
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * n_cells) return;
    const bool is_proof = j >= n_cells;
    const int i = is_proof ? j - n_cells : j;
    const uint8_t *src = (is_proof ? proofs : commitments) + (size_t)48 * i;
    uint8_t b[48];
    for (int k = 0; k < 48; k++) b[k] = src[k];
    G1Affine p;
    const int rc = g1_decompress(p, b);
    const int g = geo.group_of_cell(i), k = geo.cell_in_group(i, g);
    if (rc != 0) { atomicOr(&err[g], ERR_BAD_POINT); p = g1a_inf(); }
    pts[geo.pts0(g) + (is_proof ? geo.count(g) + k : k)] = p;
}
// thread j: the subgroup test of point slot j (infinity is accepted, utils.rs:298-301)
__global__ void __launch_bounds__(64) k_subgroup_points_sets(const G1Affine *pts, int n_points, const int *goff, const int *cgrp, int *err) {
    const GroupGeoSets geo{goff, cgrp};
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_points) return;
    const G1Affine p = pts[j];
    if (!g1a_is_inf(p) && !g1_in_subgroup(p)) atomicOr(&err[geo.group_of_point(j)], ERR_BAD_POINT);
}
// the same by DPP quads for few points (four lanes per point: the latency form, as k_subgroup_points_quad): [x^2]P by two passes of the 63-step
// ladder for |x| = 0xd201000000010000, then phi(P) == -[x^2]P
__global__ void __launch_bounds__(256) k_subgroup_points_quad_sets(const G1Affine *pts, int n_points, const int *goff, const int *cgrp, int *err) {
    const GroupGeoSets geo{goff, cgrp};
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, role = tid & 3;
    const bool live = (tid >> 2) < n_points;
    const int j = live ? (tid >> 2) : n_points - 1;               // idle quads redo the last point (every lane takes part in the DPP moves)
    G1Affine p = pts[j];
    if (!live) p = g1a_inf();
    G1Jac base; g1_from_affine(base, p);
    G1Jac t = base;
#pragma unroll 1
    for (int step = 0; step < 126; step++) {
        const int i = 62 - (step % 63);
        if (step == 63) { g1_canon_lazy(t, t); base = t; }       // second ladder: [|x|] of the first one's result
        g1_dbl_quad(t, role);
        if ((BLS_X_ABS >> i) & 1) g1_add_quad(t, t, base, role);  // (a constant exponent: the branch is uniform)
    }
    g1_canon_lazy(t, t);
    const bool ok = g1a_is_inf(p) || g1_phi_matches(p, t);
    if (live && role == 0 && !ok) atomicOr(&err[geo.group_of_point(j)], ERR_BAD_POINT);
}

void launch_cell_points_sets(const uint8_t *d_commitments, const uint8_t *d_proofs, const int *d_goff, const int *d_cgrp, int n_cells, G1Affine *d_pts,
                             int *d_err, hipStream_t st) {
    if (n_cells <= 0) return;
    const int n_points = 2 * n_cells;
    hipLaunchKernelGGL(k_decompress_points_sets, dim3((n_points + 63) / 64), dim3(64), 0, st, d_commitments, d_proofs, n_cells, d_goff, d_cgrp, d_pts, d_err);
    if (n_points <= 1024)               // few points: four lanes per point, the threshold of launch_subgroup_points
        hipLaunchKernelGGL(k_subgroup_points_quad_sets, dim3((4 * n_points + 255) / 256), dim3(256), 0, st, d_pts, n_points, d_goff, d_cgrp, d_err);
    else
        hipLaunchKernelGGL(k_subgroup_points_sets, dim3((n_points + 63) / 64), dim3(64), 0, st, d_pts, n_points, d_goff, d_cgrp, d_err);
}

}  // namespace kzg
