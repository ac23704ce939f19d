// group_geo.h -- where the groups of a cell launch set lie, behind one small interface (k_cells.hip, and the point kernels of k_cell_points.hip).  Cells
// are numbered group after group.  Group g holds count(g) cells from first(g) on; its points, [count(g) unique-commitment slots | count(g) proofs],
// start at pts0(g); its cell_terms(count(g)) lincomb terms start at term0(g).  A kernel body takes the geometry as a template argument and is
// instantiated once per form under a thin __global__ wrapper:
//   GroupGeoUniform   every group has npg cells: arithmetic on npg, the expressions the kernels had before there was a second form
//   GroupGeoSets      every group has its own count (kzg355_verify_cell_kzg_proof_batch_many_sets): goff[groups + 1], the cells before each
//                     group, STRICTLY increasing (the host drops empty groups), and cgrp[cells], the group of each cell
// Index width: a launch set has at most 2^18 cells and at most as many (non-empty) groups, so a term index stays below 3 2^18 + 64 2^18 < 2^25
// and fits int; the uniform form keeps the size_t products it always had.
#pragma once
#include "kernels.h"

namespace kzg {

struct GroupGeoUniform {
    int npg;
    __device__ __forceinline__ int group_of_cell(int c) const { return c / npg; }
    __device__ __forceinline__ int cell_in_group(int c, int) const { return c % npg; }
    __device__ __forceinline__ int first(int g) const { return g * npg; }
    __device__ __forceinline__ int count(int) const { return npg; }
    __device__ __forceinline__ size_t pts0(int g) const { return (size_t)g * 2 * npg; }
    __device__ __forceinline__ size_t term0(int g) const { return (size_t)g * cell_terms(npg); }
    __device__ __forceinline__ int group_of_term(size_t t, int) const { return (int)(t / cell_terms(npg)); }
};

struct GroupGeoSets {
    const int *goff, *cgrp;
    __device__ __forceinline__ int group_of_cell(int c) const { return cgrp[c]; }
    __device__ __forceinline__ int cell_in_group(int c, int g) const { return c - goff[g]; }
    __device__ __forceinline__ int first(int g) const { return goff[g]; }
    __device__ __forceinline__ int count(int g) const { return goff[g + 1] - goff[g]; }
    __device__ __forceinline__ size_t pts0(int g) const { return (size_t)2 * goff[g]; }
    __device__ __forceinline__ size_t term0(int g) const { return (size_t)(3 * goff[g] + CELL_FE * g); }
    // the last group whose terms start at or before t (term0 is strictly increasing in g): at most 18 steps beside a 255-bit scalar multiplication
    __device__ __forceinline__ int group_of_term(size_t t, int groups) const {
        int lo = 0, hi = groups - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (term0(mid) <= t) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
    // point slots 2 first(g) .. 2 first(g + 1) belong to group g, so slot j lies in the group of cell j / 2
    __device__ __forceinline__ int group_of_point(int j) const { return cgrp[j >> 1]; }
};

}  // namespace kzg
