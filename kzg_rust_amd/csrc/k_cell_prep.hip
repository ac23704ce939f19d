// k_cell_prep.hip -- the preparation of a verify_cell_kzg_proof_batch call on the device, for inputs that are resident in HBM (cells.hip: the
// *_device entry points).  It leaves what the host preparation of cells.hip leaves -- the clamped cell indices, each cell's position in its
// group's list of unique commitments (first-appearance order), that list padded with the encoding of infinity, the cells sorted by column with
// one segment per column, and the SHA-256 digest of the group's transcript -- so that the kernels of k_cells.hip run on either unchanged.
//
// k_cell_prep: one workgroup per group.  Commitments are deduplicated through an open-addressing table of cell numbers (LDS up to 4096 cells per
// group, HBM above): a cell claims the slot its commitment hashes to or, if the slot's owner has the same 48 bytes (compared in full: the hash only
// picks the slot), lowers the owner to the smaller cell number; otherwise it probes on.  After a barrier every slot holds the first cell of its
// commitment, and a scan over "I am that first cell" in cell order numbers the unique commitments as the host's pass over the cells does.
// The column sort counts with LDS atomics and places serially per column (one thread per column walks the group's cells in order: stable).
// The segment list has a fixed stride of min(n, 128) slots per group, the columns present first and empty segments (count 0) behind them: the
// host knows the number of segments, here it would be data, and an empty segment contributes zero to its group's interpolant.
// k_cell_prep_sets is the same body on groups of different sizes (kzg355_verify_cell_kzg_proof_batch_many_sets_device).
//
// k_cell_rhash_lanes / k_cell_rhash_wave: the transcript "RCKZGCBATCH__V1_" | u64be(4096) | u64be(64) | u64be(u) | u64be(n) | unique commitments |
// per cell: u64be(position) u64be(index) cell proof, gathered from the caller's buffers 16 bytes at a time (every piece of the message is a
// multiple of 16 bytes long and every source 16-byte aligned; nothing is staged).  The two shapes are those of the blob path's batch challenge
// (k_verify.hip): one lane per group when the groups outnumber the SIMDs, and one wave per group otherwise, whose 64 lanes expand the message
// schedule of 64 blocks at once before lane 0 runs their rounds.
#include "kernels.h"
#include "sha256_rounds.h"
#include "fr_block.h"

namespace kzg {

// ------------------------------------------------------------------------------------------------ dedup + column sort
struct Key48 { uint4 a, b, c; };
__device__ __forceinline__ Key48 cp_key(const uint8_t *commitments, size_t cell) {
    const uint4 *p = reinterpret_cast<const uint4 *>(commitments + 48 * cell);
    Key48 k; k.a = p[0]; k.b = p[1]; k.c = p[2];
    return k;
}
__device__ __forceinline__ bool cp_same(const Key48 &x, const Key48 &y) {
    const uint32_t d = (x.a.x ^ y.a.x) | (x.a.y ^ y.a.y) | (x.a.z ^ y.a.z) | (x.a.w ^ y.a.w) | (x.b.x ^ y.b.x) | (x.b.y ^ y.b.y) | (x.b.z ^ y.b.z) |
                       (x.b.w ^ y.b.w) | (x.c.x ^ y.c.x) | (x.c.y ^ y.c.y) | (x.c.z ^ y.c.z) | (x.c.w ^ y.c.w);
    return d == 0;
}
// picks the slot only: equality is decided on the 48 bytes
__device__ __forceinline__ uint32_t cp_hash(const Key48 &k) {
    const uint32_t w[12] = {k.a.x, k.a.y, k.a.z, k.a.w, k.b.x, k.b.y, k.b.z, k.b.w, k.c.x, k.c.y, k.c.z, k.c.w};
    uint32_t h = 0x9e3779b9u;
#pragma unroll
    for (int i = 0; i < 12; i++) { h ^= w[i]; h *= 0x85ebca6bu; h ^= h >> 15; }
    return h;
}

constexpr int CP_THREADS = 256;
constexpr int CP_SORT_TILE = 2048;     // cells whose columns one placement step keeps in LDS
// k_cell_prep has one body and two entries, as the hash kernels below: the uniform one (every group npg cells, its arithmetic on npg) and the
// `_sets` one (group g is cells goff[g] .. goff[g + 1] - 1).  The body prepares the npg cells from `base` on as group g: its segment slots are
// seg0 .. seg0 + seg_cap - 1, its dedup table is `tab` (tab_size slots in HBM) or, with tab null, the LDS one.
__device__ __forceinline__ void cp_prep_body(const uint8_t *commitments, const uint64_t *indices, size_t base, int npg, int g, size_t seg0, int seg_cap,
                                             int *tab, int tab_size, uint8_t *uc, int4 *segs, int *cell, int *cidx, int *perm, int *ucount, int *err) {
    __shared__ int tab_l[CELL_PREP_LDS_SLOTS];
    __shared__ uint8_t col_l[CP_SORT_TILE];
    __shared__ int cnt[CELLS_PER_EXT_BLOB], at[CELLS_PER_EXT_BLOB];
    __shared__ int wsum[CP_THREADS / 64], n_segs_l;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (!tab) tab = tab_l;
    const uint32_t mask = (uint32_t)tab_size - 1u;

    for (int t = tid; t < tab_size; t += CP_THREADS) tab[t] = -1;
    if (tid < CELLS_PER_EXT_BLOB) cnt[tid] = 0;
    __syncthreads();
    // cell indices: an index >= 128 is the group's error; the clamped index goes on
    bool bad = false;
    for (int k = tid; k < npg; k += CP_THREADS) {
        const uint64_t c = indices[base + k];
        bad |= c >= (uint64_t)CELLS_PER_EXT_BLOB;
        const int cc = c < (uint64_t)CELLS_PER_EXT_BLOB ? (int)c : 0;
        cell[base + k] = cc;
        atomicAdd(&cnt[cc], 1);
    }
    if (bad) atomicOr(&err[g], ERR_CELL_INDEX);
    // every cell into the table; cidx holds its slot for now
    for (int k = tid; k < npg; k += CP_THREADS) {
        const Key48 key = cp_key(commitments, base + k);
        uint32_t slot = cp_hash(key) & mask;
        for (;;) {
            const int cur = atomicCAS(&tab[slot], -1, k);
            if (cur == -1) break;
            if (cp_same(key, cp_key(commitments, base + cur))) { atomicMin(&tab[slot], k); break; }
            slot = (slot + 1u) & mask;                             // (the table has at least 2 n slots: a free one exists)
        }
        cidx[base + k] = (int)slot;
    }
    __syncthreads();
    // number the unique commitments in cell order; perm holds the number of a first cell for now
    int u = 0;
    for (int k0 = 0; k0 < npg; k0 += CP_THREADS) {
        const int k = k0 + tid;
        const bool first = k < npg && tab[cidx[base + k]] == k;
        const uint64_t bal = __ballot(first);
        if (lane == 0) wsum[wid] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int q = 0; q < CP_THREADS / 64; q++) { if (q < wid) before += wsum[q]; total += wsum[q]; }
        if (first) {
            const int pos = u + before;
            perm[base + k] = pos;
            const Key48 key = cp_key(commitments, base + k);
            uint4 *dst = reinterpret_cast<uint4 *>(uc + 48 * (base + pos));
            dst[0] = key.a; dst[1] = key.b; dst[2] = key.c;
        }
        u += total;
        __syncthreads();
    }
    for (int k = tid; k < npg; k += CP_THREADS) cidx[base + k] = perm[base + tab[cidx[base + k]]];
    for (int i = u + tid; i < npg; i += CP_THREADS) {             // infinity, weight 0
        uint4 *dst = reinterpret_cast<uint4 *>(uc + 48 * (base + i));
        dst[0] = make_uint4(0xc0u, 0u, 0u, 0u); dst[1] = make_uint4(0u, 0u, 0u, 0u); dst[2] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (tid == 0) ucount[g] = u;
    __syncthreads();                                              // perm is the sort's from here on
    // stable counting sort by column
    if (tid < CELLS_PER_EXT_BLOB) {
        int acc = 0, ord = 0;
        for (int c = 0; c < tid; c++) { acc += cnt[c]; ord += cnt[c] != 0; }
        at[tid] = acc;
        if (cnt[tid]) segs[seg0 + ord] = make_int4(g, tid, (int)base + acc, cnt[tid]);
        if (tid == CELLS_PER_EXT_BLOB - 1) n_segs_l = ord + (cnt[tid] != 0);
    }
    __syncthreads();
    for (int i = n_segs_l + tid; i < seg_cap; i += CP_THREADS) segs[seg0 + i] = make_int4(g, 0, (int)base, 0);
    int put = tid < CELLS_PER_EXT_BLOB ? at[tid] : 0;
    for (int k0 = 0; k0 < npg; k0 += CP_SORT_TILE) {
        const int len = npg - k0 < CP_SORT_TILE ? npg - k0 : CP_SORT_TILE;
        for (int i = tid; i < len; i += CP_THREADS) col_l[i] = (uint8_t)cell[base + k0 + i];
        __syncthreads();
        if (tid < CELLS_PER_EXT_BLOB)
            for (int i = 0; i < len; i++)
                if (col_l[i] == tid) perm[base + put++] = (int)base + k0 + i;
        __syncthreads();
    }
}
// (gtab is set when tab_size > CELL_PREP_LDS_SLOTS)
__global__ void __launch_bounds__(CP_THREADS) k_cell_prep(const uint8_t *commitments, const uint64_t *indices, int npg, int groups, int seg_cap, int tab_size,
                                                          int *gtab, uint8_t *uc, int4 *segs, int *gseg, int *cell, int *cidx, int *perm, int *ucount,
                                                          int *err) {
    const int g = blockIdx.x;
    if (threadIdx.x == 0) { gseg[g] = g * seg_cap; if (g == groups - 1) gseg[groups] = groups * seg_cap; }
    cp_prep_body(commitments, indices, (size_t)g * npg, npg, g, (size_t)g * seg_cap, seg_cap, gtab ? gtab + (size_t)g * tab_size : nullptr, tab_size, uc,
                 segs, cell, cidx, perm, ucount, err);
}
// Groups of different sizes: the table of a group of n cells has cell_prep_table_slots(n) < 4 n slots, so an HBM one at gtab + 4 goff[g] ends
// before its neighbour's begins (gtab: 4 ints per cell of the launch set, or null when no group's table exceeds LDS).  gseg (the prefix sums of
// min(count, 128)) comes from the host, which knows the counts; the group of every cell is written here.
__global__ void __launch_bounds__(CP_THREADS) k_cell_prep_sets(const uint8_t *commitments, const uint64_t *indices, const int *goff, const int *gseg,
                                                               int *gtab, uint8_t *uc, int4 *segs, int *cell, int *cidx, int *perm, int *cgrp,
                                                               int *ucount, int *err) {
    const int g = blockIdx.x, base = goff[g], npg = goff[g + 1] - base, tab_size = cell_prep_table_slots(npg);
    for (int k = threadIdx.x; k < npg; k += CP_THREADS) cgrp[base + k] = g;
    cp_prep_body(commitments, indices, (size_t)base, npg, g, (size_t)gseg[g], npg < CELLS_PER_EXT_BLOB ? npg : CELLS_PER_EXT_BLOB,
                 tab_size > CELL_PREP_LDS_SLOTS ? gtab + 4 * (size_t)base : nullptr, tab_size, uc, segs, cell, cidx, perm, ucount, err);
}

// ------------------------------------------------------------------------------------------------ transcript hash
constexpr uint32_t CP_CELL_QUADS = 1u + CELL_BYTES / 16u + 3u;    // u64be(position) u64be(index) | cell | proof, in 16-byte pieces: 132
struct CellMsg {
    const uint4 *uc, *cells, *proofs;       // of the group
    const uint64_t *indices;
    const int *cidx;
    uint32_t u, n, nq, nblocks;             // unique commitments, cells, 16-byte pieces of the message, SHA-256 blocks
    uint64_t bits;
};
// the message of group g: its n cells are cells base .. base + n - 1 of the launch set (uniform groups: base = g npg, n = npg)
__device__ __forceinline__ CellMsg cp_msg(const uint8_t *uc, const uint64_t *indices, const uint8_t *cells, const uint8_t *proofs, const int *cidx,
                                          const int *ucount, size_t base, int n, int g) {
    CellMsg m;
    m.uc = reinterpret_cast<const uint4 *>(uc + 48 * base);
    m.cells = reinterpret_cast<const uint4 *>(cells + (size_t)CELL_BYTES * base);
    m.proofs = reinterpret_cast<const uint4 *>(proofs + 48 * base);
    m.indices = indices + base;
    m.cidx = cidx + base;
    m.u = (uint32_t)ucount[g]; m.n = (uint32_t)n;
    m.nq = 3u + 3u * m.u + CP_CELL_QUADS * m.n;
    m.nblocks = (m.nq * 16u + 9u + 63u) / 64u;
    m.bits = (uint64_t)m.nq * 128u;
    return m;
}
__device__ __forceinline__ uint4 cp_swap(const uint4 v) { return make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w)); }
// piece q of the padded message as four big-endian words
__device__ __forceinline__ uint4 cp_quad(const CellMsg &m, uint32_t q) {
    if (q >= m.nq) {
        uint4 v = make_uint4(q == m.nq ? 0x80000000u : 0u, 0u, 0u, 0u);
        if (q == 4u * m.nblocks - 1u) { v.z = (uint32_t)(m.bits >> 32); v.w = (uint32_t)m.bits; }
        return v;
    }
    if (q >= 3u + 3u * m.u) {
        const uint32_t t = q - 3u - 3u * m.u, k = t / CP_CELL_QUADS, j = t - k * CP_CELL_QUADS;
        if (j == 0u) { const uint64_t c = m.indices[k]; return make_uint4(0u, (uint32_t)m.cidx[k], (uint32_t)(c >> 32), (uint32_t)c); }
        if (j <= CELL_BYTES / 16u) return cp_swap(m.cells[(size_t)k * (CELL_BYTES / 16u) + (j - 1u)]);
        return cp_swap(m.proofs[(size_t)k * 3u + (j - 1u - CELL_BYTES / 16u)]);
    }
    if (q >= 3u) return cp_swap(m.uc[q - 3u]);
    if (q == 0u) return make_uint4(0x52434b5au, 0x47434241u, 0x5443485fu, 0x5f56315fu);      // "RCKZGCBATCH__V1_"
    if (q == 1u) return make_uint4(0u, (uint32_t)N_FE, 0u, (uint32_t)CELL_FE);
    return make_uint4(0u, m.u, 0u, m.n);
}
__device__ __forceinline__ void cp_block_words(uint32_t w[16], const CellMsg &m, uint32_t b) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = cp_quad(m, 4u * b + (uint32_t)q);
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
}
__device__ __forceinline__ void cp_store_digest(uint8_t *digests, int g, const uint32_t hs[8]) {
    uint4 *dst = reinterpret_cast<uint4 *>(digests + 32 * (size_t)g);  // big-endian bytes, as SHA-256 emits them
    dst[0] = make_uint4(bswap32(hs[0]), bswap32(hs[1]), bswap32(hs[2]), bswap32(hs[3]));
    dst[1] = make_uint4(bswap32(hs[4]), bswap32(hs[5]), bswap32(hs[6]), bswap32(hs[7]));
}

// Each hash kernel has one body and two entries: the uniform one (every group npg cells) and the `_sets` one (group g is cells goff[g] ..
// goff[g + 1] - 1: the groups of kzg355_verify_cell_kzg_proof_batch_many_sets_device, or whole blobs of different counts).  Message assembly, schedule and rounds are
// the body's and do not know which entry called.
// many groups: one lane per group, schedule and rounds in the lane's registers
__device__ __forceinline__ void cp_rhash_lanes_body(const CellMsg &m, int g, uint8_t *digests) {
    uint32_t hs[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll 1
    for (uint32_t b = 0; b < m.nblocks; b++) {
        uint32_t w[16];
        cp_block_words(w, m, b);
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = hs[i];
#pragma unroll
        for (int t = 0; t < 64; t++) {
            if (t >= 16) sha_schedule(w, t);
            sha_round(v, w[t & 15] + SHA_K[t]);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) hs[i] += v[i];
    }
    cp_store_digest(digests, g, hs);
}
__global__ void __launch_bounds__(64) k_cell_rhash_lanes(const uint8_t *uc, const uint64_t *indices, const uint8_t *cells, const uint8_t *proofs,
                                                         const int *cidx, const int *ucount, int npg, int groups, uint8_t *digests) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= groups) return;
    cp_rhash_lanes_body(cp_msg(uc, indices, cells, proofs, cidx, ucount, (size_t)g * npg, npg, g), g, digests);
}
// The lanes of a wave hash transcripts of DIFFERENT lengths here: each lane's loop runs over its own nblocks, a lane that is done is masked off,
// and the wave runs as long as its longest transcript.  That is correct (no lane reads past its own message, nothing is shared between lanes);
// it only means that a wave of mixed sizes is as slow as its largest group.
__global__ void __launch_bounds__(64) k_cell_rhash_lanes_sets(const uint8_t *uc, const uint64_t *indices, const uint8_t *cells, const uint8_t *proofs,
                                                              const int *cidx, const int *ucount, const int *goff, int groups, uint8_t *digests) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= groups) return;
    cp_rhash_lanes_body(cp_msg(uc, indices, cells, proofs, cidx, ucount, (size_t)goff[g], goff[g + 1] - goff[g], g), g, digests);
}

// few groups: one wave per group (four per workgroup, one per SIMD of its CU; the waves share nothing and synchronise with themselves only).
// The message schedule of a block does not depend on the chaining state: the 64 lanes expand 64 blocks at once (W[t] + K[t] to LDS), then lane 0
// runs the rounds of those blocks.
constexpr int CP_WAVES = 4;
// (the message m of the calling wave's group g; wave wid of its workgroup, lane of the wave)
__device__ __forceinline__ void cp_rhash_wave_body(const CellMsg &m, int g, int wid, int lane, uint8_t *digests) {
    __shared__ uint32_t wk_all[CP_WAVES][64][64];                 // per wave: [t][block of the chunk]
    uint32_t (*wk)[64] = wk_all[wid];
    uint32_t hs[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll 1
    for (uint32_t b0 = 0; b0 < m.nblocks; b0 += 64) {
        const uint32_t b = b0 + (uint32_t)lane;
        if (b < m.nblocks) {
            uint32_t w[16];
            cp_block_words(w, m, b);
#pragma unroll
            for (int t = 0; t < 64; t++) {
                if (t >= 16) sha_schedule(w, t);
                wk[t][lane] = w[t & 15] + SHA_K[t];
            }
        }
        SHA_WAVE_SYNC();
        if (lane == 0) {
            const uint32_t cnt = m.nblocks - b0 < 64u ? m.nblocks - b0 : 64u;
#pragma unroll 1
            for (uint32_t q = 0; q < cnt; q++) {
                uint32_t v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = hs[i];
#pragma unroll
                for (int t = 0; t < 64; t++) sha_round(v, wk[t][q]);
#pragma unroll
                for (int i = 0; i < 8; i++) hs[i] += v[i];
            }
        }
        SHA_WAVE_SYNC();
    }
    if (lane == 0) cp_store_digest(digests, g, hs);
}
__global__ void __launch_bounds__(64 * CP_WAVES) k_cell_rhash_wave(const uint8_t *uc, const uint64_t *indices, const uint8_t *cells, const uint8_t *proofs,
                                                                   const int *cidx, const int *ucount, int npg, int groups, uint8_t *digests) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * CP_WAVES + wid;
    if (g >= groups) return;
    cp_rhash_wave_body(cp_msg(uc, indices, cells, proofs, cidx, ucount, (size_t)g * npg, npg, g), g, wid, lane, digests);
}
// (a wave hashes one group, so the waves of a workgroup differ in length and share nothing but the LDS array's address)
__global__ void __launch_bounds__(64 * CP_WAVES) k_cell_rhash_wave_sets(const uint8_t *uc, const uint64_t *indices, const uint8_t *cells,
                                                                        const uint8_t *proofs, const int *cidx, const int *ucount, const int *goff,
                                                                        int groups, uint8_t *digests) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * CP_WAVES + wid;
    if (g >= groups) return;
    cp_rhash_wave_body(cp_msg(uc, indices, cells, proofs, cidx, ucount, (size_t)goff[g], goff[g + 1] - goff[g], g), g, wid, lane, digests);
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_cell_prep(const uint8_t *d_commitments, const size_t *d_indices, int npg, int groups, int tab_size, int *d_gtab, uint8_t *d_uc, int4 *d_segs,
                      int *d_gseg, int *d_cell, int *d_cidx, int *d_perm, int *d_ucount, int *d_err, hipStream_t st) {
    if (groups <= 0 || npg <= 0) return;
    static_assert(sizeof(size_t) == sizeof(uint64_t), "cell indices are 64-bit");
    const int seg_cap = npg < CELLS_PER_EXT_BLOB ? npg : CELLS_PER_EXT_BLOB;
    hipLaunchKernelGGL(k_cell_prep, dim3(groups), dim3(CP_THREADS), 0, st, d_commitments, reinterpret_cast<const uint64_t *>(d_indices), npg, groups, seg_cap,
                       tab_size, tab_size > CELL_PREP_LDS_SLOTS ? d_gtab : nullptr, d_uc, d_segs, d_gseg, d_cell, d_cidx, d_perm, d_ucount, d_err);
}
void launch_cell_prep_sets(const uint8_t *d_commitments, const size_t *d_indices, const int *d_goff, const int *d_gseg, int groups, int *d_gtab,
                           uint8_t *d_uc, int4 *d_segs, int *d_cell, int *d_cidx, int *d_perm, int *d_cgrp, int *d_ucount, int *d_err, hipStream_t st) {
    if (groups <= 0) return;
    hipLaunchKernelGGL(k_cell_prep_sets, dim3(groups), dim3(CP_THREADS), 0, st, d_commitments, reinterpret_cast<const uint64_t *>(d_indices), d_goff, d_gseg,
                       d_gtab, d_uc, d_segs, d_cell, d_cidx, d_perm, d_cgrp, d_ucount, d_err);
}
void launch_cell_rhash(const uint8_t *d_uc, const size_t *d_indices, const uint8_t *d_cells, const uint8_t *d_proofs, const int *d_cidx, const int *d_ucount,
                       int npg, int groups, bool lanes, uint8_t *d_digests, hipStream_t st) {
    if (groups <= 0 || npg <= 0) return;
    const uint64_t *idx = reinterpret_cast<const uint64_t *>(d_indices);
    if (lanes) hipLaunchKernelGGL(k_cell_rhash_lanes, dim3((groups + 63) / 64), dim3(64), 0, st, d_uc, idx, d_cells, d_proofs, d_cidx, d_ucount, npg, groups,
                                  d_digests);
    else hipLaunchKernelGGL(k_cell_rhash_wave, dim3((groups + CP_WAVES - 1) / CP_WAVES), dim3(64 * CP_WAVES), 0, st, d_uc, idx, d_cells, d_proofs, d_cidx,
                            d_ucount, npg, groups, d_digests);
}
void launch_cell_rhash_sets(const uint8_t *d_uc, const size_t *d_indices, const uint8_t *d_cells, const uint8_t *d_proofs, const int *d_cidx,
                            const int *d_ucount, const int *d_goff, int groups, bool lanes, uint8_t *d_digests, hipStream_t st) {
    if (groups <= 0) return;
    const uint64_t *idx = reinterpret_cast<const uint64_t *>(d_indices);
    if (lanes) hipLaunchKernelGGL(k_cell_rhash_lanes_sets, dim3((groups + 63) / 64), dim3(64), 0, st, d_uc, idx, d_cells, d_proofs, d_cidx, d_ucount, d_goff,
                                  groups, d_digests);
    else hipLaunchKernelGGL(k_cell_rhash_wave_sets, dim3((groups + CP_WAVES - 1) / CP_WAVES), dim3(64 * CP_WAVES), 0, st, d_uc, idx, d_cells, d_proofs,
                            d_cidx, d_ucount, d_goff, groups, d_digests);
}

}  // namespace kzg
