// cell_domain.h -- what the device code of the three EIP-7594 cell paths (k_cells.hip, k_cell_compute.hip, k_cell_recover.hip) shares about the
// extended domain <w>, w = 7^((r-1)/8192): bit reversals, powers of w, and the radix-2 Fr transforms.  Included after kernels.h.
#pragma once

namespace kzg {

// 7^((r-1)/8192) as eight words (fr_from_words)
#define FR_W8192_INIT {0xc78c8967u, 0x6fdd00bfu, 0x434906acu, 0x146b58bcu, 0x972e89edu, 0x2ccddea2u, 0x37b1da3du, 0x485d5127u}

// the BITS-bit bit reversal of j < 2^BITS (the comments' rev6, rev7, rev12)
template <int BITS> __device__ __forceinline__ uint32_t rev(uint32_t j) { return __brev(j) >> (32 - BITS); }

__device__ __forceinline__ void fr_store_words(uint32_t *dst, const Fr &a) {
    uint32_t w[8]; fr_to_words(w, a);
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i] = w[i];
}
// w^e for e < 8192 from the w4096 table
__device__ __forceinline__ Fr cell_wpow(const CellComputeConsts *cc, uint32_t e) {
    Fr v = cc->w4096[e >> 1];
    if (e & 1u) fr_mul(v, v, cc->w8192);
    return v;
}

// Radix-2 transforms of N values in LDS by T threads (tid < T, all of them call): per stage a thread takes the butterflies q = tid, tid + T, ...
// below N / 2, then the workgroup meets.  A butterfly reads and writes the same two slots, so that one barrier per stage is enough.
// wN^e = w4096^(e 4096 / N).
// forward (root wN): natural in, bit-reversed out
template <int N, int T> __device__ __forceinline__ void fr_dif(Fr *a, const CellComputeConsts *cc, int tid) {
    for (int h = N / 2; h >= 1; h >>= 1) {
        for (int q = tid; q < N / 2; q += T) {
            const int j = q % h, s = (q / h) * 2 * h, e = j * (N / 2 / h);
            const Fr u = a[s + j], v = a[s + j + h];
            Fr x, y; fr_add(x, u, v); fr_sub(y, u, v);
            if (e) fr_mul(y, y, cc->w4096[e * (N_FE / N)]);
            a[s + j] = x; a[s + j + h] = y;
        }
        __syncthreads();
    }
}
// inverse (root wN^-1, no 1/N): bit-reversed in, natural out
template <int N, int T> __device__ __forceinline__ void fr_dit_inv(Fr *a, const CellComputeConsts *cc, int tid) {
    for (int h = 1; h < N; h <<= 1) {
        for (int q = tid; q < N / 2; q += T) {
            const int j = q % h, s = (q / h) * 2 * h, e = j * (N / 2 / h);
            const Fr u = a[s + j];
            Fr v = a[s + j + h];
            if (e) fr_mul(v, v, cc->w4096[N_FE - e * (N_FE / N)]);
            Fr x, y; fr_add(x, u, v); fr_sub(y, u, v);
            a[s + j] = x; a[s + j + h] = y;
        }
        __syncthreads();
    }
}

}  // namespace kzg
