// k_point_eval.hip -- the front of the EIP-4844 point-evaluation precompile on the device (point_eval.hip): one lane per input hashes the
// commitment (one SHA-256 block), compares the versioned hash and re-packs the input into the 160-byte record verify_kzg_proof reads.
// The byte layout is point_eval.h's; here are the loads, the stores and the device rounds.  No LDS, no scratch, no atomics: everything an
// input needs lives in the registers of its lane, and all indices are constants once the loops are unrolled.
#include "kernels.h"
#include "point_eval.h"
#include "sha256_rounds.h"

namespace kzg {

// one compression on the round primitives of sha256_rounds.h, the rolling schedule in registers
struct PeDeviceCompress {
    __device__ __forceinline__ void operator()(Sha256 &s, uint32_t *w) const {
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = s.h[i];
#pragma unroll
        for (int t = 0; t < 64; t++) {
            if (t >= 16) sha_schedule(w, t);
            sha_round(v, w[t & 15] + SHA_K[t]);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) s.h[i] += v[i];
    }
};

// inputs: n * 192 bytes, 16-byte aligned (192 = 12 x 16: every input of an aligned array is aligned); records: n * 160 bytes, 16-byte aligned
__global__ void __launch_bounds__(64) k_pe_unpack(const uint4 *__restrict__ inputs, int n, uint4 *__restrict__ records, int *__restrict__ match) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint4 *src = inputs + (size_t)i * (PE_INPUT_WORDS / 4);
    uint32_t in[PE_INPUT_WORDS], rec[PE_RECORD_WORDS];
#pragma unroll
    for (int q = 0; q < PE_INPUT_WORDS / 4; q++) {
        const uint4 v = src[q];
        in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
    }
    const uint32_t m = pe_unpack(rec, in, PeDeviceCompress());
    uint4 *dst = records + (size_t)i * (PE_RECORD_WORDS / 4);
#pragma unroll
    for (int q = 0; q < PE_RECORD_WORDS / 4; q++) dst[q] = make_uint4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
    match[i] = (int)m;
}

// commitments: n * 48 bytes, 4-byte aligned; out: n * 32 bytes, 16-byte aligned
__global__ void __launch_bounds__(64) k_versioned_hash(const uint32_t *__restrict__ commitments, int n, uint4 *__restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t *src = commitments + (size_t)i * PE_POINT_WORDS;
    uint32_t c[PE_POINT_WORDS], vh[PE_HASH_WORDS];
#pragma unroll
    for (int k = 0; k < PE_POINT_WORDS; k++) c[k] = src[k];
    pe_versioned_hash(vh, c, PeDeviceCompress());
    out[2 * (size_t)i] = make_uint4(vh[0], vh[1], vh[2], vh[3]);
    out[2 * (size_t)i + 1] = make_uint4(vh[4], vh[5], vh[6], vh[7]);
}

void launch_pe_unpack(const uint8_t *d_inputs, int n, uint8_t *d_records, int *d_match, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pe_unpack, dim3((n + 63) / 64), dim3(64), 0, st, reinterpret_cast<const uint4 *>(d_inputs), n, reinterpret_cast<uint4 *>(d_records),
                       d_match);
}

void launch_versioned_hash(const uint8_t *d_commitments, int n, uint8_t *d_out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_versioned_hash, dim3((n + 63) / 64), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_commitments), n,
                       reinterpret_cast<uint4 *>(d_out));
}

}  // namespace kzg
