// sha256_rounds.h -- the device-only pieces of SHA-256 that the hand-scheduled hash kernels share (k_verify.hip: the blob path's challenge and
// transcript hashes; k_cell_prep.hip: the cell transcript): the round primitives on gfx950's v_alignbit / v_bitop3, the round constants in constant
// memory, and the wave-local LDS hand-over of the one-wave-per-message form.  sha256.h holds the portable host + device block function.
#pragma once
#include <stdint.h>

namespace kzg {

__device__ __forceinline__ uint32_t ror(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t ch3(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xca); }   // e ? f : g
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xe8); }

static __constant__ uint32_t SHA_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

// message schedule, in place in the rolling window: W[t] for t >= 16
__device__ __forceinline__ void sha_schedule(uint32_t w[16], int t) {
    const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
    const uint32_t s0 = xor3(ror(w15, 7), ror(w15, 18), w15 >> 3);
    const uint32_t s1 = xor3(ror(w2, 17), ror(w2, 19), w2 >> 10);
    w[t & 15] = w[t & 15] + s0 + w[(t + 9) & 15] + s1;
}
// one round on the working variables v = a .. h; wk = W[t] + K[t]
__device__ __forceinline__ void sha_round(uint32_t v[8], uint32_t wk) {
    const uint32_t t1 = v[7] + xor3(ror(v[4], 6), ror(v[4], 11), ror(v[4], 25)) + ch3(v[4], v[5], v[6]) + wk;
    const uint32_t t2 = xor3(ror(v[0], 2), ror(v[0], 13), ror(v[0], 22)) + maj3(v[0], v[1], v[2]);
    v[7] = v[6]; v[6] = v[5]; v[5] = v[4]; v[4] = v[3] + t1; v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = t1 + t2;
}

// The waves of a workgroup that share nothing: each hands its own LDS slice from all lanes to lane 0 and back behind wave-local fences.
#define SHA_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); \
                             __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

}  // namespace kzg
