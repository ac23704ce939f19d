// point_eval.h -- the byte layout of the EIP-4844 point-evaluation precompile (address 0x0A), written once for host and device.
// An input is 192 bytes, versioned_hash[32] | z[32] | y[32] | commitment[48] | proof[48], and the precompile's first step binds the commitment
// to the hash: versioned_hash == 0x01 || SHA-256(commitment)[1:32], all 32 bytes compared, only the 48 bytes hashed, nothing validated.  What
// verify_kzg_proof then reads is the 160-byte record C | z | y | proof (kernels.h: RECORD_BYTES).  Every field starts on a 4-byte border, so
// the functions below work on the 32-bit words of the input as they lie in memory (little-endian loads); `compress` is one SHA-256
// compression on big-endian message words -- the device rounds of sha256_rounds.h in k_point_eval.hip, sha256_block of sha256.h on the host
// (kzg355_kzg_to_versioned_hash_many, tests/native/point_eval_probe.cpp).
#pragma once
#include <stdint.h>
#include "sha256.h"

namespace kzg {

constexpr int PE_INPUT_BYTES = 192, PE_INPUT_WORDS = PE_INPUT_BYTES / 4;       // KZG355_BYTES_PER_POINT_EVALUATION_INPUT
constexpr int PE_RECORD_WORDS = 160 / 4;                                        // RECORD_BYTES
constexpr int PE_HASH_WORDS = 8, PE_POINT_WORDS = 12, PE_FR_WORDS = 8;
// field offsets of the input and of the record, in words
constexpr int PE_IN_HASH = 0, PE_IN_Z = 8, PE_IN_Y = 16, PE_IN_C = 24, PE_IN_PROOF = 36;
constexpr int PE_REC_C = 0, PE_REC_Z = 12, PE_REC_Y = 20, PE_REC_PROOF = 28;
constexpr uint32_t PE_VERSION_KZG = 0x01;                                       // VERSIONED_HASH_VERSION_KZG

// vh = 0x01 || sha256(c)[1:32] as 8 memory-order words, from the 12 memory-order words of a commitment.  The message is one block: the 48
// bytes, 0x80, zeros, and the bit length 384 in the last word.
template <class Compress> KZG_HD void pe_versioned_hash(uint32_t vh[PE_HASH_WORDS], const uint32_t c[PE_POINT_WORDS], Compress &&compress) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < PE_POINT_WORDS; i++) w[i] = __builtin_bswap32(c[i]);
    w[12] = 0x80000000u; w[13] = 0; w[14] = 0; w[15] = 8 * 4 * PE_POINT_WORDS;
    Sha256 s;
    sha256_init(s);
    compress(s, w);
#pragma unroll
    for (int i = 0; i < PE_HASH_WORDS; i++) vh[i] = __builtin_bswap32(s.h[i]);
    vh[0] = (vh[0] & 0xffffff00u) | PE_VERSION_KZG;                             // byte 0 of the hash is the low byte of word 0
}

// One input (48 words as loaded) -> its record (40 words as stored); returns 1 when the input's versioned hash is that of its commitment.
template <class Compress> KZG_HD uint32_t pe_unpack(uint32_t rec[PE_RECORD_WORDS], const uint32_t in[PE_INPUT_WORDS], Compress &&compress) {
    uint32_t vh[PE_HASH_WORDS];
    pe_versioned_hash(vh, in + PE_IN_C, compress);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < PE_HASH_WORDS; i++) diff |= vh[i] ^ in[PE_IN_HASH + i];
#pragma unroll
    for (int i = 0; i < PE_POINT_WORDS; i++) { rec[PE_REC_C + i] = in[PE_IN_C + i]; rec[PE_REC_PROOF + i] = in[PE_IN_PROOF + i]; }
#pragma unroll
    for (int i = 0; i < PE_FR_WORDS; i++) { rec[PE_REC_Z + i] = in[PE_IN_Z + i]; rec[PE_REC_Y + i] = in[PE_IN_Y + i]; }
    return diff == 0 ? 1u : 0u;
}

// the host's compression (sha256.h; on the device the kernels pass the rounds of sha256_rounds.h)
struct PeHostCompress { void operator()(Sha256 &s, uint32_t *w) const { sha256_block(s, w); } };

}  // namespace kzg
