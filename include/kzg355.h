/*
 * kzg355.h -- C ABI of libkzg355.so, the MI355X-native (HIP / gfx950) KZG-4844 engine.
 *
 * This is the drop-in boundary for the hot path of pawanjay176/kzg_rust: every entry point below
 * replaces one associated function of `pub struct Kzg` (reference src/kzg.rs:983-1079) -- i.e. it sits
 * one level ABOVE the 35 blst `extern "C"` symbols the reference binds today,
 * because per-field-op FFI is too fine-grained for a GPU.  Bytes in, bytes out: no blst limb layouts,
 * no torch types, plain pointers and sizes.  INTEGRATION.md shows the Rust `extern "C"` block and the
 * `impl Kzg` forwards a maintainer would add.
 *
 * Status codes mirror `enum Error` (src/kzg.rs:10-22).  The reference's tests only distinguish
 * Ok / Err (src/lib.rs:47-50), so Ok-vs-Err and the returned bytes / bool are exact; the particular
 * non-zero code is best effort.  Outputs are written only on KZG355_OK.
 *
 * Ownership: the caller owns every buffer; the library copies in and retains nothing after return.
 * kzg355_settings is created by a load function, destroyed by kzg355_free_trusted_setup, immutable in
 * between, and may be used from several host threads at once (each call takes a private workspace +
 * HIP stream from a pool inside the handle) -- the reference takes `&KzgSettings` everywhere.
 *
 * There is NO CPU fallback: every function fails with KZG355_NO_DEVICE if no HIP device is usable.
 */
#ifndef KZG355_H
#define KZG355_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZG355_BYTES_PER_FIELD_ELEMENT 32   /* src/consts.rs:5  */
#define KZG355_BYTES_PER_COMMITMENT 48      /* src/consts.rs:8  */
#define KZG355_BYTES_PER_PROOF 48           /* src/consts.rs:11 */
#define KZG355_FIELD_ELEMENTS_PER_BLOB 4096 /* src/consts.rs:13 */
#define KZG355_BYTES_PER_BLOB 131072        /* src/consts.rs:16 */
#define KZG355_BYTES_PER_G1 48              /* src/consts.rs:31 */
#define KZG355_BYTES_PER_G2 96              /* src/consts.rs:34 */
#define KZG355_NUM_G2_POINTS 65             /* src/consts.rs:37 */
#define KZG355_BYTES_PER_RECORD 160         /* C(48) | z(32) | y(32) | proof(48): one r-transcript record, utils.rs:454-463 */
/* EIP-7594 (PeerDAS) cells: 64 field elements of a blob's 2x Reed-Solomon extension */
#define KZG355_BYTES_PER_CELL 2048
#define KZG355_FIELD_ELEMENTS_PER_CELL 64
#define KZG355_CELLS_PER_EXT_BLOB 128

enum {
    KZG355_OK = 0,
    KZG355_BADARGS = 1,               /* Error::BadArgs            kzg.rs:13 */
    KZG355_INTERNAL = 2,              /* Error::InternalError      kzg.rs:15 */
    KZG355_INVALID_BYTES_LENGTH = 3,  /* Error::InvalidBytesLength kzg.rs:17 */
    KZG355_INVALID_HEX = 4,           /* Error::InvalidHexFormat   kzg.rs:19 */
    KZG355_INVALID_TRUSTED_SETUP = 5, /* Error::InvalidTrustedSetup kzg.rs:21 */
    KZG355_NO_DEVICE = 6,             /* no usable HIP device (no reference counterpart; there is no CPU fallback) */
    KZG355_NO_MEMORY = 7,             /* a device or pinned-host allocation failed (no reference counterpart) */
    KZG355_DEVICE_ERROR = 8           /* a HIP runtime / RCCL call failed on a device that exists: a launch, copy, stream or collective error (no reference counterpart) */
};

typedef struct kzg355_settings kzg355_settings; /* opaque; replaces `KzgSettings` (kzg.rs:28-40) */

/* ---- trusted setup ---------------------------------------------------------------------------- */
/* Kzg::load_trusted_setup (kzg.rs:1005 -> 45-78 -> 833-899).  g1: n1*48 bytes, g2: n2*96 bytes, compressed,
 * Lagrange form, file order.  n1 not in {4096} + {4, 8, .., 64} or n2 != 65 -> INVALID_TRUSTED_SETUP; bad point / monomial form -> BADARGS.
 * Builds the device-resident tables (roots of unity, bit-reversed G1 table and its per-window multiples,
 * Miller-loop line tables of the two G2 points the verify path uses).  The wide-window MSM table of commitments / proofs (every multiple
 * 1..2^(c-1) of 2^(c w) * g1[i] over 128 bits: 10.9 .. 143.5 GB, kzg355_options.msm_bits) is built by the FIRST commitment / proof call,
 * sized from the HBM free at that moment -- a handle that only verifies never allocates it; if the allocation fails, or with
 * KZG355_MSM=bucket, only the 15 MB 8-bit table is kept and commitments / proofs take the bucket path (same results).  Takes the defaults of
 * kzg355_options below with the KZG355_* environment overrides applied; kzg355_load_trusted_setup_ex is the explicit form. */
int kzg355_load_trusted_setup(const uint8_t *g1_bytes, size_t n1, const uint8_t *g2_bytes, size_t n2, kzg355_settings **out);
/* The same over several GPUs of one node: a full replica of the tables per device, and the host-buffer entry points below spread
 * their work over the devices INSIDE the call, invisibly to the caller (the reference has no notion of devices): independent
 * batches / blobs go to the devices in contiguous ranges with no exchange; a call with fewer batches than devices (one 512-blob
 * batch on 8 GPUs) cuts every batch into per-device blocks of blobs, runs stage 1 per block, exchanges the 160-byte records with
 * ONE all-gather (RCCL ncclAllGather over xGMI on a communicator set kept in the handle; peer copies if RCCL is not available,
 * the device list has duplicates, the blocks are ragged, or KZG355_EXCHANGE=peer) and runs stage 2 of each batch on one device.
 * kzg355_load_trusted_setup does the same when KZG355_DEVICES=0,1,... is set.  The *_device entry points (device pointers) and
 * kzg355_settings_device refer to the first device of the list. */
int kzg355_load_trusted_setup_devices(const uint8_t *g1_bytes, size_t n1, const uint8_t *g2_bytes, size_t n2, const int *devices, size_t n_devices,
                                      kzg355_settings **out);
/* Everything a deployment may want to pin when a handle is created.  kzg355_options_default fills in the defaults (and struct_size, which
 * lets a library newer than the caller's header keep its own defaults for fields the caller does not know); 0 means "default" for every
 * numeric field unless stated otherwise.  The dispatch thresholds default to multiples of the device's compute-unit count -- the
 * measured crossovers of the 256-CU MI355X scaled to the device at hand.  The KZG355_* environment variables named
 * below are TEST / EXPERIMENT overrides: only kzg355_load_trusted_setup, _devices and _file read them (through
 * kzg355_options_from_env, the library's one reader of the environment beside the KZG355_DEBUG* switches and KZG355_DEVICES, all in csrc/options.hip);
 * kzg355_load_trusted_setup_ex takes what it is given and reads no environment. */
typedef struct kzg355_options {
    size_t struct_size;        /* sizeof(kzg355_options) as the caller compiled it */
    int device;                /* device ordinal; -1: the calling thread's current device                                   KZG355_DEVICE */
    int msm_bits;              /* fixed-base MSM table (built on the first commitment / proof call): 0 = the widest form whose table fits half of
                                  the HBM free at that moment; 12 / 13 / 15 / 16 = 10.9 / 20.1 / 68.9 / 143.5 GB at 22 / 20 / 18 / 16 table rows
                                  per scalar; 8 = the 15 MB 8-bit bucket form only                                KZG355_MSM_BITS, KZG355_MSM=bucket */
    int msm_require_wide;      /* 1: failing to allocate / build the wide table fails the load (else: bucket form, noted on stderr)  KZG355_MSM=wide */
    int self_test;             /* 1 (default): known-answer self-test of the new handle (~10 ms); 0: skip                   KZG355_SELFTEST */
    int host_threads;          /* host worker threads of the handle (Fiat-Shamir hashing of small host-buffer calls, staging copies);
                                  0 = min(16, cpus the process may run on / 2)                                             KZG355_HOST_THREADS */
    int host_hash;             /* challenges of host-buffer verify / blob-proof calls hashed on the host: 0 by size, 1 always, -1 never  KZG355_HOST_HASH=auto|on|off */
    int host_hash_max_blobs;   /* ... up to this many blobs per call (0 = 4096: measured crossover, profiles/r03/host_hash_crossover_v4.txt)          KZG355_HOST_HASH_MAX */
    int host_sha;              /* host SHA-256 form: 0 SHA extensions when the CPU has them, 1 portable C, 2 SHA extensions      KZG355_HOST_SHA=portable|shani */
    int host_rhash;            /* batch challenge r of lone small calls hashed on the host (records copied back, ~60 us instead of a 0.33 ms
                                  device chain): 0 by size, -1 never                                                       KZG355_HOST_RHASH=off */
    int host_rhash_max_records;/* ... up to this many records per call (0 = 1024: one 512-blob batch is a 2.6 ms chain on the device)  KZG355_HOST_RHASH_MAX */
    int challenge_form;        /* device Fiat-Shamir kernel: 0 by size (two-wave form up to 2 workgroups per CU), 1 one wave, 2 two waves   KZG355_CHALLENGE=1w|2w */
    int lincomb_form;          /* batch linear combination: 0 by size, 1 per-term windows, 2 buckets, 3 pre-shifted,       KZG355_LINCOMB=window|bucket|preshift|bucket_halves
                                  5 buckets on the scalars' halves even where the validation could supply the quarters' points (A/B runs, tests) */
    int pairing_lane;          /* 1: one-lane pairing kernel (A/B and tests)                                               KZG355_PAIRING=lane */
    int pairing_two_wave_upto; /* batches per launch set up to which a pairing runs its two Miller loops on two waves; 0 = 1 per CU; -1 never  KZG355_PAIRING_2W_UPTO */
    int lc_chain_from;         /* batches from which the bucket form ends in one Horner chain per class; 0 = 4 per CU       KZG355_LC_CHAIN_FROM */
    int rhash_lanes_from;      /* batches from which the r-transcripts are hashed one lane per batch; 0 = 4 per CU          KZG355_RHASH_LANES_FROM */
    int beside_max_blobs;      /* blobs per launch set up to which the point kernels run on side streams; 0 = 64 per CU */
    int split_parts;           /* device-resident verify calls as this many overlapped launch sets (0 / 1: one set)         KZG355_SPLIT=parts[,streams] */
    int split_streams;         /* ... over this many streams (0 = 2) */
    int chunk_mb;              /* MiB of blobs per chunk of a streamed host-buffer call (0 = 1024)                          KZG355_CHUNK_MB */
    int chunks_in_flight;      /* workspaces such a call rotates over (0 = 3)                                               KZG355_CHUNKS_IN_FLIGHT */
    int staging_ring;          /* 1: stage caller memory through pinned slots instead of letting the runtime DMA from it    KZG355_STAGING=ring */
    int exchange;              /* handles over several devices: 0 RCCL all-gather when available, 1 peer copies, 2 RCCL or fail   KZG355_EXCHANGE=peer|rccl */
    int verify_only;           /* 1: the handle serves verification: no wide-window MSM table is built or kept in HBM (the verify path never reads it;
                                  commitments / proofs still work, through the 15 MB bucket form)                          KZG355_VERIFY_ONLY=1 */
    int msm_glv;               /* 0 (default): scalars are split k = a + b x^2 and the table spans 128 bits (half the memory per window width);
                                  -1: round 3's form, windows over all 256 bits (12 .. 15 bits: 23.6 / 42.9 / 81.6 / 154.6 GB)     KZG355_MSM_GLV=off */
    int msm_eager;             /* 1: build the table inside the load call instead of on first use                        KZG355_MSM_EAGER=1 */
    int pairing_hard12_from;   /* batches per launch set from which the hard part of the final exponentiation runs twelve lanes per check, five checks per
                                  wave (throughput) instead of one wave per check (latency); 0 = 16 per CU; -1 never                KZG355_PAIRING_HARD12_FROM */
    int submit_sets;           /* submit / collect: 0 by size (sets of <= 128 blobs per CU as 1, larger ones as 2); 1 = every submitted set on a stream of its
                                  own; 2 = two-stage pipeline: stage 1 of the submitted sets in order on one stream, stage 2 of a set on a second
                                  one, queued behind the NEXT set's Fiat-Shamir kernel                                   KZG355_SUBMIT=sets|pipeline */
    int host_hash_device_max_blobs; /* DEVICE-RESIDENT verify / blob-proof calls (the *_device entry points) of up to this many blobs copy their blobs back
                                  to the host (8 MiB = 0.16 ms per 64) and hash the challenges on the host threads instead of the 3.7 ms device
                                  chain: 0 = 1024 (measured crossover ~1500: profiles/r05/device_host_hash_crossover.txt), -1 never; host_hash = -1 turns it off as well                          KZG355_HOST_HASH_DEVICE_MAX */
    int quotient_form;         /* k_quotient_tree's leaves per lane as a power of two: 0 by size (2 below 512 blobs, else 4); 2 / 4 / 6 pin one (tuning knob
                                  and test hook)                                                                          KZG355_QUOTIENT_FORM */
    int miller_segments;       /* few batches: segments per Miller loop of the multi-wave pairing form, two waves each: 0 = 2; 1 .. 4   KZG355_MILLER_SEGMENTS */
    int force_multi;           /* test hook: a device list of ONE device still builds the multi-device handle (replica list, exchange)    KZG355_FORCE_MULTI=1 */
    int force_sharded;         /* test hook: a multi-device handle cuts EVERY batch into per-device blocks, whatever the batch count     KZG355_FORCE_SHARDED=1 */
} kzg355_options;
void kzg355_options_default(kzg355_options *options);
void kzg355_options_from_env(kzg355_options *options);     /* defaults, then the KZG355_* overrides listed above */
/* kzg355_load_trusted_setup with explicit options, on options->device or -- devices != NULL -- over the listed devices (as
 * kzg355_load_trusted_setup_devices).  options == NULL: all defaults.  Reads no environment variable. */
int kzg355_load_trusted_setup_ex(const uint8_t *g1_bytes, size_t n1, const uint8_t *g2_bytes, size_t n2, const int *devices, size_t n_devices,
                                 const kzg355_options *options, kzg355_settings **out);
/* Kzg::load_trusted_setup_file (kzg.rs:995 -> 906-979): "4096\n65\n" + hex lines. */
int kzg355_load_trusted_setup_file(const char *path, kzg355_settings **out);
/* Minimal preset helper: n compressed MONOMIAL points [tau^k]G1 (n a power of two in [4, 64], e.g. the first four `setup_G1`
 * entries of a ceremony JSON) -> the n compressed points of the size-n LAGRANGE setup, L_j = (1/n) sum_k w^(-jk) [tau^k]G1, in
 * file (natural) order, ready for kzg355_load_trusted_setup.  (src/trusted_setup.rs:144-151 truncates the 4096-point Lagrange
 * setup instead; that loads but is not a basis of the smaller domain.)  Bad point -> BADARGS. */
int kzg355_lagrange_setup_from_monomial(uint8_t *out /* n*48 */, const uint8_t *monomial_g1 /* n*48 */, size_t n);
/* Drop for KzgSettings. */
void kzg355_free_trusted_setup(kzg355_settings *s);

/* ---- the reference's seven operations, host buffers in / out ---------------------------------- */
/* Kzg::blob_to_kzg_commitment (kzg.rs:1013 -> 401-406). blob: 131072 bytes. */
int kzg355_blob_to_kzg_commitment(uint8_t out[48], const uint8_t *blob, const kzg355_settings *s);
/* Kzg::compute_kzg_proof (kzg.rs:1021 -> 446-457): returns proof and y = p(z). */
int kzg355_compute_kzg_proof(uint8_t proof_out[48], uint8_t y_out[32], const uint8_t *blob, const uint8_t z_bytes[32], const kzg355_settings *s);
/* Kzg::compute_blob_kzg_proof (kzg.rs:1030 -> 533-544). */
int kzg355_compute_blob_kzg_proof(uint8_t proof_out[48], const uint8_t *blob, const uint8_t commitment[48], const kzg355_settings *s);
/* Kzg::verify_kzg_proof (kzg.rs:1039 -> 429-443). */
int kzg355_verify_kzg_proof(bool *ok, const uint8_t commitment[48], const uint8_t z_bytes[32], const uint8_t y_bytes[32], const uint8_t proof[48], const kzg355_settings *s);
/* Kzg::verify_blob_kzg_proof (kzg.rs:1050 -> 547-569). */
int kzg355_verify_blob_kzg_proof(bool *ok, const uint8_t *blob, const uint8_t commitment[48], const uint8_t proof[48], const kzg355_settings *s);
/* Kzg::verify_blob_kzg_proof_batch (kzg.rs:1066 -> 637-693).  The Rust slices `&[Blob]`, `&[KzgCommitment]`,
 * `&[KzgProof]` carry their own lengths; the shim passes all three so that the reference's length check
 * (kzg.rs:644-651 -> BadArgs) is made on this side of the boundary too.  blobs: n_blobs*131072 contiguous bytes
 * (the shim gathers the `Box`ed blobs into one staging buffer).  n == 0 -> ok = true (kzg.rs:653-655). */
int kzg355_verify_blob_kzg_proof_batch(bool *ok, const uint8_t *blobs, size_t n_blobs, const uint8_t *commitments, size_t n_commitments,
                                       const uint8_t *proofs, size_t n_proofs, const kzg355_settings *s);

/* ---- throughput extensions (same semantics, many independent units per call) ------------------ */
/* n independent blob_to_kzg_commitment calls.  status[i] per blob (may be NULL); returns first non-OK status. */
int kzg355_blob_to_kzg_commitment_many(uint8_t *out /* n*48 */, int *status /* n or NULL */, const uint8_t *blobs, size_t n, const kzg355_settings *s);
/* n independent compute_blob_kzg_proof calls. */
int kzg355_compute_blob_kzg_proof_many(uint8_t *out /* n*48 */, int *status, const uint8_t *blobs, const uint8_t *commitments, size_t n, const kzg355_settings *s);
/* `groups` independent verify_blob_kzg_proof_batch calls of n_per_group blobs each, executed by ONE set of kernel
 * launches.  ok[g] / status[g] are per group.  Inputs are group-major contiguous. */
int kzg355_verify_blob_kzg_proof_batch_many(bool *ok /* groups */, int *status /* groups */, const uint8_t *blobs, const uint8_t *commitments,
                                            const uint8_t *proofs, size_t n_per_group, size_t groups, const kzg355_settings *s);

/* n independent verify_kzg_proof calls (kzg.rs:1039 -> 429-443; benches/kzg_benches.rs:70-81 times one per call): ok[i] / status[i] per check
 * (status may be NULL), the inputs of check i at commitments + 48 i, zs + 32 i, ys + 32 i, proofs + 48 i.  A bad point or a non-canonical z / y is
 * that check's KZG355_BADARGS; the others are unaffected.  Returns the first non-OK status.  One set of kernel launches per 2^17 checks: four
 * scalar-multiplication ladder lanes and twelve pairing lanes per check instead of a 1.9 ms latency-bound chain per call. */
int kzg355_verify_kzg_proof_many(bool *ok /* n */, int *status /* n or NULL */, const uint8_t *commitments /* n*48 */, const uint8_t *zs /* n*32 */,
                                 const uint8_t *ys /* n*32 */, const uint8_t *proofs /* n*48 */, size_t n, const kzg355_settings *s);
/* n independent verify_blob_kzg_proof calls (kzg.rs:1050 -> 547-569): = kzg355_verify_blob_kzg_proof_batch_many with one blob per batch (the
 * batch equation with r^0 = 1 is the single check, kzg.rs:658-660). */
int kzg355_verify_blob_kzg_proof_many(bool *ok /* n */, int *status /* n or NULL */, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs,
                                      size_t n, const kzg355_settings *s);
/* n independent compute_kzg_proof calls (kzg.rs:1021 -> 446-457): proof i and y_i = p_i(z_i) for blob i at the caller's point zs + 32 i.  A
 * non-canonical z_i or blob is that unit's KZG355_BADARGS; outputs of a unit are written only on its KZG355_OK. */
int kzg355_compute_kzg_proof_many(uint8_t *proofs_out /* n*48 */, uint8_t *ys_out /* n*32 */, int *status /* n or NULL */, const uint8_t *blobs,
                                  const uint8_t *zs /* n*32 */, size_t n, const kzg355_settings *s);

/* ---- the EIP-4844 point-evaluation precompile (address 0x0A), batched ---------------------------- */
/* The KZG question of the execution side.  Input i is KZG355_BYTES_PER_POINT_EVALUATION_INPUT bytes, versioned_hash[32] | z[32] | y[32] |
 * commitment[48] | proof[48]; with vh(C) = 0x01 || SHA-256(C)[1:32]:
 *   hash_match[i] = (versioned_hash == vh(commitment)) -- all 32 bytes compared (a wrong version byte is a mismatch), only the 48 bytes hashed,
 *   nothing validated at this step;
 *   no match: ok[i] = false, status[i] = KZG355_OK and NOTHING ELSE about that input is reported -- the precompile fails at the hash before it looks
 *   at the rest, so invalid point bytes or a non-canonical z behind a wrong hash are still KZG355_OK / false;
 *   match: ok[i] / status[i] are exactly what kzg355_verify_kzg_proof_many gives for (commitment, z, y, proof): a point that fails validate_kzg_g1
 *   or a non-canonical z or y is that input's KZG355_BADARGS with ok[i] = false, and the other inputs are unaffected.
 * Returns the first non-OK status in input order.  status may be NULL, hash_match may be NULL.  n == 0: KZG355_OK, nothing touched.
 * REFUSED AS A WHOLE, from the arguments alone, before any array is read or any device touched, every status marked and every ok / hash_match
 * false: a NULL handle, a NULL ok, a NULL inputs with n > 0, n above 2^24; for the device forms d_inputs or d_out not 16-byte aligned, or
 * d_commitments not 4-byte aligned.  (The two hash calls have no per-input arrays: they return KZG355_BADARGS and write nothing.)
 * Both _many forms run in launch sets of at most 2^17 inputs, whatever n is: per set one kernel hashes, compares and writes the 160-byte records
 * C | z | y | proof, then the records chain of kzg355_verify_kzg_proof_many checks them (inputs whose hash does not match run through it with
 * the others; its answer for them is dropped).  The host form stages the raw inputs of a set in pinned memory -- nothing is hashed or re-packed
 * on the host -- and follows kzg355_verify_kzg_proof_many on a handle over several devices: contiguous ranges of inputs per device when n is at
 * least the device count, else one device.  The device forms run on the handle's first device.  The caller's buffers are only read.  Every
 * handle is served, the minimal preset included (verify_kzg_proof does not depend on the blob size). */
#define KZG355_BYTES_PER_POINT_EVALUATION_INPUT 192
/* pure host, no handle, no device: out[32 i ..] = 0x01 || sha256(commitments[48 i ..])[1:] */
int kzg355_kzg_to_versioned_hash_many(uint8_t *out /* n*32 */, const uint8_t *commitments /* n*48 */, size_t n);
int kzg355_kzg_to_versioned_hash_many_device(uint8_t *d_out /* n*32 */, const uint8_t *d_commitments /* n*48 */, size_t n, const kzg355_settings *s);
int kzg355_point_evaluation_many(bool *ok, int *status /* or NULL */, bool *hash_match /* or NULL */, const uint8_t *inputs /* n*192 */, size_t n,
                                 const kzg355_settings *s);
int kzg355_point_evaluation_many_device(bool *ok /* host */, int *status /* host or NULL */, bool *hash_match /* host or NULL */,
                                        const uint8_t *d_inputs /* n*192, 16-byte aligned */, size_t n, const kzg355_settings *s);
/* one precompile call as the EIP words it.  KZG355_OK means success, and out = u256be(FIELD_ELEMENTS_PER_BLOB of the handle) | u256be(BLS_MODULUS).
 * input_len != 192, a hash mismatch, an invalid input or a false proof: KZG355_BADARGS, and out is not written. */
int kzg355_point_evaluation(uint8_t out[64], const uint8_t *input, size_t input_len, const kzg355_settings *s);

/* ---- device-resident inputs (what bench.py times: blobs already in HBM) ----------------------- */
/* As above, but d_* are DEVICE pointers (hipMalloc / torch tensors .data_ptr()) on the settings' device.
 * ok / status are host pointers.  Synchronous: returns when the verdicts are on the host. */
int kzg355_verify_blob_kzg_proof_batch_many_device(bool *ok, int *status, const uint8_t *d_blobs, const uint8_t *d_commitments,
                                                   const uint8_t *d_proofs, size_t n_per_group, size_t groups, const kzg355_settings *s);
/* The same call in two halves, for a caller that keeps several launch sets in flight from ONE host thread (a set of 1024 batches is 8.6 GB of
 * blobs; the synchronous call wants ~8192 batches = 69 GB per call to reach the same rate): _submit queues the whole set on a private stream of
 * the handle and returns at once with a ticket; kzg355_verify_collect waits for that set, writes ok[g] / status[g] (host, `groups` entries as
 * submitted) and CONSUMES the ticket, whatever it returns.  Stage 2 of a submitted set (r powers, linear combination, pairing) runs beside the
 * evaluation and point kernels of the set submitted after it; keep THREE sets in flight (submit k + 2 before collecting k) and 1024-batch sets
 * run at 4.0 M blobs/s against 3.4 M one at a time (profiles/r04/pipeline_sweep.txt).  Collect in any order; every ticket must be collected before the handle is freed; the
 * device buffers of a set must stay untouched until its collect returns.  Returns as the synchronous call (first non-OK status at collect). */
typedef struct kzg355_ticket kzg355_ticket;
int kzg355_verify_blob_kzg_proof_batch_many_device_submit(kzg355_ticket **ticket, const uint8_t *d_blobs, const uint8_t *d_commitments,
                                                          const uint8_t *d_proofs, size_t n_per_group, size_t groups, const kzg355_settings *s);
int kzg355_verify_collect(kzg355_ticket *ticket, bool *ok /* groups */, int *status /* groups or NULL */);
int kzg355_blob_to_kzg_commitment_many_device(uint8_t *out /* host n*48 */, int *status /* host n or NULL */, const uint8_t *d_blobs, size_t n,
                                              const kzg355_settings *s);
int kzg355_compute_blob_kzg_proof_many_device(uint8_t *out /* host n*48 */, int *status, const uint8_t *d_blobs, const uint8_t *d_commitments,
                                              size_t n, const kzg355_settings *s);

/* The *_many forms of the single-proof functions on device memory: d_records = n records C_i | z_i | y_i | proof_i of KZG355_BYTES_PER_RECORD bytes
 * (16-byte aligned; = kzg355_verify_records_checked_device with one record per batch); d_blobs / d_zs as the host forms lay them out.  (n independent
 * verify_blob_kzg_proof checks on device memory are kzg355_verify_blob_kzg_proof_batch_many_device with n_per_group = 1.) */
int kzg355_verify_kzg_proof_many_device(bool *ok /* host n */, int *status /* host n or NULL */, const uint8_t *d_records, size_t n, const kzg355_settings *s);
int kzg355_compute_kzg_proof_many_device(uint8_t *proofs_out /* host n*48 */, uint8_t *ys_out /* host n*32 */, int *status, const uint8_t *d_blobs,
                                         const uint8_t *d_zs /* n*32 */, size_t n, const kzg355_settings *s);

/* ---- verify_blob_kzg_proof_batch on batches of different blob counts in one call ---------------- */
/* A block brings 0..9 blobs, a blob transaction 1..6: `groups` batches, batch g being the next blob_counts[g] blobs / commitments / proofs of
 * the three arrays, which hold the batches one after the other with no padding.  Per batch EXACTLY what kzg355_verify_blob_kzg_proof_batch
 * returns on that slice: its own transcript (with its own n), challenge r, pairing, verdict and status; a count of 1 takes r^0 = 1 with no
 * hash; a count of 0 is true / KZG355_OK (kzg.rs:653-655).  A blob element >= r, or a commitment or proof that fails validate_kzg_g1, is that
 * batch's KZG355_BADARGS with ok[g] = false; the other batches are untouched.  Returns the first non-OK status in batch order.
 * REFUSED AS A WHOLE, from the counts alone, before any array is read or any device touched, every status marked and every verdict false: a
 * NULL handle, ok or (groups > 0) blob_counts; a NULL array while the sum of the counts is > 0; groups or the sum above 2^24 (or a sum that
 * overflows); for the device form d_blobs not 16-byte aligned or a point array not 4-byte aligned.  groups == 0: KZG355_OK, nothing touched.
 * Work and device memory follow the SUM of the counts.  The non-empty batches run in launch sets of whole batches, taken in order while a set
 * stays within 32768 blobs (kzg355_settings_set_blob_sets_max_blobs, below, sets another limit); a batch
 * is never cut, and a batch larger than the limit is a set of its own.  The host form stages the blobs set by set (a set of at most
 * chunk_mb of blobs, chunks_in_flight sets on the device at a time).  A handle over D devices (host form): contiguous ranges of batches,
 * balanced by BLOBS -- range d ends at the batch border nearest to d N / D on the prefix sums of the counts (N their sum; the lower border of
 * two equally near); kzg355_settings_blob_sets_blobs_per_device tells how many blobs each device has run.  The device form expects its arrays
 * on the handle's first device and runs there.  The minimal preset is served too. */
int kzg355_verify_blob_kzg_proof_batch_many_sets(bool *ok /* groups */, int *status /* groups or NULL */, const size_t *blob_counts /* groups */,
                                                 const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs /* sum of the counts, batch after batch */,
                                                 size_t groups, const kzg355_settings *s);
int kzg355_verify_blob_kzg_proof_batch_many_sets_device(bool *ok /* host */, int *status /* host or NULL */, const size_t *blob_counts /* HOST */,
                                                        const uint8_t *d_blobs, const uint8_t *d_commitments, const uint8_t *d_proofs, size_t groups,
                                                        const kzg355_settings *s);
/* test / audit forms: out[128 g ..] = r | proof_lincomb | rhs as kzg355_debug_batch_intermediates lays them out (r reads 1 for a count of 1);
 * zero bytes for a count of 0.  A NULL out refuses the call. */
int kzg355_debug_batch_intermediates_sets(uint8_t *out /* groups*128 */, bool *ok, int *status, const size_t *blob_counts, const uint8_t *blobs,
                                          const uint8_t *commitments, const uint8_t *proofs, size_t groups, const kzg355_settings *s);
int kzg355_debug_batch_intermediates_sets_device(uint8_t *out /* host, groups*128 */, bool *ok, int *status, const size_t *blob_counts,
                                                 const uint8_t *d_blobs, const uint8_t *d_commitments, const uint8_t *d_proofs, size_t groups,
                                                 const kzg355_settings *s);
/* Tuning knob and test hook: the blobs per launch set of the four calls above, on the handle and every replica of it; 1 .. 2^24, 0 = the default
 * 32768, anything else KZG355_BADARGS.  Call it while no such call is running on the handle. */
int kzg355_settings_set_blob_sets_max_blobs(kzg355_settings *s, size_t max_blobs);
/* introspection for tests: returns the device count and fills out[d] (up to cap) with the blobs device d has run through the four calls above */
int kzg355_settings_blob_sets_blobs_per_device(const kzg355_settings *s, long *out /* cap */, size_t cap);

/* ---- sharded verification (one process per GPU; the exchange between the two stages is the caller's
 *      exchange of the 160-byte records, e.g. torch.distributed over RCCL) --------------------------- */
/* Stage 1, per rank, over its contiguous shard of every batch: `groups` batches, n_local blobs of each (group-major:
 * blob (g, i) at index g*n_local + i).  Validates C_i / proof_i, blob -> field elements, Fiat-Shamir challenge z_i
 * (kzg.rs:298-339), y_i = p_i(z_i) (kzg.rs:346-389).  Writes the records C_i|z_i|y_i|proof_i -- byte for byte the body of
 * the r-transcript (utils.rs:454-463) -- to d_records (device, same indexing), and per-batch status (KZG355_OK or
 * KZG355_BADARGS) to status[g] (host).  Returns the first non-OK status.  Device pointers: d_blobs and d_records 16-byte aligned
 * (hipMalloc and torch allocations are), else KZG355_BADARGS. */
int kzg355_verify_shard_records_device(uint8_t *d_records /* groups*n_local*160, device */, int *status /* groups, host */,
                                       const uint8_t *d_blobs, const uint8_t *d_commitments, const uint8_t *d_proofs, size_t n_local,
                                       size_t groups, const kzg355_settings *s);
/* Stage 2 over gathered records (device; every rank its share of the batches, or replicated): `groups` batches of n records each
 * (group-major).  r-powers (utils.rs:426-474), the three linear combinations and the pairing check (kzg.rs:579-627).
 * n == 1 reproduces the single-blob path (kzg.rs:658); n == 0 is an error like kzg.rs:588-592. */
/* The same two stages with the decoded points travelling next to the records: stage 1 also writes the validated affine points of its
 * shard (d_points: groups x [n_local commitments, n_local proofs] x KZG355_BYTES_PER_POINT opaque bytes), and stage 2 takes the points
 * of the gathered batches (groups x [n commitments, n proofs]) instead of decompressing C_i / proof_i again (a 381-bit square root
 * per point).  The caller exchanges both buffers (kzg_rust_amd/sharded.py: one all-to-all, every rank receives the batches of its share). */
#define KZG355_BYTES_PER_POINT 112
int kzg355_verify_shard_records_points_device(uint8_t *d_records, uint8_t *d_points, int *status, const uint8_t *d_blobs, const uint8_t *d_commitments,
                                              const uint8_t *d_proofs, size_t n_local, size_t groups, const kzg355_settings *s);
int kzg355_verify_records_points_device(bool *ok, int *status, const uint8_t *d_records, const uint8_t *d_points, size_t n, size_t groups,
                                        const kzg355_settings *s);
/* The same two calls with the per-batch results left ON THE DEVICE (int32 words, device memory, 4-byte aligned), for a caller that merges them
 * across ranks with a collective and reads them back once (kzg_rust_amd/sharded.py): stage 1 writes d_status_words[g] = the KZG355 status of
 * batch g on this rank's shard; stage 2 writes d_words[g] = 1 + ok + 256 * status.  Both return after their stream has been synchronised (the
 * words may be read from any stream), and return only whole-call failures (KZG355_BADARGS for bad pointers, device errors). */
int kzg355_verify_shard_records_points_words_device(uint8_t *d_records, uint8_t *d_points, int32_t *d_status_words, const uint8_t *d_blobs,
                                                    const uint8_t *d_commitments, const uint8_t *d_proofs, size_t n_local, size_t groups, const kzg355_settings *s);
int kzg355_verify_records_points_words_device(int32_t *d_words, const uint8_t *d_records, const uint8_t *d_points, size_t n, size_t groups,
                                              const kzg355_settings *s);
/* PRECONDITION: the records come from kzg355_verify_shard_records_device (here or on another rank) and every rank's stage-1
 * status has been merged into the verdict by the caller (kzg_rust_amd/sharded.py does): this entry point decompresses C_i and
 * proof_i WITHOUT the subgroup test and does not re-check that z_i, y_i are canonical -- stage 1 already did both.  A caller
 * holding records of unknown origin must use kzg355_verify_records_checked_device instead. */
int kzg355_verify_records_device(bool *ok /* groups */, int *status /* groups */, const uint8_t *d_records /* groups*n*160, device */,
                                 size_t n, size_t groups, const kzg355_settings *s);
/* The same stage 2 with full input validation: validate_kzg_g1 (utils.rs:282-310, incl. subgroup) on every C_i / proof_i and
 * bytes_to_bls_field (utils.rs:262-275) on every z_i / y_i; = verify_kzg_proof_batch (kzg.rs:579-627) on untrusted bytes. */
int kzg355_verify_records_checked_device(bool *ok /* groups */, int *status /* groups */, const uint8_t *d_records, size_t n, size_t groups,
                                         const kzg355_settings *s);
/* Test / audit readback of the stage-2 intermediates of `groups` batches of n records: out[128 g ..] = r (32 bytes big-endian, the
 * Fiat-Shamir batch challenge of utils.rs:426-474) | proof_lincomb (48, kzg.rs:601) | rhs (48, kzg.rs:618-622), the two points
 * ZCash-compressed.  For n == 1 the r field reads 1 (r^0: the single-blob path takes no challenge).  Also returns the verdicts.
 * Not on the hot path; tests/test_gpu_parity.py diffs these against the oracle and the committed n = 64 / 512 fixtures. */
int kzg355_debug_batch_intermediates(uint8_t *out /* groups*128, host */, bool *ok /* groups */, int *status /* groups or NULL */,
                                     const uint8_t *d_records /* device */, size_t n, size_t groups, const kzg355_settings *s);

/* ---- introspection ---------------------------------------------------------------------------- */
/* Device ordinal the handle lives on, and average duration in milliseconds of the most recent launch of a named
 * kernel family on that handle ("verify_eval", "msm_bucket", ...), measured with HIP events on the launch stream;
 * returns a negative number if that kernel has not run.  Used by bench.py for the roofline line. */
int kzg355_settings_device(const kzg355_settings *s);
/* Number of devices the handle spans (1 for a plain handle). */
int kzg355_settings_device_count(const kzg355_settings *s);
/* Multi-device handles: how many record exchanges ran as an RCCL all-gather / as peer copies so far.  Returns the exchange the
 * handle is set up for (1 RCCL, 0 peer copies; -1 for a plain handle). */
int kzg355_settings_exchange_stats(const kzg355_settings *s, long *allgathers, long *peer_exchanges);
/* FIELD_ELEMENTS_PER_BLOB of the handle (consts.rs:13 is a compile-time 4096; the reference's README also names a minimal preset
 * with 4).  It is fixed by the number of G1 points given to the load function: 4096 -> the mainnet kernels; a power of two in
 * [4, 64] -> the small-domain path (one lane per blob, naive lincomb as utils.rs:369-371 takes below 8 points).  Every `blob`
 * argument of this header is 32 * FIELD_ELEMENTS_PER_BLOB bytes for the handle it is passed with. */
int kzg355_settings_field_elements_per_blob(const kzg355_settings *s);
/* Which MSM form commitments / proofs take on this handle: 10 .. 16 = wide-window table of that digit width; 8 = the 8-bit
 * bucket form because msm_bits = 8 / verify_only / KZG355_MSM=bucket asked for it; -8 = the bucket form because the wide table could NOT be
 * allocated or built (also reported once on stderr; msm_require_wide / KZG355_MSM=wide makes that an error instead).  Before the table
 * exists (it is built by the first commitment / proof call unless msm_eager): the width asked for, 0 = to be sized from the free HBM. */
int kzg355_settings_msm_form(const kzg355_settings *s);
/* The table as built: digit width, windows per (half-)scalar, 1 if the scalars are GLV-split, bytes of HBM; all 0 while it does not exist.
 * Any pointer may be NULL. */
int kzg355_settings_msm_shape(const kzg355_settings *s, int *bits, int *windows, int *glv, size_t *table_bytes);
/* Build the table now (every device of the handle) instead of inside the first commitment / proof call.  OK if it exists afterwards or
 * the handle is set to the bucket form. */
int kzg355_settings_build_msm_table(const kzg355_settings *s);
double kzg355_last_kernel_ms(const kzg355_settings *s, const char *kernel_family);
/* Accumulated HIP-event time and launch count of a kernel family since timing was enabled / last reset. 0 on success. */
int kzg355_kernel_ms_stats(const kzg355_settings *s, const char *kernel_family, double *total_ms, long *launches);
void kzg355_reset_kernel_stats(kzg355_settings *s);
/* Enable (1) / disable (0) per-kernel HIP-event timing on the handle (off by default: it adds event records). */
void kzg355_set_kernel_timing(kzg355_settings *s, int enabled);
const char *kzg355_version(void);

/* ---- host-side Fiat-Shamir hashing ------------------------------------------------ */
/* compute_challenge (kzg.rs:298-339) hashes 131,152 bytes per blob: on the device a 3.7 ms dependent chain for a small call, on a
 * host core with the SHA extensions ~60 us.  Host-buffer verify / blob-proof calls of at most `max_blobs` blobs (one chunk) therefore
 * hash their transcripts on the handle's host threads WHILE the H2D copy and the point kernels run and upload 32-byte digests; larger
 * and device-resident calls keep the device kernels.  mode: 0 by size (default), 1 always, -1 never (the batch challenge r of lone small
 * calls -- kzg355_options.host_rhash -- follows the same mode: -1 keeps every hash on the device); max_blobs 0 keeps the current
 * crossover (default 4096; KZG355_HOST_HASH=auto|on|off and KZG355_HOST_HASH_MAX in the environment set the same at load). */
int kzg355_settings_set_host_hash(kzg355_settings *s, int mode, int max_blobs);
/* How many host-buffer calls on this handle had their challenges hashed on the host so far. */
long kzg355_settings_host_hashed_calls(const kzg355_settings *s);
/* Host threads that hash for one call on this handle: the handle's workers plus the calling thread (kzg355_options.host_threads; the default is
 * min(16, cpus / 2)).  A CPU figure quoted next to a host-hashed call should use as many threads (bench.py: cpu_baseline.threads_matched_value). */
int kzg355_settings_host_threads(const kzg355_settings *s);
/* The host hash itself, exported for the tests (tests/test_host_sha256.py checks it against hashlib): impl 0 auto, 1 portable C,
 * 2 SHA extensions (KZG355_INTERNAL if the CPU has none).  kzg355_host_challenge_digests writes the n digests of
 * "FSBLOBVERIFY_V1_" | u64be(0) | u64be(blob_bytes / 32) | blob_i | commitment_i. */
/* Test / audit form of kzg355_verify_blob_kzg_proof_batch_many for calls of at most 64 MiB of blobs on a single-device handle: also
 * returns the stage-1 records C_i | z_i | y_i | proof_i of every blob (the body of the r-transcript, utils.rs:454-463), so that the z_i
 * of the host-hashed and the device-hashed route can each be diffed against the oracle (tests/test_gpu_host_hash.py). */
int kzg355_debug_verify_host_records(uint8_t *records_out /* groups*n_per_group*160, host */, bool *ok /* groups */, int *status /* groups or NULL */,
                                     const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs, size_t n_per_group, size_t groups,
                                     const kzg355_settings *s);
/* Test / audit form of the SHARDED execution of kzg355_verify_blob_kzg_proof_batch_many on a handle over several devices (BASELINE config 5: one
 * 512-blob batch cut into per-device blocks): every batch goes through stage 1 per block -> the record exchange -> stage 2 on one
 * device, whatever the batch count, and out[128 g ..] receives r | proof_lincomb | rhs of batch g as kzg355_debug_batch_intermediates lays them
 * out.  n_per_group >= the handle's device count; plain handles -> KZG355_BADARGS.  tests/test_gpu_multi_device.py diffs these against
 * tests/golden/batch512.json. */
int kzg355_debug_verify_sharded_intermediates(uint8_t *out /* groups*128, host */, bool *ok /* groups */, int *status /* groups or NULL */,
                                              const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs, size_t n_per_group, size_t groups,
                                              const kzg355_settings *s);
/* ---- EIP-7594 cell proofs ---------------------------------------------------------------------------------------------------------------------
 * verify_cell_kzg_proof_batch of the consensus specs (fulu/polynomial-commitments-sampling.md; c-kzg-4844 2.x): n cells, each with its commitment
 * (48 bytes), cell index (< 128), cell (2048 bytes: 64 big-endian field elements) and proof (48 bytes).  n == 0 -> true.  A cell index >= 128, a
 * commitment or proof that fails validate_kzg_g1 or a cell element >= r -> KZG355_BADARGS.  The challenge r hashes the domain
 * "RCKZGCBATCH__V1_", u64be(4096), u64be(64), u64be(#unique commitments), u64be(n), the unique commitments (first-appearance order), then per cell
 * u64be(commitment position), u64be(cell index), cell, proof -- on host threads; everything else runs on the device.  Mainnet handles only (a
 * handle of another FIELD_ELEMENTS_PER_BLOB -> KZG355_BADARGS).  The first cell call of a handle derives what the check needs from the setup
 * (the 64 monomial points [tau^t]_1 and the lines of setup g2[64]).
 *
 * A handle over several devices runs the host-buffer cell calls (verify, compute, recover: every call of this section but the debug readbacks of
 * the setup) on all of them, inside the library.  Independent units -- groups for verify, blobs for compute and recover -- go to the devices in
 * contiguous ranges, each device running the single-device call on its range from its own host thread; a call uses as many devices as it has
 * units.  A verify call with fewer groups than devices D and n_per_group >= 2 D cuts every group into D contiguous blocks of cells instead: the
 * check is linear in the cells once r is known, so each device reduces its block to three G1 points per group, those go to one device per group
 * (peer copies), and that device adds them and runs the pairing.  Results are byte for byte those of a single-device handle.  What refuses a call
 * as a whole is decided once, before any device is used; per-unit statuses keep their positions and the return value stays the first non-OK
 * status in unit order.  Every device builds its own cell setup on its first use.  The caller's current device is left as it was. */
int kzg355_verify_cell_kzg_proof_batch(bool *ok, const uint8_t *commitments /* n*48 */, const size_t *cell_indices /* n */, const uint8_t *cells /* n*2048 */,
                                       const uint8_t *proofs /* n*48 */, size_t n, const kzg355_settings *s);
/* `groups` independent calls of the above in one set of launches (one verdict per data-column sidecar): the four arrays group-major, n_per_group
 * cells each.  ok[g] / status[g] per group; the return value is the first non-OK status.  A refusal of the call as a whole marks every group. */
int kzg355_verify_cell_kzg_proof_batch_many(bool *ok /* groups */, int *status /* groups or NULL */, const uint8_t *commitments, const size_t *cell_indices,
                                            const uint8_t *cells, const uint8_t *proofs, size_t n_per_group, size_t groups, const kzg355_settings *s);
/* Test form of the _many call: out[176 g ..] receives r (32 bytes, big-endian) | [I(tau)]_1 | LL | RL (48 bytes each, compressed) of group g. */
int kzg355_debug_cell_batch_intermediates(uint8_t *out /* groups*176 */, bool *ok /* groups */, int *status /* groups or NULL */, const uint8_t *commitments,
                                          const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs, size_t n_per_group, size_t groups,
                                          const kzg355_settings *s);
/* Groups of DIFFERENT sizes in one call, one set of launches for all non-empty groups (the data-column sidecars of many blocks: a sidecar has one
 * cell per blob of its block).  Layout: with off_g = cell_counts[0] + ... + cell_counts[g-1], group g is entries [off_g, off_g + cell_counts[g]) of
 * the four arrays, which hold sum of the counts entries each, group after group.
 * Result per group: EXACTLY that of kzg355_verify_cell_kzg_proof_batch on that slice -- the same verdict, status and challenge r; commitments
 * deduplicated inside the group only, in order of first appearance; the transcript carries the group's own n.  A count of 0: that group is true /
 * KZG355_OK.  A cell index >= 128, a cell element >= r, a commitment or proof that fails validate_kzg_g1: that group's KZG355_BADARGS, the others
 * are left alone; the return value is the first non-OK status in group order.
 * Refused as a whole (every status marked, every verdict false), decided before any array is read and before any device is touched: a NULL
 * handle, NULL ok, or NULL cell_counts with groups > 0; a NULL array while the sum of the counts is > 0; a handle of another
 * FIELD_ELEMENTS_PER_BLOB; groups above 2^24; a sum of the counts that overflows size_t or exceeds 2^18 (the uniform form's limit on
 * n_per_group * groups).  groups == 0: KZG355_OK, nothing is touched.
 * Work and device memory are proportional to the sum of the counts (a group of n cells costs its own 3 n + 64 scalar multiplications), not to
 * groups times the largest.
 * A handle over several devices: the non-empty groups go to the devices in contiguous ranges, equal in GROUPS -- so the ranges can be uneven in
 * cells (not measured on several cards).  A group of this call is never cut into blocks, and kzg355_options.force_sharded does not apply to it.
 * kzg355_settings_cell_calls_per_device counts one launch set per device that received a non-empty group.
 * The device-resident form of this call is kzg355_verify_cell_kzg_proof_batch_many_sets_device, below.  Not offered: cutting a group of this
 * call over several devices.  (Per-transaction blob counts for kzg355_verify_blob_cell_proofs_batch_many are offered: its _many_sets form
 * below runs this call's chain with ragged forms of its own kernels.) */
int kzg355_verify_cell_kzg_proof_batch_many_sets(bool *ok /* groups */, int *status /* groups or NULL */, const size_t *cell_counts /* groups */,
                                                 const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells,
                                                 const uint8_t *proofs /* each: sum of the counts entries, group after group */, size_t groups,
                                                 const kzg355_settings *s);
/* Test form of the _many_sets call: out[176 g ..] as kzg355_debug_cell_batch_intermediates lays it out; zero bytes for a group of count 0. */
int kzg355_debug_cell_batch_intermediates_sets(uint8_t *out /* groups*176 */, bool *ok, int *status, const size_t *cell_counts, const uint8_t *commitments,
                                               const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs, size_t groups,
                                               const kzg355_settings *s);
/* The 64 monomial points [tau^t]_1 (t < 64) the handle derived from its Lagrange setup, compressed (building them first if no cell call has). */
int kzg355_debug_cell_setup_monomial(uint8_t *out /* 64*48 */, const kzg355_settings *s);
/* compute_cells_and_kzg_proofs of the consensus specs: the 128 cells of the blob's 2x extension (cells 0..63 are the blob itself) and their
 * 128 proofs (FK20), in cell order.  Either output may be NULL (then that half is not computed; without proofs_out no proof setup is built),
 * not both (KZG355_BADARGS).  A blob element >= r -> KZG355_BADARGS.  Mainnet handles only; a handle over several devices spreads the blobs of a
 * call over them (above; one blob is never cut).  The first call that wants proofs derives the 4096 monomial points [tau^t]_1 and a fixed-base
 * table (384 MiB) from the setup, on every device that gets a blob. */
int kzg355_compute_cells_and_kzg_proofs(uint8_t *cells_out /* 128*2048 or NULL */, uint8_t *proofs_out /* 128*48 or NULL */, const uint8_t *blob,
                                        const kzg355_settings *s);
/* n independent calls of the above (blobs n*131072 bytes): status[i] per blob; the return value is the first non-OK status.  n == 0 -> OK.  A
 * refusal of the call as a whole marks every blob.  Large n runs in chunks inside the call. */
int kzg355_compute_cells_and_kzg_proofs_many(uint8_t *cells_out /* n*128*2048 or NULL */, uint8_t *proofs_out /* n*128*48 or NULL */,
                                             int *status /* n or NULL */, const uint8_t *blobs, size_t n, const kzg355_settings *s);
/* recover_cells_and_kzg_proofs of the consensus specs: from n known cells of a blob's 2x extension (64 <= n <= 128; cell_indices strictly
 * ascending and < 128, cells in the same order) all 128 cells and all 128 proofs, exactly what kzg355_compute_cells_and_kzg_proofs returns for
 * the blob.  n outside 64..128, an index >= 128, indices not strictly ascending (so: any duplicate) or a cell element >= r -> KZG355_BADARGS.
 * Either output may be NULL, with the meaning it has there; not both.  More than 64 cells that lie on no polynomial of degree < 4096 are no
 * error, as in the specs and in c-kzg-4844: the result is the cells and proofs of the 4096 coefficients the specs' algorithm keeps.  Mainnet
 * handles only; a handle over several devices spreads the blobs of a call over them (above). */
int kzg355_recover_cells_and_kzg_proofs(uint8_t *cells_out /* 128*2048 or NULL */, uint8_t *proofs_out /* 128*48 or NULL */,
                                        const size_t *cell_indices /* n */, const uint8_t *cells /* n*2048 */, size_t n, const kzg355_settings *s);
/* m blobs known at the SAME n cell indices (a node holds the same columns of every blob of a block) in one set of launches: cells holds blob
 * after blob, n cells each.  status[i] per blob; the return value is the first non-OK status.  m == 0 -> OK.  A refusal of the call as a whole
 * marks every blob.  Large m runs in chunks inside the call. */
int kzg355_recover_cells_and_kzg_proofs_many(uint8_t *cells_out /* m*128*2048 or NULL */, uint8_t *proofs_out /* m*128*48 or NULL */,
                                             int *status /* m or NULL */, const size_t *cell_indices /* n, shared by all blobs */,
                                             const uint8_t *cells /* m*n*2048: blob after blob */, size_t n, size_t m, const kzg355_settings *s);
/* m independent recover_cells_and_kzg_proofs calls in one set of launches: blob i is known at cell_counts[i] cells; with
 * off_i = cell_counts[0] + .. + cell_counts[i-1], its indices are cell_indices[off_i .. off_i + cell_counts[i]) and its cells
 * cells + 2048 * off_i, in the same order.  Outputs as kzg355_recover_cells_and_kzg_proofs_many (either may be NULL, not both).
 * The result is exactly that of m single calls (a node that catches up recovers many blocks, each with its own columns).  What is wrong with
 * one blob is that blob's KZG355_BADARGS: a count outside 64..128 (0 included), an index >= 128, indices not strictly ascending, a cell element
 * >= r.  The other blobs are computed and are right: the layout always follows the counts as given.  The return value is the first non-OK
 * status; the output slots of a refused blob are unspecified.  What is wrong with the call refuses it as a whole and marks every status: a NULL
 * handle, both outputs NULL, NULL cell_counts, cell_indices or cells with m > 0, a handle of another FIELD_ELEMENTS_PER_BLOB, m > 2^32, a sum of
 * the counts that overflows size_t (or does so times 2048).  m == 0 -> OK, and nothing is touched.  More than 64 cells of a blob that lie on no
 * polynomial of degree < 4096 are no error: that blob's result is the single call's.  Blobs known at the same index set share its tables
 * wherever they sit in the call (on a handle over several devices: wherever they sit in a device's range of blobs, whose indices and cells start
 * at the sum of the counts before it).  Mainnet handles only.  Large m runs in chunks. */
int kzg355_recover_cells_and_kzg_proofs_many_sets(uint8_t *cells_out /* m*128*2048 or NULL */, uint8_t *proofs_out /* m*128*48 or NULL */,
                                                  int *status /* m or NULL */, const size_t *cell_counts /* m */,
                                                  const size_t *cell_indices /* sum of the counts */,
                                                  const uint8_t *cells /* (sum of the counts)*2048 */, size_t m, const kzg355_settings *s);
/* ---- proofs of chosen cells ----------------------------------------------------------------------------------------------------------------
 * The cells of a blob at k chosen indices and their proofs.  kzg355_compute_cells_and_kzg_proofs runs the whole FK20 chain whatever is wanted
 * of its 128 proofs; here every (blob, index) pair is computed on its own -- the proof as the commitment to the quotient of the blob polynomial
 * by X^64 - a_index, through the fixed-base MSM of the commitment calls -- so that a few proofs of a blob cost a few MSMs (a node that
 * custodies a handful of columns, a server that answers one sample request).  All 128 proofs of many blobs remain the other call's work.
 * Layout: slot j holds cell cell_indices[j] of the blob and its proof, byte for byte what kzg355_compute_cells_and_kzg_proofs returns at that
 * index.  Each index is < 128; they may come in any order and may repeat.  k may be 0 (the blob is still read and checked) and may not exceed
 * 128.  Either output may be NULL, not both (KZG355_BADARGS); without proofs_out no MSM runs and no MSM table is built.  A blob element >= r, an
 * index >= 128 or k > 128 -> KZG355_BADARGS.  The first call that wants proofs builds the handle's fixed-base MSM table, exactly as the first
 * commitment does (kzg355_options.msm_bits; kzg355_settings_build_msm_table builds it ahead of time); a handle loaded with msm_bits = 8 runs
 * the bucket form and gives the same bytes.  Mainnet handles only. */
int kzg355_compute_cell_kzg_proofs_at(uint8_t *cells_out /* k*2048 or NULL */, uint8_t *proofs_out /* k*48 or NULL */, const uint8_t *blob,
                                      const size_t *cell_indices /* k */, size_t k, const kzg355_settings *s);
/* n independent calls of the above in one set of launches: blob i asks for cell_counts[i] cells; with off_i = cell_counts[0] + .. +
 * cell_counts[i-1], its indices are cell_indices[off_i .. off_i + cell_counts[i]) and output slot off_i + j holds cell cell_indices[off_i + j]
 * of blob i and its proof.  A count may be 0: that blob is still read and checked, and it fills no slot.  What is wrong with one blob is that
 * blob's KZG355_BADARGS: an element >= r, an index >= 128, a count > 128.  The other blobs are computed and are right: the layout always follows
 * the counts as given.  The return value is the first non-OK status; the output slots of a refused blob are unspecified.  What is wrong with
 * the call refuses it as a whole and marks every status: a NULL handle, both outputs NULL, NULL blobs, cell_counts or cell_indices with n > 0
 * (cell_indices may be NULL when the sum of the counts is 0), a handle of another FIELD_ELEMENTS_PER_BLOB, n > 2^32, a sum of the counts that
 * overflows size_t (or does so times 2048).  n == 0 -> OK, and nothing is touched.  A handle over several devices spreads contiguous ranges of
 * blobs over them, each range's indices and slots starting at the sum of the counts before it (a blob is never cut), and every range counts in
 * kzg355_settings_cell_calls_per_device.  Large calls run in chunks of whole blobs. */
int kzg355_compute_cell_kzg_proofs_at_many(uint8_t *cells_out /* (sum of the counts)*2048 or NULL */, uint8_t *proofs_out /* (sum)*48 or NULL */,
                                           int *status /* n or NULL */, const uint8_t *blobs /* n*131072 */, size_t n,
                                           const size_t *cell_counts /* n */, const size_t *cell_indices /* sum of the counts */,
                                           const kzg355_settings *s);
/* The same with the blobs and both outputs in HBM: device pointers on the handle's device (its first device, for a handle over several: the
 * call runs on that device alone), 16-byte aligned -- a misaligned pointer refuses the call as a whole; status, counts and indices stay HOST
 * arguments.  The blobs are read and the slots written where they are; nothing but the pair list and the status words crosses PCIe. */
int kzg355_compute_cell_kzg_proofs_at_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status /* host */, const uint8_t *d_blobs, size_t n,
                                                  const size_t *cell_counts /* HOST */, const size_t *cell_indices /* HOST */,
                                                  const kzg355_settings *s);
/* ---- openings at chosen points --------------------------------------------------------------------------------------------------------------
 * A blob opened at k points of the caller's choice: the proofs and the values y = p(z) that kzg355_verify_kzg_proof and the point-evaluation
 * precompile (kzg355_point_evaluation_many) consume.  kzg355_compute_kzg_proof_many takes one 128 KiB blob per opening; here the blob is given
 * once (a server of preimage or fault-proof requests opens the same blob at many points), and every (blob, point) pair is computed on its own
 * -- the quotient of the blob polynomial by X - z by synthetic division, which needs no inversion and is the same route for a z inside the
 * domain as for any other, through the fixed-base MSM of the commitment calls.
 * Layout: slot j receives the proof and y of point zs[32 j .. 32 j + 32), byte for byte what kzg355_compute_kzg_proof returns for (blob, z).
 * Points may repeat, come in any order and lie inside the domain.  k may be 0 (the blob is still read and checked; zs may then be NULL) and
 * may not exceed 4096, one opening per element of the blob.  Either output may be NULL, not both (KZG355_BADARGS); without proofs_out no MSM
 * runs and no MSM table is built: the call is then evaluate_polynomial_in_evaluation_form at many points.  A blob element >= r, a point >= r
 * (non-canonical) or k > 4096 -> KZG355_BADARGS.  The first call that wants proofs builds the handle's fixed-base MSM table, exactly as the
 * first commitment does (kzg355_options.msm_bits; kzg355_settings_build_msm_table builds it ahead of time); a handle loaded with
 * msm_bits = 8 runs the bucket form and gives the same bytes.  Mainnet handles only. */
int kzg355_compute_kzg_proofs_at(uint8_t *proofs_out /* k*48 or NULL */, uint8_t *ys_out /* k*32 or NULL */, const uint8_t *blob,
                                 const uint8_t *zs /* k*32 */, size_t k, const kzg355_settings *s);
/* n independent calls of the above in one set of launches: blob i is opened at point_counts[i] points; with off_i = point_counts[0] + .. +
 * point_counts[i-1], its points are zs[32 off_i .. 32 (off_i + point_counts[i])) and output slot off_i + j receives the proof and y of the
 * j-th of them.  A count may be 0: that blob is still read and checked, and it fills no slot.  What is wrong with one blob is that blob's
 * KZG355_BADARGS: an element >= r, any of its points >= r, a count > 4096.  The other blobs are computed and are right: the layout always
 * follows the counts as given.  The return value is the first non-OK status in blob order; the output slots of a refused blob are
 * unspecified.  What is wrong with the call refuses it as a whole and marks every status, before any array is read or any device is
 * touched: a NULL handle, both outputs NULL, NULL blobs or point_counts with n > 0, NULL zs while the counts sum to more than 0, a handle of
 * another FIELD_ELEMENTS_PER_BLOB, n > 2^32, a sum of the counts that overflows size_t (alone or times 48).  n == 0 -> OK, and nothing is
 * touched.  A handle over several devices spreads contiguous ranges of blobs over them, each range's points and slots starting at the sum of
 * the counts before it, and every range counts in kzg355_settings_cell_calls_per_device.  Large calls run in chunks of at most 512 blobs and
 * 1152 openings; a blob with more openings than a chunk has room for is cut at the chunk's border and read again by the next chunk.
 * Not offered: cutting one blob's points over several devices (a range is whole blobs); a status per point; an FK20 form for all 4096
 * openings of a blob. */
int kzg355_compute_kzg_proofs_at_many(uint8_t *proofs_out /* (sum of the counts)*48 or NULL */, uint8_t *ys_out /* (sum)*32 or NULL */,
                                      int *status /* n or NULL */, const uint8_t *blobs /* n*131072 */, size_t n,
                                      const size_t *point_counts /* n */, const uint8_t *zs /* (sum of the counts)*32 */,
                                      const kzg355_settings *s);
/* The same with the blobs and both outputs in HBM: device pointers on the handle's device (its first device, for a handle over several: the
 * call runs on that device alone), 16-byte aligned -- a misaligned pointer refuses the call as a whole; status, the counts and zs stay HOST
 * arguments (the host checks the points while it plans the chunks).  The blobs are read and the slots written where they are; nothing but
 * the points, the pair list and the status words crosses PCIe. */
int kzg355_compute_kzg_proofs_at_many_device(uint8_t *d_proofs_out, uint8_t *d_ys_out, int *status /* host */, const uint8_t *d_blobs, size_t n,
                                             const size_t *point_counts /* HOST */, const uint8_t *zs /* HOST */, const kzg355_settings *s);
/* ---- chosen cells of recovered blobs -----------------------------------------------------------------------------------------------------
 * kzg355_recover_cells_and_kzg_proofs runs the whole FK20 chain whatever is wanted of its 128 proofs.  A node that holds most columns of a
 * block and lacks a few wants the cells and proofs of the missing ones, or of the few it custodies: here the blob is recovered as there, and
 * then every wanted (blob, index) pair is computed on its own, as kzg355_compute_cell_kzg_proofs_at does for a blob.
 * Input: that of kzg355_recover_cells_and_kzg_proofs (n known cells at strictly ascending cell_indices, 64 <= n <= 128).  Output: that of
 * kzg355_compute_cell_kzg_proofs_at -- slot j holds cell want_indices[j] of the recovered extension and its proof, byte for byte what
 * kzg355_recover_cells_and_kzg_proofs returns at that index for the same input (for a known index too, and also when more than 64 cells lie
 * on no polynomial of degree < 4096: the result is that of the 4096 coefficients the specs' algorithm keeps, as there).  Each wanted index is
 * < 128; they may come in any order and may repeat.  k may be 0 (the blob is still recovered and checked; want_indices may then be NULL) and
 * may not exceed 128.  Either output may be NULL, not both; without proofs_out no MSM runs and no MSM table is built.  The first call that
 * wants proofs builds the handle's fixed-base MSM table, exactly as the first commitment does; a handle loaded with msm_bits = 8 runs the
 * bucket form and gives the same bytes.  n outside 64..128, a known index >= 128, known indices not strictly ascending, a cell element >= r,
 * a wanted index >= 128 or k > 128 -> KZG355_BADARGS.  Mainnet handles only. */
int kzg355_recover_cells_and_kzg_proofs_at(uint8_t *cells_out /* k*2048 or NULL */, uint8_t *proofs_out /* k*48 or NULL */,
                                           const size_t *cell_indices /* n */, const uint8_t *cells /* n*2048 */, size_t n,
                                           const size_t *want_indices /* k */, size_t k, const kzg355_settings *s);
/* m independent calls of the above in one set of launches.  Input layout of kzg355_recover_cells_and_kzg_proofs_many_sets: blob i is known
 * at cell_counts[i] cells; with koff_i the sum of the cell_counts before it, its indices are cell_indices[koff_i ..] and its cells are at
 * cells + 2048 * koff_i.  Output layout of kzg355_compute_cell_kzg_proofs_at_many: with woff_i the sum of the want_counts before blob i, slot
 * woff_i + j holds cell want_indices[woff_i + j] of blob i's recovered extension and its proof.  A want count may be 0: that blob is still
 * recovered and checked, and it fills no slot; want_indices may be NULL when the want counts sum to 0.  What is wrong with one blob is that
 * blob's KZG355_BADARGS: a known count outside 64..128, a known index >= 128, known indices not strictly ascending, a cell element >= r, a
 * wanted index >= 128, a want count > 128.  The other blobs are computed and are right: both layouts always follow the counts as given.  The
 * return value is the first non-OK status; the output slots of a refused blob are unspecified.  What is wrong with the call refuses it as a
 * whole and marks every status, before any array is read or any device is touched: a NULL handle, both outputs NULL, NULL cell_counts,
 * want_counts, cell_indices or cells with m > 0, NULL want_indices while the want counts sum to more than 0, a handle of another
 * FIELD_ELEMENTS_PER_BLOB, m > 2^32, either sum of counts overflowing size_t (alone or times 2048).  m == 0 -> OK, and nothing is touched.  A
 * handle over several devices spreads contiguous ranges of blobs over them, each range starting at its own two prefix sums (a blob is never
 * cut), and every range counts in kzg355_settings_cell_calls_per_device.  Blobs known at the same index set share its tables wherever they sit
 * in a chunk; large calls run in chunks of whole blobs.
 * Not offered: a form with one index set shared by all blobs (the sets form already shares tables between blobs of equal sets), and a switch
 * to the FK20 chain when many blobs want many cells -- that remains kzg355_recover_cells_and_kzg_proofs_many_sets.  Measured on one MI355X
 * ("Recovery of chosen cells"): with 1, 6 and 21 blobs this call is the quicker one up to all the cells measured (6 blobs x 64
 * wanted: 5.8 against 67.2 ms); at 128 blobs the two cross at about 50 wanted cells per blob on the wide MSM table and at about 17 on the
 * bucket form (msm_bits = 8). */
int kzg355_recover_cells_and_kzg_proofs_at_many_sets(uint8_t *cells_out /* (sum of the want counts)*2048 or NULL */,
                                                     uint8_t *proofs_out /* (sum of the want counts)*48 or NULL */, int *status /* m or NULL */,
                                                     const size_t *cell_counts /* m */, const size_t *cell_indices /* sum of the cell counts */,
                                                     const uint8_t *cells /* (sum of the cell counts)*2048 */, const size_t *want_counts /* m */,
                                                     const size_t *want_indices /* sum of the want counts */, size_t m, const kzg355_settings *s);
/* The same with the known cells and both outputs in HBM: device pointers on the handle's device (its first device, for a handle over several:
 * the call runs on that device alone), 16-byte aligned -- a misaligned pointer refuses the call as a whole; status, the counts and both index
 * lists stay HOST arguments.  The cells are read and the slots written where they are. */
int kzg355_recover_cells_and_kzg_proofs_at_many_sets_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status /* host */,
                                                            const size_t *cell_counts /* HOST */, const size_t *cell_indices /* HOST */,
                                                            const uint8_t *d_cells, const size_t *want_counts /* HOST */,
                                                            const size_t *want_indices /* HOST */, size_t m, const kzg355_settings *s);
/* Test form: the FK20 intermediates H_0 .. H_63 of each blob, compressed (H_e = sum_{m >= 64(e+1)} f_m [tau^(m - 64(e+1))]_1; H_63 = infinity). */
int kzg355_debug_cell_compute_h(uint8_t *out /* n*64*48 */, int *status /* n or NULL */, const uint8_t *blobs, size_t n, const kzg355_settings *s);
/* The 4096 monomial points [tau^t]_1 the handle derived for compute_cells_and_kzg_proofs, compressed (building the proof setup first if needed). */
int kzg355_debug_cell_setup_monomial_all(uint8_t *out /* 4096*48 */, const kzg355_settings *s);
/* ---- EIP-7594 cell calls on device-resident data -------------------------------------------------------------------------------------------
 * The three *_many cell calls with their bulk arguments in HBM: every d_* argument is a DEVICE pointer on the handle's device (its first device,
 * for a handle over several: these calls run on that device alone), ok / status are host pointers, and the calls are synchronous like the other *_device calls.  Layouts, NULL-output
 * meanings, per-unit status, "a refusal of the whole call marks every unit", the n == 0 / m == 0 / groups == 0 / n_per_group == 0 cases and every
 * KZG355_BADARGS rule are those of the host forms above.  Device byte buffers (commitments, cells, proofs, blobs, outputs) must be 16-byte
 * aligned and device cell indices 8-byte aligned (hipMalloc and torch allocations are); a misaligned pointer is KZG355_BADARGS.  Output buffers
 * must not overlap the inputs.  Nothing but the 4-byte status words (and the verdicts) crosses PCIe, except as the next paragraph says.
 *
 * Verification prepares a batch -- commitment deduplication, the column sort and the transcript SHA-256 -- on the device, reading the caller's
 * buffers where they are.  A transcript is one serial hash chain per group, so a call of few groups with long transcripts is quicker when the
 * four arrays are copied back and the host prepares them as it does for the host form: the call chooses by shape (bytes of transcript per group
 * and groups per compute unit), and the answer is the same either way.  The device preparation takes up to 16384 cells
 * per group (128 blobs x 128 cells: a whole block as one batch); a call with more per group (up to the host form's limit) always takes the
 * host preparation. */
int kzg355_verify_cell_kzg_proof_batch_many_device(bool *ok /* host, groups */, int *status /* host, groups or NULL */, const uint8_t *d_commitments,
                                                   const size_t *d_cell_indices, const uint8_t *d_cells, const uint8_t *d_proofs, size_t n_per_group,
                                                   size_t groups, const kzg355_settings *s);
/* compute_cells_and_kzg_proofs of n resident blobs; the cells and proofs are written straight into the caller's device buffers (either may be
 * NULL, not both).  The output slots of a blob whose status is not KZG355_OK are unspecified. */
int kzg355_compute_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out /* n*128*2048 or NULL */, uint8_t *d_proofs_out /* n*128*48 or NULL */,
                                                    int *status /* host, n or NULL */, const uint8_t *d_blobs, size_t n, const kzg355_settings *s);
/* recover_cells_and_kzg_proofs of m resident blobs known at the same n cell indices.  The index set stays a HOST argument (at most 128 values,
 * checked before any device work); outputs as in the call above. */
int kzg355_recover_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out /* m*128*2048 or NULL */, uint8_t *d_proofs_out /* m*128*48 or NULL */,
                                                    int *status /* host, m or NULL */, const size_t *cell_indices /* HOST, n, shared by all blobs */,
                                                    const uint8_t *d_cells /* m*n*2048: blob after blob */, size_t n, size_t m, const kzg355_settings *s);
/* kzg355_recover_cells_and_kzg_proofs_many_sets with d_cells and both outputs in HBM (16-byte aligned, as the other *_device cell calls; a
 * misaligned pointer refuses the call as a whole); counts and indices stay HOST arguments.  The cells are read where they are. */
int kzg355_recover_cells_and_kzg_proofs_many_sets_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const size_t *cell_counts,
                                                         const size_t *cell_indices, const uint8_t *d_cells, size_t m, const kzg355_settings *s);
/* ---- commitments out of the FK20 chain --------------------------------------------------------------------------------------------------------
 * The six calls below are kzg355_compute_cells_and_kzg_proofs_many, kzg355_recover_cells_and_kzg_proofs_many, .._many_sets and their *_device
 * forms with one more output in front: commitments_out, 48 bytes per blob, the blob's KZG commitment (what kzg355_blob_to_kzg_commitment
 * returns for it; the zero polynomial gives c0 00..00).  The chain computes it on its way to the proofs: slot 63 of the 128-point convolution
 * whose slots 0..62 are the proofs' H_e is sum_m f_m [tau^m]_1, so a block builder gets commitment, cells and proofs
 * from one call and no wide MSM table is built, and a node that rebuilt blobs from columns can compare 48 bytes per blob with the block's
 * blob_kzg_commitments.  Any of the three outputs may be NULL (that part is not computed), not all three: KZG355_BADARGS, every status marked.
 * With commitments_out == NULL a call is the one it is named after, byte for byte, and every other rule of that call holds unchanged: per-blob
 * statuses, what refuses the call as a whole, n == 0, mainnet handles only, chunks, the spread over the devices of a handle over several
 * (host forms).  The commitment slot of a blob whose status is not KZG355_OK is unspecified, like its other slots.  Recovery from more than 64
 * cells that lie on no polynomial of degree < 4096 returns the commitment of the 4096 coefficients the algorithm keeps, so that the
 * comparison with the expected commitment is what shows such cells up.  A call that wants commitments alone is legal: it builds the proof
 * setup (384 MiB table) and runs the chain up to the inverse G1 transform; for computing, kzg355_blob_to_kzg_commitment_many is the cheaper
 * route to commitments alone.  *_device: d_commitments_out is device memory on the handle's first device, 16-byte aligned like the other
 * pointers (a misaligned one refuses the call as a whole, and nothing is written). */
int kzg355_compute_commitments_cells_and_kzg_proofs_many(uint8_t *commitments_out /* n*48 or NULL */, uint8_t *cells_out /* n*128*2048 or NULL */,
                                                         uint8_t *proofs_out /* n*128*48 or NULL */, int *status /* n or NULL */,
                                                         const uint8_t *blobs, size_t n, const kzg355_settings *s);
int kzg355_compute_commitments_cells_and_kzg_proofs_many_device(uint8_t *d_commitments_out /* n*48 or NULL */,
                                                                uint8_t *d_cells_out /* n*128*2048 or NULL */,
                                                                uint8_t *d_proofs_out /* n*128*48 or NULL */, int *status /* host, n or NULL */,
                                                                const uint8_t *d_blobs, size_t n, const kzg355_settings *s);
int kzg355_recover_commitments_cells_and_kzg_proofs_many(uint8_t *commitments_out /* m*48 or NULL */, uint8_t *cells_out /* m*128*2048 or NULL */,
                                                         uint8_t *proofs_out /* m*128*48 or NULL */, int *status /* m or NULL */,
                                                         const size_t *cell_indices /* n, shared by all blobs */,
                                                         const uint8_t *cells /* m*n*2048: blob after blob */, size_t n, size_t m,
                                                         const kzg355_settings *s);
int kzg355_recover_commitments_cells_and_kzg_proofs_many_device(uint8_t *d_commitments_out /* m*48 or NULL */,
                                                                uint8_t *d_cells_out /* m*128*2048 or NULL */,
                                                                uint8_t *d_proofs_out /* m*128*48 or NULL */, int *status /* host, m or NULL */,
                                                                const size_t *cell_indices /* HOST, n, shared by all blobs */,
                                                                const uint8_t *d_cells /* m*n*2048: blob after blob */, size_t n, size_t m,
                                                                const kzg355_settings *s);
int kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(uint8_t *commitments_out /* m*48 or NULL */,
                                                              uint8_t *cells_out /* m*128*2048 or NULL */,
                                                              uint8_t *proofs_out /* m*128*48 or NULL */, int *status /* m or NULL */,
                                                              const size_t *cell_counts /* m */, const size_t *cell_indices /* sum of the counts */,
                                                              const uint8_t *cells /* (sum of the counts)*2048 */, size_t m,
                                                              const kzg355_settings *s);
int kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(uint8_t *d_commitments_out, uint8_t *d_cells_out, uint8_t *d_proofs_out,
                                                                     int *status, const size_t *cell_counts, const size_t *cell_indices,
                                                                     const uint8_t *d_cells, size_t m, const kzg355_settings *s);
/* Test form of the device verify call: the 176 bytes per group of kzg355_debug_cell_batch_intermediates, with the preparation pinned by
 * prep_form: 0 by shape (what the call above does), 1 on the device, 2 copy back and prepare on the host; anything else is KZG355_BADARGS. */
int kzg355_debug_cell_batch_intermediates_device(uint8_t *out /* host, groups*176 */, bool *ok /* host, groups */, int *status /* host, groups or NULL */,
                                                 const uint8_t *d_commitments, const size_t *d_cell_indices, const uint8_t *d_cells, const uint8_t *d_proofs,
                                                 size_t n_per_group, size_t groups, int prep_form, const kzg355_settings *s);
/* kzg355_verify_cell_kzg_proof_batch_many_sets with the four bulk arrays in HBM (sidecars received over RDMA, or the outputs of the compute and
 * recover *_device calls): device pointers on the handle's first device, the byte buffers 16-byte and the indices 8-byte aligned -- a misaligned
 * pointer refuses the call as a whole: KZG355_BADARGS -- read where they are; ok, status and cell_counts are HOST pointers.  Layout, results
 * per group, empty groups, the limits and everything that refuses the call from the counts alone, before any device is touched, are those of
 * the host form.  One set of launches on that device for all non-empty groups, counted once in kzg355_settings_cell_calls_per_device; a group is
 * never cut over several devices.  The preparation runs on the device (one workgroup per group; nothing per cell crosses PCIe, only two
 * offsets per group go up) or, the four arrays copied back, on the host: the rule of kzg355_verify_cell_kzg_proof_batch_many_device applied to
 * the call's largest group and its number of non-empty groups, and always the host with a group above 16384 cells.  That rule was measured on
 * uniform shapes only.  On the three ragged shapes timed so far ("Ragged device-resident cell verify": 128 groups of 1 .. 64 cells,
 * 1024 groups of 1 .. 6, 8 groups of 1000 .. 16000) it chose the host preparation every time: the faster route at the first and the third, a
 * tie at the second.  There the call was level with copying the arrays back and calling the host form at the two small shapes and took 45 ms
 * against 70 ms at the large one; with the device preparation it was never the quicker of the two. */
int kzg355_verify_cell_kzg_proof_batch_many_sets_device(bool *ok /* host, groups */, int *status /* host, groups or NULL */,
                                                        const size_t *cell_counts /* HOST, groups */, const uint8_t *d_commitments,
                                                        const size_t *d_cell_indices, const uint8_t *d_cells,
                                                        const uint8_t *d_proofs /* each: sum of the counts entries */, size_t groups,
                                                        const kzg355_settings *s);
/* Test form of the call above: out[176 g ..] as kzg355_debug_cell_batch_intermediates_sets lays it out (zero bytes for a count of 0), prep_form as
 * in kzg355_debug_cell_batch_intermediates_device (with prep_form 1 and a group above 16384 cells the host still prepares). */
int kzg355_debug_cell_batch_intermediates_sets_device(uint8_t *out /* host, groups*176 */, bool *ok, int *status, const size_t *cell_counts,
                                                      const uint8_t *d_commitments, const size_t *d_cell_indices, const uint8_t *d_cells,
                                                      const uint8_t *d_proofs, size_t groups, int prep_form, const kzg355_settings *s);
/* How many device-resident cell verify calls on this handle were prepared on the device so far (the others took the host preparation). */
long kzg355_settings_cell_device_prep_calls(const kzg355_settings *s);
/* How the cell calls of a handle were spread: returns the number of devices the handle spans (1 for a plain handle) and fills out[d], d < min(cap,
 * that number), with the cell launch sets device d has run so far -- a verify, compute or recover call (or its range of one) counts one on the
 * device that ran it, a verify call cut into blocks one on every device.  A call refused as a whole counts nowhere.  A NULL handle, or a NULL out
 * with cap > 0, is KZG355_BADARGS. */
int kzg355_settings_cell_calls_per_device(const kzg355_settings *s, long *out /* cap */, size_t cap);
/* ---- blobs against their EIP-7594 cell proofs ----------------------------------------------------------------------------------------------
 * The Fulu counterpart of kzg355_verify_blob_kzg_proof_batch: since EIP-7594 a blob transaction (or a builder's blobs bundle) carries the 128 cell
 * proofs of each blob instead of one blob proof, and is checked by VerifyCellProofs(blobs, commitments, cell_proofs).  For n blobs with their n
 * commitments and 128 n cell proofs (blob after blob, cell order) the answer is EXACTLY that of kzg355_verify_cell_kzg_proof_batch on 128 n
 * cells, the cell at position 128 b + k having commitment b, cell index k, cell k of kzg355_compute_cells_and_kzg_proofs(blob b) and proof
 * 128 b + k: the same verdict, the same statuses and the same challenge r (the commitments deduplicated by their bytes in order of first
 * appearance; the transcript hashes the computed cells).  n == 0 -> true.  A blob element >= r, or a commitment or proof that fails
 * validate_kzg_g1 -> KZG355_BADARGS.  n_commitments != n_blobs or n_cell_proofs != 128 n_blobs -> KZG355_BADARGS.  Mainnet handles only.
 * The blobs cross PCIe once (128 KiB each); their cells are computed and checked on the device, and the call builds no proof setup (the 384 MiB
 * table of kzg355_compute_cells_and_kzg_proofs is not needed). */
int kzg355_verify_blob_cell_proofs_batch(bool *ok, const uint8_t *blobs, size_t n_blobs, const uint8_t *commitments, size_t n_commitments,
                                         const uint8_t *cell_proofs, size_t n_cell_proofs, const kzg355_settings *s);
/* `groups` independent calls of the above (one verdict per transaction) in one set of launches: the three arrays group-major, n_per_group blobs
 * (and commitments, and 128 n_per_group proofs) each.  ok[g] / status[g] per group; the return value is the first non-OK status; what is wrong
 * with one group is that group's status and leaves the others alone.  A refusal of the call as a whole marks every group: a NULL handle or array,
 * a handle of another FIELD_ELEMENTS_PER_BLOB, n_per_group above 2048 blobs (262144 cells, the most one set of launches takes), groups above
 * 2^24.  groups == 0 -> OK and nothing is touched; n_per_group == 0 -> every group true.  More groups than fit one set of launches (2048 blobs)
 * run in chunks of whole groups inside the call.  A handle over several devices spreads the groups over them in contiguous ranges, as the other
 * host-buffer cell calls do (a group is never cut), and counts its launch sets in kzg355_settings_cell_calls_per_device. */
int kzg355_verify_blob_cell_proofs_batch_many(bool *ok /* groups */, int *status /* groups or NULL */, const uint8_t *blobs, const uint8_t *commitments,
                                              const uint8_t *cell_proofs, size_t n_per_group, size_t groups, const kzg355_settings *s);
/* The same with the three bulk arrays in HBM: device pointers on the handle's device (its first device, for a handle over several), 16-byte
 * aligned (a misaligned pointer is KZG355_BADARGS); ok / status are host pointers.  The 48 bytes of every commitment come back for the
 * deduplication; calls of few groups also copy the cells and proofs back and hash their transcripts on the host, by the rule of
 * kzg355_verify_cell_kzg_proof_batch_many_device (always above 128 blobs per group). */
int kzg355_verify_blob_cell_proofs_batch_many_device(bool *ok /* host, groups */, int *status /* host, groups or NULL */, const uint8_t *d_blobs,
                                                     const uint8_t *d_commitments, const uint8_t *d_cell_proofs, size_t n_per_group, size_t groups,
                                                     const kzg355_settings *s);
/* Test forms: out[176 g ..] receives r | [I(tau)]_1 | LL | RL of group g as kzg355_debug_cell_batch_intermediates lays them out.  interp_form pins
 * how [I(tau)]_1's scalars are found: 0 what the calls above do, 1 from the blobs' monomial coefficients, 2 by the column
 * kernel of kzg355_verify_cell_kzg_proof_batch over the computed cells; prep_form as in kzg355_debug_cell_batch_intermediates_device (1: the
 * transcripts are hashed on the device, 2: on the host).  Any other value of either is KZG355_BADARGS. */
int kzg355_debug_blob_cell_batch_intermediates(uint8_t *out /* groups*176 */, bool *ok /* groups */, int *status /* groups or NULL */, const uint8_t *blobs,
                                               const uint8_t *commitments, const uint8_t *cell_proofs, size_t n_per_group, size_t groups, int interp_form,
                                               const kzg355_settings *s);
int kzg355_debug_blob_cell_batch_intermediates_device(uint8_t *out /* host, groups*176 */, bool *ok /* host, groups */, int *status /* host, groups or NULL */,
                                                      const uint8_t *d_blobs, const uint8_t *d_commitments, const uint8_t *d_cell_proofs, size_t n_per_group,
                                                      size_t groups, int interp_form, int prep_form, const kzg355_settings *s);
/* Groups of DIFFERENT blob counts in one call (the blob transactions of a mempool or a builder: 1, 2, 3 ... blobs side by side), one set of
 * launches for all non-empty groups.  Layout: with boff_g = blob_counts[0] + ... + blob_counts[g-1], group g is blobs [boff_g, boff_g +
 * blob_counts[g]) of `blobs`, the same entries of `commitments` and proofs [128 boff_g, 128 (boff_g + blob_counts[g])) of `cell_proofs`; the
 * arrays hold the groups one after the other, with no padding.
 * Result per group: EXACTLY that of kzg355_verify_blob_cell_proofs_batch on that slice -- the same verdict, status and challenge r; commitments
 * deduplicated inside the group only, in order of first appearance; the transcript carries the group's own 128 * count.  A count of 0: that group
 * is true / KZG355_OK.  A blob element >= r, a commitment or proof that fails validate_kzg_g1: that group's KZG355_BADARGS, the others are left
 * alone; the return value is the first non-OK status in group order.
 * Refused as a whole (every status marked, every verdict false), decided from the counts alone, before any array is read and before any device
 * is touched: a NULL handle, NULL ok, or NULL blob_counts with groups > 0; a NULL array while the sum of the counts is > 0; a handle of another
 * FIELD_ELEMENTS_PER_BLOB; groups above 2^24; one count above 2048 blobs (the most one set of launches takes, as for n_per_group above); a sum of
 * the counts that overflows size_t, alone or times 131072.  groups == 0: KZG355_OK, nothing is touched.
 * The sum of the counts is not limited: the non-empty groups run in launch sets of whole groups, taken in order while the set's blobs stay
 * within 2048.  Work and device memory are proportional to the sum of the counts, not to groups times the largest count.
 * A handle over several devices: the non-empty groups go to the devices in contiguous ranges, equal in GROUPS -- so the ranges can be uneven in
 * blobs (not measured on several cards).  A group is never cut.  kzg355_settings_cell_calls_per_device counts the launch sets of every device
 * that received a non-empty group. */
int kzg355_verify_blob_cell_proofs_batch_many_sets(bool *ok /* groups */, int *status /* groups or NULL */, const size_t *blob_counts /* groups */,
                                                   const uint8_t *blobs, const uint8_t *commitments,
                                                   const uint8_t *cell_proofs /* sum of the counts blobs / commitments / x128 proofs */, size_t groups,
                                                   const kzg355_settings *s);
/* The same with the three bulk arrays in HBM, as kzg355_verify_blob_cell_proofs_batch_many_device takes them: device pointers on the handle's
 * first device, 16-byte aligned (a misaligned pointer refuses the call: KZG355_BADARGS); ok, status and blob_counts are HOST pointers.  The 48
 * bytes of every commitment come back for the deduplication; whether the transcripts are hashed on the device follows the rule of
 * kzg355_verify_cell_kzg_proof_batch_many_device applied to a launch set's largest group and its number of groups (always on the host with a
 * group above 128 blobs) -- a rule measured on uniform shapes only. */
int kzg355_verify_blob_cell_proofs_batch_many_sets_device(bool *ok /* host, groups */, int *status /* host, groups or NULL */,
                                                          const size_t *blob_counts /* HOST, groups */, const uint8_t *d_blobs, const uint8_t *d_commitments,
                                                          const uint8_t *d_cell_proofs, size_t groups, const kzg355_settings *s);
/* Test forms of the two _many_sets calls: out[176 g ..] as kzg355_debug_blob_cell_batch_intermediates lays it out, zero bytes for a group of
 * count 0; interp_form and prep_form as there (interp_form 0: per set of launches from its blob total; any value out of range refuses the call). */
int kzg355_debug_blob_cell_batch_intermediates_sets(uint8_t *out /* groups*176 */, bool *ok, int *status, const size_t *blob_counts, const uint8_t *blobs,
                                                    const uint8_t *commitments, const uint8_t *cell_proofs, size_t groups, int interp_form,
                                                    const kzg355_settings *s);
int kzg355_debug_blob_cell_batch_intermediates_sets_device(uint8_t *out, bool *ok, int *status, const size_t *blob_counts, const uint8_t *d_blobs,
                                                           const uint8_t *d_commitments, const uint8_t *d_cell_proofs, size_t groups, int interp_form,
                                                           int prep_form, const kzg355_settings *s);
int kzg355_host_sha256(uint8_t out[32], const uint8_t *msg, size_t len, int impl);
int kzg355_host_challenge_digests(uint8_t *out /* n*32 */, const uint8_t *blobs, size_t blob_bytes, const uint8_t *commitments /* n*48 */, size_t n, int impl);

#ifdef __cplusplus
}
#endif
#endif /* KZG355_H */
