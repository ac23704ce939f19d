// kernels.h -- internal interface between the C-ABI host code (engine.h and the host translation units it lists) and the HIP kernel translation
// units (k_setup.hip, k_verify.hip, k_msm.hip, k_prove.hip).  Not installed; the public boundary is
// include/kzg355.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "field.h"
#include "tower.h"
#include "g1.h"
#include "pairing.h"
#include "sha256.h"
#include "pairing_coop.h"
#include "eval_core.h"
#include "cell_plan.h"
#include "point_plan.h"

namespace kzg {

constexpr int N_FE = 4096;                 // FIELD_ELEMENTS_PER_BLOB (consts.rs:13)
constexpr int BLOB_BYTES = N_FE * 32;      // consts.rs:16
constexpr int RECORD_BYTES = 160;          // C | z | y | proof  (utils.rs:454-463)
constexpr int MSM_WINDOW_BITS = 8;
constexpr int MSM_WINDOWS = 32;            // 32 x 8 bits cover the 255-bit scalars
constexpr int MSM_BUCKETS = 128;           // signed digits in [-127, 128]
// wide-window form of the same MSM (k_msm_wide.hip): signed c-bit digits, every multiple 1..2^(c-1) tabulated; c is chosen when
// the handle is created (12: 22 windows, 23.6 GB; 13: 20 windows, 42.9 GB; 14: 19 windows, 81.6 GB)
// Shape of the fixed-base MSM table (k_msm_wide.hip): `windows` signed `bits`-bit windows of `rows` = 2^(bits-1) multiples each, except the
// top window, which takes an unsigned digit (no carry leaves it) and has rows_top rows.  glv = 0: the windows span the 256 bits of the scalar.
// glv = 1 (round 4): the scalar is split k = a + b x^2 (g1.h glv_split_fast; a, b < x^2 < 2^127.5) and the windows span 128 bits -- the
// SAME table serves both halves, because sum_i [b_i](-phi P_i) = -phi(sum_i [b_i] P_i): the rows of the b halves are added up as they
// are and the endomorphism is applied once, to their sum.  Half the table at the same number of rows per scalar, or (16-bit windows: 8
// windows per half) 16 rows per scalar in 143 GB where the 256-bit form took 17.45 rows in 155 GB.
struct WideShape { int bits, windows, rows, glv, rows_top; };
inline WideShape wide_shape(int bits, bool glv = false) {
    WideShape w; w.bits = bits; w.rows = 1 << (bits - 1); w.glv = glv ? 1 : 0;
    if (!glv) { w.windows = (256 + bits - 1) / bits; w.rows_top = w.rows; return w; }
    w.windows = (128 + bits - 1) / bits;
    // largest top digit: the top bits of x^2 - 1 = 0xac45a4010001a40200000000ffffffff (both halves are below x^2), plus the carry coming in
    const int shift = bits * (w.windows - 1);                     // >= 96 for every supported width
    const unsigned top = (unsigned)(0xac45a401u >> (shift - 96)) + 1u;
    w.rows_top = (int)((top + 256u) & ~255u);                     // (segments of 256 rows: k_wide_rows)
    return w;
}
inline size_t wide_rows_per_point(WideShape w) { return (size_t)(w.windows - 1) * w.rows + w.rows_top; }
constexpr int N_G2 = 65;

// error bits accumulated on the device; any bit => the call returns Err (reference: `?` on each step)
constexpr int ERR_BAD_POINT = 1;           // validate_kzg_g1 failed (utils.rs:282-310)
constexpr int ERR_NONCANONICAL_FR = 2;     // bytes_to_bls_field failed (utils.rs:262-275)
constexpr int ERR_SETUP_POINT = 4;         // load_trusted_setup: bad g1/g2 bytes (kzg.rs:863, 878)
constexpr int ERR_SETUP_MONOMIAL = 8;      // is_trusted_setup_in_lagrange_form (kzg.rs:823-826)
constexpr int ERR_CELL_INDEX = 16;         // a cell index >= CELLS_PER_EXT_BLOB, found by the device preparation (k_cell_prep.hip)

struct alignas(128) WideRow { Fp x, y; uint32_t pad[4]; };       // one affine point per 128-byte line

struct DeviceTables {
    int n_fe;                // FIELD_ELEMENTS_PER_BLOB of this handle: 4096 (mainnet) or a small power of two (minimal preset: 4)
    Fr *roots;               // [4096] bit-reversal order, Montgomery (kzg.rs:34)
    EvalPiece *eval_tab;     // [EVAL_TAB_PIECES] the node roots of k_eval's tree, three per group, levels 1..6, in 16-byte pieces (eval_core.h)
    WideShape wide;          // shape of wide_table
    WideRow *wide_table;        // [22][4096][2048] multiples m * 2^(12w) * g1_values[i], 23.6 GB; null: 8-bit bucket form only
    G1Affine *msm_table;     // [32][4096]: window w holds 2^(8w) * g1_values[i]; window 0 IS g1_values (kzg.rs:37)
    LineCoeff *lines;        // [3][68]: Miller-loop lines of G2_GENERATOR, setup g2[0], setup g2[1]
    int *lines_inf;          // [3] 1 if that G2 point is the point at infinity
    G1Affine *g1_first2;     // file-order g1[0], g1[1] (only for the Lagrange-form check)
    LineW *lines_w;          // [3][68]: the same lines in the w basis (pairing_coop.h)
    FrobTables *frob;        // w-basis Frobenius tables
    CoopInsn *pairing_prog;  // the pairing check as an instruction list (pairing_coop.h)
    int pairing_prog_len;
    int pairing_hard_start;  // index of the first instruction of the final exponentiation's hard part (k_pairing_hard12 runs the tail)
    CoopScheds *coop_scheds; // product, square, line-product and cyclotomic-square work schedules
};

// ---- k_setup.hip
int launch_setup(const uint8_t *d_g1_bytes, const uint8_t *d_g2_bytes, DeviceTables t, int *d_err, hipStream_t st);

// ---- k_verify.hip
// stage 1 (per blob): validate points, Fiat-Shamir challenge, barycentric evaluation -> 160-byte records
// d_proofs may be null (commitments only, e.g. compute_blob_kzg_proof's challenge step, kzg.rs:321)
void launch_validate_points(const uint8_t *d_commitments, const uint8_t *d_proofs, int n_total, int n_per_group,
                            G1Affine *d_pts /* [group][2*npg]: commitments then proofs; may be null */, int *d_err /* per group */,
                            hipStream_t st, int stride = 48 /* bytes between consecutive inputs: 48 packed, 160 inside records */,
                            G1Jac *d_q = nullptr /* in the layout of d_pts: [|x|]P of every point, Jacobian -- the first ladder of the subgroup test, kept
                                                    for the quarters form of launch_lincomb_buckets; infinity for a point at infinity or a failed one */);
// validate_kzg_g1 in two launches: decoding (-> points, error on a bad encoding / off-curve x) and the subgroup test (-> error only)
void launch_decompress_points(const uint8_t *d_commitments, const uint8_t *d_proofs, int n_total, int n_per_group, G1Affine *d_pts, int *d_err, hipStream_t st,
                              int stride = 48);
void launch_subgroup_points(const G1Affine *d_pts, int n_total, int n_per_group, int *d_err, hipStream_t st, int commitments_only = 0);
void launch_dump_intermediates(const uint32_t *d_scal_a, const PairPt *d_pair_pts, int n_per_group, int groups, uint8_t *d_out /* [groups][128] */,
        hipStream_t st);
// d_zpow (may be null): EVAL_ZPOWERS values per blob, z^2, z^4, .. z^4096 (Montgomery) -- what launch_eval needs beside z
void launch_challenges(const uint8_t *d_blobs, const uint8_t *d_commitments, const uint8_t *d_proofs, int n_total,
                       Fr *d_z, Fr *d_zpow, uint8_t *d_records, hipStream_t st, int form = 0 /* 0 by size, 1 one wave, 2 two waves */);
// the same records / z from digests hashed on the host (32 bytes per blob, host_sha256.h)
void launch_challenges_from_digests(const uint8_t *d_digests, const uint8_t *d_commitments, const uint8_t *d_proofs, int n_total, Fr *d_z, Fr *d_zpow,
                                    uint8_t *d_records, hipStream_t st);
void launch_eval(const uint8_t *d_blobs, const Fr *d_z, const Fr *d_zpow, DeviceTables t, int n_total, int n_per_group, Fr *d_y /* may be null */,
                 uint8_t *d_records /* y written at +80; may be null */, int *d_err, hipStream_t st);
// stage 2 (per group of n records): points from records, r-powers, lincomb, pairing
// few commitments (compute_blob_kzg_proof): the subgroup ladder from x alone (beside the square root of the decoding), then the test once y is there
void launch_subgroup_ladder_from_x(const uint8_t *d_commitments, int stride, int n, G1Jac *d_T, hipStream_t st);
void launch_subgroup_finish(const G1Affine *d_pts, const G1Jac *d_T, int n, int *d_err, hipStream_t st);
void launch_points_from_records(const uint8_t *d_records, int n_total, int n_per_group, G1Affine *d_pts, int *d_err, hipStream_t st);
void launch_rpowers(const uint8_t *d_records, int n_per_group, int groups, int check_zy, uint32_t *d_scal_a, uint32_t *d_scal_b,
                    uint32_t *d_scal_c, int *d_err, hipStream_t st, int n_fe = N_FE /* the u64be(FIELD_ELEMENTS_PER_BLOB) field of the transcript */,
                    int lanes_from = 1024 /* batches from which the hash runs one lane per batch (k_rhash_lanes) */,
                    int have_digest = 0 /* 1: the transcript digests are already in d_scal_c (8 little-endian words per batch: hashed on the host) */);
void launch_lincomb(const G1Affine *d_pts, const uint32_t *d_scal_a, const uint32_t *d_scal_b, const uint32_t *d_scal_c,
                    int n_per_group, int groups, G1Jac *d_partials /* lincomb_partials_bytes() */, PairPt *d_pair_pts /* [group][2]: -proof_lincomb, rhs */,
                    hipStream_t st);
size_t lincomb_partials_bytes(int n_per_group, int groups);
// n_per_group == 1 with many groups (the *_many forms of the single-proof functions): rhs = C + [z] proof - [y] G, four lanes per check
void launch_lincomb_single(const G1Affine *d_pts, const uint32_t *d_scal_b, const uint32_t *d_scal_c, int groups, void *d_scratch /* lincomb_single_bytes() */,
                           PairPt *d_pair_pts, hipStream_t st);
size_t lincomb_single_bytes(int groups);
// bucket-method (Pippenger) form of the same sums, for many batches in flight; n_per_group <= 4096 (item indices are 15-bit)
void launch_lincomb_buckets(const G1Affine *d_pts, const uint32_t *d_scal_a, const uint32_t *d_scal_b, const uint32_t *d_scal_c,
                            int n_per_group, int groups, void *d_scratch /* lincomb_buckets_scratch_bytes() */, PairPt *d_pair_pts, hipStream_t st,
                            int stage = 0 /* 0: all three kernels; 1 prep, 2 buckets, 3 horner (per-kernel timing) */,
                            int chain_from = 6144 /* batches from which the tail is k_lc_wsum + k_lc_hchain instead of k_lc_horner */,
                            G1Jac *d_q = nullptr /* what launch_validate_points left for these points: the quarters form (four 64-bit scalars per term,
                                                    6-bit windows; lincomb_quarters_fit(n_per_group) must hold); stage 1 makes them affine IN PLACE */);
size_t lincomb_buckets_scratch_bytes(int n_per_group, int groups, bool quarters = false);
bool lincomb_quarters_fit(int n_per_group);
// pre-shifted form for few batches: launch_lincomb_preshift needs only the validated points (it can run beside the Fiat-Shamir
// hash), launch_lincomb_preshifted finishes once the r powers exist.  d_scratch: lincomb_buckets_scratch_bytes().
bool lincomb_preshift_fits(int n_per_group, int groups);
size_t lincomb_preshift_bytes(int n_per_group, int groups);
void launch_lincomb_preshift(const G1Affine *d_pts, int n_per_group, int groups, G1Jac *d_shifts, hipStream_t st);
// the same chains straight from the compressed inputs (x only: they do not wait for the square root of the decompression)
void launch_lincomb_preshift_bytes(const uint8_t *d_commitments, const uint8_t *d_proofs, int stride, int n_per_group, int groups, G1Jac *d_shifts,
        hipStream_t st);
void launch_lincomb_preshifted(const G1Affine *d_pts, const G1Jac *d_shifts, const uint32_t *d_scal_a, const uint32_t *d_scal_b, const uint32_t *d_scal_c,
                               int n_per_group, int groups, void *d_scratch, PairPt *d_pair_pts, hipStream_t st,
                                       int stage = 0 /* 1: digits only; 2: sums only */);
// Stage 2 for batches of different sizes in one launch set (kzg355_verify_blob_kzg_proof_batch_many_sets).  Stage 1 has run with one blob per
// "batch": records blob after blob, points as [C_i, proof_i] pairs at 2 i, 2 i + 1, one error word per blob.  d_goff (groups + 1 ints) holds
// the blobs before each batch and must be STRICTLY increasing (the host drops empty batches); n_total = d_goff[groups].  Batch g's scalars go to
// d_scal_a / d_scal_b at 8 (d_goff[g] + i) and to d_scal_c at 8 g; its 2 (3 n_g + 1) lincomb items start at 2 (3 d_goff[g] + g).
void launch_err_fold_sets(const int *d_blob_err, const int *d_goff, int groups, int *d_err /* per batch: or-ed into */, hipStream_t st);
void launch_rpowers_sets(const uint8_t *d_records, const int *d_goff, int groups, int check_zy, uint32_t *d_scal_a, uint32_t *d_scal_b, uint32_t *d_scal_c,
                         int *d_err, hipStream_t st, int n_fe, int lanes_from, int have_digest);
size_t lincomb_sets_bytes(size_t n_total, size_t groups);
void launch_lincomb_sets(const G1Affine *d_pts, const uint32_t *d_scal_a, const uint32_t *d_scal_b, const uint32_t *d_scal_c, const int *d_goff, int n_total,
                         int groups, void *d_scratch /* lincomb_sets_bytes() */, PairPt *d_pair_pts, hipStream_t st);
void launch_dump_intermediates_sets(const uint32_t *d_scal_a, const PairPt *d_pair_pts, const int *d_goff, int groups, uint8_t *d_out /* [groups][128] */,
                                    hipStream_t st);
void launch_pairing(const PairPt *d_pair_pts, DeviceTables t, int groups, int *d_ok, hipStream_t st,
                    int two_wave_upto = 256 /* batches up to which the two Miller loops of a check run on two waves */,
                    Fp *d_f12 = nullptr /* groups * 12 Fp of scratch */,
                            int hard12_from = 0 /* batches from which the hard part runs twelve lanes per check; 0: never */,
                    int miller_segments = 0 /* few batches: segments per Miller loop, 2 waves each (1: the two-wave kernel; 0: the default, 2) */);
size_t pairing_f12_bytes(int groups);
void launch_pairing_lane(const PairPt *d_pair_pts, DeviceTables t, int groups, int *d_ok, hipStream_t st);   // one lane per batch (A/B, tests)

// ---- k_pairing.hip
void launch_lines_to_w(DeviceTables t, hipStream_t st);

// ---- k_msm_wide.hip
size_t wide_table_bytes(WideShape ws);
int build_wide_table(DeviceTables t, hipStream_t st);                 // needs t.msm_table; 0 on success
int msm_wide_partials_per_blob(int n);
// scalars from blobs (canonical check fused, err per blob) or, if d_scalars != null, from Montgomery field elements
void launch_msm_wide(const uint8_t *d_blobs, const Fr *d_scalars, DeviceTables t, int n, G1Jac *d_partials /* [n][msm_wide_partials_per_blob(n)] */,
                     int *d_err, hipStream_t st);
// ---- k_msm.hip
void launch_digits_from_blobs(const uint8_t *d_blobs, int n, uint8_t *d_digits /* [n][32][4096] */, int *d_err /* per blob */, hipStream_t st);
void launch_digits_from_fr(const Fr *d_scalars /* [n][4096] Montgomery */, int n, uint8_t *d_digits, hipStream_t st);
void launch_msm_bucket(const uint8_t *d_digits, DeviceTables t, int n, G1Jac *d_partials /* [n][32] */, hipStream_t st);
void launch_msm_finalize(const G1Jac *d_partials, int n, uint8_t *d_out48 /* [n][48] */, hipStream_t st, int ppb = 0 /* partials per blob; 0: bucket form */);

// ---- k_small.hip: handles with 4 <= FIELD_ELEMENTS_PER_BLOB <= 64 (minimal preset); t.msm_table holds the n bit-reversed points
constexpr int SMALL_N_MIN = 4, SMALL_N_MAX = 64;
void launch_lagrange_from_monomial(const uint8_t *d_mono, int n, uint8_t *d_out /* n*48 */, int *d_err, hipStream_t st);
void launch_setup_small(const uint8_t *d_g1_bytes, int n, DeviceTables t, int *d_err, hipStream_t st);
void launch_small_records(const uint8_t *d_blobs, const uint8_t *d_c, const uint8_t *d_p /* may be null */, int n_total, int npg, DeviceTables t,
        Fr *d_z /* may be null */,
                          uint8_t *d_records /* may be null */, int *d_err /* per group */, hipStream_t st);
void launch_small_commit(const uint8_t *d_blobs, int n_blobs, DeviceTables t, uint8_t *d_out48, int *d_err /* per blob */, hipStream_t st);
// proofs at d_z (Montgomery, one per blob) or, if d_c != null, at each blob's own Fiat-Shamir challenge; d_y32 (32-byte y per blob) may be null
void launch_small_proof(const uint8_t *d_blobs, const uint8_t *d_c, const Fr *d_z, int n_blobs, DeviceTables t, uint8_t *d_out48, uint8_t *d_y32, int *d_err,
        hipStream_t st);

// ---- k_prove.hip
// quotient polynomial q(X) = (p(X) - y)/(X - z) in evaluation form (kzg.rs:461-523) for n blobs; also y.
// d_q: the quotient of every blob in the BLOB format (n x 131,072 bytes: 4096 canonical 32-byte big-endian integers; 16-byte aligned) -- the fixed-base MSM
// reads it like a blob; d_scratch: quotient_scratch_bytes(n) of device memory; form: 0 by size, 2 / 4 / 6 = 2^form leaves per lane.  Non-zero: a HIP call
// failed.
size_t quotient_scratch_bytes(int n);
int launch_quotient(const uint8_t *d_blobs, const Fr *d_z, DeviceTables t, int n, Fr *d_y, uint8_t *d_q /* [n][131072] */, void *d_scratch, int *d_err,
        hipStream_t st,
                    int form = 0);
void launch_fr_from_bytes(const uint8_t *d_in32, int n, Fr *d_out, int *d_err /* per element, ERR_NONCANONICAL_FR */, hipStream_t st);
void launch_fr_to_bytes(const Fr *d_in, int n, uint8_t *d_out32, hipStream_t st);
void launch_status_words(const int *d_err, const int *d_ok /* or null */, int32_t *d_words, int groups, hipStream_t st);

// ---- k_point_eval.hip: the front of the point-evaluation precompile (point_eval.h has the byte layout), one lane per input
// d_inputs: n * 192 bytes, versioned_hash | z | y | commitment | proof, 16-byte aligned and only read; d_records: n * RECORD_BYTES, 16-byte aligned;
// d_match[i] = 1 when input i's versioned hash is 0x01 || sha256(commitment)[1:], else 0
void launch_pe_unpack(const uint8_t *d_inputs, int n, uint8_t *d_records, int *d_match, hipStream_t st);
// d_out[32 i ..] = 0x01 || sha256(d_commitments[48 i ..])[1:]; d_commitments 4-byte, d_out 16-byte aligned
void launch_versioned_hash(const uint8_t *d_commitments, int n, uint8_t *d_out, hipStream_t st);

// ---- k_cells.hip: verify_cell_kzg_proof_batch (EIP-7594 cells of the 2x extended blob; mainnet handles only)
constexpr int CELL_FE = 64;                // FIELD_ELEMENTS_PER_CELL
constexpr int CELL_BYTES = CELL_FE * 32;   // BYTES_PER_CELL
constexpr int CELLS_PER_EXT_BLOB = 128;
constexpr int CELL_DEBUG_BYTES = 32 + 3 * 48;   // r | [I(tau)]_1 | LL | RL per group
// lincomb terms of a group of n cells: n unique-commitment slots (padded), n proofs (RL), 64 monomial points, n proofs (LL)
KZG_HD int cell_terms(int npg) { return 3 * npg + CELL_FE; }
struct CellConsts {
    Fr h64[CELLS_PER_EXT_BLOB];                // h_c^64, h_c = w^rev7(c), w = 7^((r-1)/8192)
    Fr shift[CELLS_PER_EXT_BLOB][CELL_FE];     // h_c^-t / 64
    Fr tw[CELL_FE];                            // w64^-j, w64 = w^128
};
// once per handle: the constants and the Miller-loop lines of setup g2[64] into slot 2 of d_lines / d_lines_inf (bad g2 bytes: ERR_SETUP_POINT in d_err)
void launch_cell_setup(const uint8_t *d_g2_tau64, CellConsts *d_cc, LineCoeff *d_lines, int *d_lines_inf, int *d_err, hipStream_t st);
// r per group (from the host digests), r^(k0 + k) (d_rpow: npg * groups), the proof scalars and the unique-commitment weights into d_scal
// ([group][cell_terms(npg)][8 words]); d_r_be: 32 bytes of r per group.  k0: where in its group the first of the npg cells sits (0 for whole groups)
void launch_cell_scalars(const uint8_t *d_digests, const int *d_cell_idx, const int *d_cidx, int npg, int groups, int k0, const CellConsts *d_cc,
                         Fr *d_rpow, uint32_t *d_scal, uint8_t *d_r_be, hipStream_t st);
// column sums, inverse DFT and shift per (group, column) segment (d_segs: group, column, first entry of d_perm, count), then I per group into d_scal;
// d_coef: n_segs * 64 Fr; non-canonical cell elements set ERR_NONCANONICAL_FR in their group's d_err
void launch_cell_interp(const uint8_t *d_cells, const int *d_perm, const int4 *d_segs, int n_segs, const int *d_gseg /* groups + 1 */, const Fr *d_rpow,
                        const CellConsts *d_cc, int npg, int groups, Fr *d_coef, uint32_t *d_scal, int *d_err, hipStream_t st);
// the two sums per group -> d_pair_pts (-LL, RL); d_partials: cell_terms(npg) * groups G1Jac, d_sums: 3 * groups G1Jac; d_dbg (or null): CELL_DEBUG_BYTES
// per group
void launch_cell_lincomb(const G1Affine *d_pts, const G1Affine *d_mono, const uint32_t *d_scal, int npg, int groups, G1Jac *d_partials, G1Jac *d_sums,
                         const uint8_t *d_r_be, PairPt *d_pair_pts, uint8_t *d_dbg, hipStream_t st);
// a group cut into blocks of cells over several devices: the first half of launch_cell_lincomb on one block of every group (its three sums per
// group into d_sums), and the second half over the sums of all blocks on the group's stage-2 device.  d_parts: [group][block][3] G1Jac,
// blocks <= CELL_MERGE_MAX_BLOCKS; r of group j at d_r_be + 32 (r_first + j r_stride); d_pair_pts, d_dbg as above
void launch_cell_sums(const G1Affine *d_pts, const G1Affine *d_mono, const uint32_t *d_scal, int npg, int groups, G1Jac *d_partials, G1Jac *d_sums,
                      hipStream_t st);
// false (nothing launched): more blocks than the one wave of k_cell_merge adds
constexpr int CELL_MERGE_MAX_BLOCKS = 64;
bool launch_cell_merge(const G1Jac *d_parts, int blocks, int groups, const uint8_t *d_r_be, int r_first, int r_stride, PairPt *d_pair_pts, uint8_t *d_dbg,
                       hipStream_t st);
// Groups of different sizes in one launch set (kzg355_verify_cell_kzg_proof_batch_many_sets): cells are numbered group after group, d_goff
// (groups + 1 ints) holds the cells before each group and must be STRICTLY increasing (the host drops empty groups), d_cgrp (n_cells ints) the
// group of each cell.  Group g's points start at 2 d_goff[g] and its cell_terms(count) lincomb terms at 3 d_goff[g] + 64 g, in the uniform
// form's order; d_scal and d_partials hold cell_terms_sets(n_cells, groups) terms.  The bodies are those of the uniform kernels (group_geo.h).
// (int: at most 2^18 cells in at most 2^18 groups are 67 * 2^18 terms)
KZG_HD int cell_terms_sets(int n_cells, int groups) { return 3 * n_cells + CELL_FE * groups; }
void launch_cell_scalars_sets(const uint8_t *d_digests, const int *d_cell_idx, const int *d_cidx, const int *d_goff, const int *d_cgrp, int n_cells,
                              const CellConsts *d_cc, Fr *d_rpow, uint32_t *d_scal, uint8_t *d_r_be, hipStream_t st);
void launch_cell_interp_sets(const uint8_t *d_cells, const int *d_perm, const int4 *d_segs, int n_segs, const int *d_gseg, const Fr *d_rpow,
                             const CellConsts *d_cc, const int *d_goff, int groups, Fr *d_coef, uint32_t *d_scal, int *d_err, hipStream_t st);
void launch_cell_lincomb_sets(const G1Affine *d_pts, const G1Affine *d_mono, const uint32_t *d_scal, const int *d_goff, int n_cells, int groups,
                              G1Jac *d_partials, G1Jac *d_sums, const uint8_t *d_r_be, PairPt *d_pair_pts, uint8_t *d_dbg, hipStream_t st);
// validate_kzg_g1 on such a launch set's points (k_cell_points.hip): launch_decompress_points and launch_subgroup_points with the slots and the error
// words of the ragged layout; d_commitments holds n_cells unique-commitment slots, group after group
void launch_cell_points_sets(const uint8_t *d_commitments, const uint8_t *d_proofs, const int *d_goff, const int *d_cgrp, int n_cells, G1Affine *d_pts,
                             int *d_err, hipStream_t st);
// ---- k_cell_prep.hip: what the host prepares per group of a cell batch, from inputs that are in HBM already (the *_device entry points)
constexpr int CELL_PREP_LDS_SLOTS = 8192;      // slots of the dedup table k_cell_prep keeps in LDS; a larger table lives in d_gtab
constexpr int CELL_PREP_MAX_CELLS = 16384;     // cells per group up to which the device prepares (128 blobs x 128 cells: a block as one batch)
// slots of a group's dedup table: a power of two >= 2 npg
KZG_HD int cell_prep_table_slots(int npg) { int t = 2; while (t < 2 * npg) t <<= 1; return t; }
// d_commitments / d_indices: the caller's (16- / 8-byte aligned).  Out: d_uc (unique commitments per group in first-appearance order, padded to npg
// with the encoding of infinity), d_ucount[g], d_cell (clamped indices; an index >= 128 sets ERR_CELL_INDEX in d_err[g]), d_cidx, d_perm, and
// the segment list with a fixed min(npg, 128) slots per group (d_gseg[g] = g * that; empty segments have count 0).  d_gtab: groups * tab_size
// ints when tab_size > CELL_PREP_LDS_SLOTS, unused otherwise.
void launch_cell_prep(const uint8_t *d_commitments, const size_t *d_indices, int npg, int groups, int tab_size, int *d_gtab, uint8_t *d_uc, int4 *d_segs,
                      int *d_gseg, int *d_cell, int *d_cidx, int *d_perm, int *d_ucount, int *d_err, hipStream_t st);
// The same for groups of different sizes (kzg355_verify_cell_kzg_proof_batch_many_sets_device), one workgroup per group: group g is cells
// d_goff[g] .. d_goff[g + 1] - 1 (d_goff: groups + 1 ints, strictly increasing, each group at most CELL_PREP_MAX_CELLS cells) and its segment
// slots start at d_gseg[g], the sum of min(count, 128) over the groups before it -- both uploaded by the host, which has the counts.  Out: what
// launch_cell_prep leaves, d_uc padded to every group's own count, d_perm in cell numbers of the launch set, and d_cgrp, the group of every
// cell.  d_gtab: 4 ints per cell of the launch set when some group's table exceeds CELL_PREP_LDS_SLOTS (group g's at 4 d_goff[g]), else unused.
void launch_cell_prep_sets(const uint8_t *d_commitments, const size_t *d_indices, const int *d_goff, const int *d_gseg, int groups, int *d_gtab,
                           uint8_t *d_uc, int4 *d_segs, int *d_cell, int *d_cidx, int *d_perm, int *d_cgrp, int *d_ucount, int *d_err, hipStream_t st);
// the transcript digests (32 bytes per group, as launch_cell_scalars takes them), gathered from the caller's buffers; lanes: one lane per group
// (many groups), else one wave per group
void launch_cell_rhash(const uint8_t *d_uc, const size_t *d_indices, const uint8_t *d_cells, const uint8_t *d_proofs, const int *d_cidx, const int *d_ucount,
                       int npg, int groups, bool lanes, uint8_t *d_digests, hipStream_t st);
// the same for groups of different sizes: group g is cells d_goff[g] .. d_goff[g + 1] - 1 of the launch set (d_goff: groups + 1 ints, strictly
// increasing), every array cell-major as above; each group at most CELL_PREP_MAX_CELLS cells
void launch_cell_rhash_sets(const uint8_t *d_uc, const size_t *d_indices, const uint8_t *d_cells, const uint8_t *d_proofs, const int *d_cidx,
                            const int *d_ucount, const int *d_goff, int groups, bool lanes, uint8_t *d_digests, hipStream_t st);
// ---- k_blob_cells.hip: verify_blob_cell_proofs_batch -- groups of n blobs, each with all its 128 cells in cell order (npg = 128 n)
// What the preparation leaves, from d_pos (groups * n: the position of each blob's commitment among its group's unique ones), d_ucount (how many
// those are) and d_uc_in (groups * n * 48: the unique commitments of a group first): d_cell, d_cidx, d_uc (padded to npg per group with the
// encoding of infinity), d_gseg, d_indices (or null: the index array launch_cell_rhash reads) and, with columns, the column sort (d_segs: 128 per
// group, d_perm); without, d_gseg counts the 64 segments per group of launch_blob_cell_coefs.  d_blob_err (per blob) is folded into d_err (per group).
void launch_blob_cell_meta(const int *d_pos, const int *d_ucount, const uint8_t *d_uc_in, const int *d_blob_err, int n, int groups, bool columns, int4 *d_segs,
                           int *d_gseg, int *d_cell, int *d_cidx, int *d_perm, size_t *d_indices, uint8_t *d_uc, int *d_err, hipStream_t st);
struct CellComputeConsts;
// the interpolation from the blobs' coefficients (d_f: groups * n * 4096 Fr as launch_cc_field leaves them; d_rpow as launch_cell_scalars does):
// d_W: groups * 64 Fr, d_coef: groups * 64 * 64 Fr in launch_cell_interp's segment layout (which finishes with n_segs = 0)
void launch_blob_cell_coefs(const Fr *d_f, const Fr *d_rpow, const CellComputeConsts *d_cc, int n, int groups, Fr *d_W, Fr *d_coef, hipStream_t st);
// Groups of different blob counts (kzg355_verify_blob_cell_proofs_batch_many_sets), in the `_sets` layout above: every group has 128 cells per
// blob, so d_goff / d_cgrp (cells) give the blobs too -- d_goff[g] / 128 blobs lie before group g, and d_pos, d_uc_in, d_blob_err and d_f are
// indexed by them, blob after blob with no padding.  Everything else as in the two launchers above.
void launch_blob_cell_meta_sets(const int *d_pos, const int *d_ucount, const uint8_t *d_uc_in, const int *d_blob_err, const int *d_goff, const int *d_cgrp,
                                int n_cells, int groups, bool columns, int4 *d_segs, int *d_gseg, int *d_cell, int *d_cidx, int *d_perm, size_t *d_indices,
                                uint8_t *d_uc, int *d_err, hipStream_t st);
void launch_blob_cell_coefs_sets(const Fr *d_f, const Fr *d_rpow, const CellComputeConsts *d_cc, const int *d_goff, int groups, Fr *d_W, Fr *d_coef,
                                 hipStream_t st);


// ---- k_cell_compute.hip: compute_cells_and_kzg_proofs (the cells of the 2x extension and their proofs by FK20; mainnet handles only)
constexpr int CC_FFT = 128;                                  // size of the circulant transforms (2 x 64)
constexpr int CC_POINTS = CELL_FE * CC_FFT;                  // X_r[i]: the fixed-base points, 8192
constexpr int CC_WINDOWS = 64, CC_DIGITS = 8;                // comb table: signed 4-bit digits, multiples 1..8 of 16^w X per window
constexpr size_t CC_TABLE_ENTRIES = (size_t)CC_POINTS * CC_WINDOWS * CC_DIGITS;   // 4,194,304 affine points, 384 MiB
struct CellComputeConsts {
    Fr w4096[N_FE];                                          // w4096^e, natural order (w4096^-e = w4096[4096 - e])
    Fr w8192, inv128, inv4096;                               // w = 7^((r-1)/8192), 1/128, 1/4096
    uint32_t tw_a[CC_FFT][4], tw_b[CC_FFT][4];               // GLV halves of w128^e (w128 = w4096^32): w128^e = a + b x^2
};
void launch_cc_consts(const Fr *d_roots, CellComputeConsts *d_cc, hipStream_t st);
// monomial points [tau^t]_1, t = t0 .. t0 + 63, compressed into d_out48 + 48 t0 (8-bit fixed-base MSM over the Lagrange table), for the setups of
// all three cell paths.  Scratch: d_scal 64 * 4096 Fr, d_digits 64 * 32 * 4096 bytes, d_partials 64 * 32 G1Jac.
void launch_monomial_chunk(DeviceTables t, int t0, Fr *d_scal, uint8_t *d_digits, G1Jac *d_partials, uint8_t *d_out48, hipStream_t st);
// count compressed points -> affine (a point that does not decode: infinity and ERR_SETUP_POINT in d_err)
void launch_monomial_decode(const uint8_t *d_mono48, int count, G1Affine *d_mono, int *d_err, hipStream_t st);
// from the 4096 monomial points: X_r = NTT128(x_r) (d_X: CC_POINTS G1Jac) and the comb table (d_tab: CC_TABLE_ENTRIES)
void launch_cc_setup_points(const G1Affine *d_mono, const CellComputeConsts *d_cc, G1Jac *d_X, G1Affine *d_tab, hipStream_t st);
// per call: field stage (d_coef: n * 4096 Fr or null; d_cells: n * 128 * 2048 bytes or null; non-canonical elements -> ERR_NONCANONICAL_FR in d_err[blob]),
// columns (d_scal: n * 128 * 64 * 8 words), fixed-base sums (d_Z: n * 128 G1Jac), G1 transforms (d_proofs48: n * 128 * 48; d_h_dbg: n * 64 * 48 or null)
void launch_cc_field(const uint8_t *d_blobs, int n, const CellComputeConsts *d_cc, Fr *d_coef, uint8_t *d_cells, int *d_err, hipStream_t st);
void launch_cc_columns(const Fr *d_coef, int n, const CellComputeConsts *d_cc, uint32_t *d_scal, hipStream_t st);
void launch_cc_msm(const uint32_t *d_scal, int n, const G1Affine *d_tab, G1Jac *d_Z, hipStream_t st);
// d_commit48 (or null): the blobs' commitments, conv[63] of the same chain, [n][48]; d_proofs48 may be null when d_h_dbg is too (commitments only)
void launch_cc_proofs(const G1Jac *d_Z, int n, const CellComputeConsts *d_cc, uint8_t *d_proofs48, uint8_t *d_h_dbg, uint8_t *d_commit48, hipStream_t st);

// ---- k_cell_quotient.hip: compute_cell_kzg_proofs_at, the proofs of chosen cells (mainnet handles only)
// d_coef and d_err (per blob of the chunk) as launch_cc_field leaves them; d_scal: pairs * 4096 Fr, Montgomery, in blob order -- the d_scalars of
// launch_msm_wide / launch_digits_from_fr (zeros for a blob whose error word is set)
void launch_cq_quotient(const Fr *d_coef, const CqPair *d_pairs, int pairs, const int *d_err, const CellComputeConsts *d_cc, Fr *d_scal, hipStream_t st);
// d_cells as launch_cc_field leaves them (128 cells per blob of the chunk); pair p's cell goes to d_out + 2048 * d_pairs[p].slot
void launch_cq_gather(const uint8_t *d_cells, const CqPair *d_pairs, int pairs, uint8_t *d_out, hipStream_t st);

// ---- k_point_quotient.hip: compute_kzg_proofs_at, openings of blobs at chosen points (mainnet handles only)
// d_coef and d_err (per blob of the chunk) as launch_cc_field leaves them; d_zs: the pairs' points, Montgomery, in pair order.  d_ys (or null):
// pair p's y = p(z), 32 canonical bytes, at d_ys + 32 * d_pairs[p].slot.  d_scal (or null: no quotient is formed): pairs * 4096 Fr, Montgomery, in
// blob order, as launch_cq_quotient leaves them
void launch_pq_quotient(const Fr *d_coef, const PqPair *d_pairs, const Fr *d_zs, int pairs, const int *d_err, const CellComputeConsts *d_cc, Fr *d_scal,
                        uint8_t *d_ys, hipStream_t st);

// ---- k_cell_recover.hip: the field stage of recover_cells_and_kzg_proofs (64..128 known cells -> coefficients and all 128 cells; mainnet handles only)
struct RecoverTables {                                        // one per distinct index set of a chunk
    Fr sd[CELLS_PER_EXT_BLOB];                               // S(a_k) / (64 * 128), S the vanishing polynomial of the missing cells' a_m
    Fr sci[CELLS_PER_EXT_BLOB];                              // 1 / (128 S(w a_k))
    int pos[CELLS_PER_EXT_BLOB];                             // cell k's place in the set's ascending index list, -1 if missing
};
// workgroup per set of the chunk: pos, sd and sci of d_rt[set] from the set's 128-bit mask (d_masks[2 set] bits 0..63, d_masks[2 set + 1] bits 64..127)
void launch_rc_vanish(const CellComputeConsts *d_cc, const uint64_t *d_masks, int sets, RecoverTables *d_rt, hipStream_t st);
// d_cells: the known cells of the chunk's m blobs (blob b: d_blobs[b].first onwards, in the order of its index list); d_u: m * 128 * 64 Fr
// ([blob][cell][column]); non-canonical elements -> ERR_NONCANONICAL_FR in d_err[blob]
void launch_rc_interp(const uint8_t *d_cells, const RecoverBlob *d_blobs, int m, const CellComputeConsts *d_cc, const RecoverTables *d_rt, Fr *d_u,
                      int *d_err, hipStream_t st);
// d_coef (or null): m * 4096 Fr, the layout launch_cc_columns reads (zero for a refused blob); want_cells: d_u receives P_r(a_k) for all 128 cells
void launch_rc_columns(Fr *d_u, const RecoverBlob *d_blobs, int m, const CellComputeConsts *d_cc, const RecoverTables *d_rt, Fr *d_coef,
                       bool want_cells, hipStream_t st);
// a refused blob's 128 output cells are left as they are
void launch_rc_cells(const Fr *d_u, const RecoverBlob *d_blobs, int m, const CellComputeConsts *d_cc, uint8_t *d_cells /* m * 128 * 2048 */,
                     hipStream_t st);
// ---- k_cell_recover_at.hip: recover_cells_and_kzg_proofs_at, the chosen cells of recovered blobs
// d_u as launch_rc_columns leaves it with want_cells; pair p's cell (d_pairs[p].cell of the chunk's blob d_pairs[p].blob) goes to
// d_out + 2048 * d_pairs[p].slot; a pair of a refused blob writes nothing
void launch_rc_cells_at(const Fr *d_u, const RecoverBlob *d_blobs, const CqPair *d_pairs, int pairs, const CellComputeConsts *d_cc, uint8_t *d_out,
                        hipStream_t st);

}  // namespace kzg
