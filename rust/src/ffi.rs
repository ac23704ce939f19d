//! `extern "C"` block for include/kzg355.h -- the seam that replaces the 35 blst symbols the reference binds
//!.  One declaration per entry point of the header; bytes in, bytes out.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_long};

#[repr(C)]
pub struct kzg355_settings {
    _private: [u8; 0],
}

pub const KZG355_OK: c_int = 0;
pub const KZG355_BADARGS: c_int = 1;
pub const KZG355_INTERNAL: c_int = 2;
pub const KZG355_INVALID_BYTES_LENGTH: c_int = 3;
pub const KZG355_INVALID_HEX: c_int = 4;
pub const KZG355_INVALID_TRUSTED_SETUP: c_int = 5;
pub const KZG355_NO_DEVICE: c_int = 6;
pub const KZG355_NO_MEMORY: c_int = 7;
pub const KZG355_DEVICE_ERROR: c_int = 8;

/// `struct kzg355_options` (include/kzg355.h): same fields, same order.  Fill with `kzg355_options_default` first.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct kzg355_options {
    pub struct_size: usize,
    pub device: c_int,
    pub msm_bits: c_int,
    pub msm_require_wide: c_int,
    pub self_test: c_int,
    pub host_threads: c_int,
    pub host_hash: c_int,
    pub host_hash_max_blobs: c_int,
    pub host_sha: c_int,
    pub host_rhash: c_int,
    pub host_rhash_max_records: c_int,
    pub challenge_form: c_int,
    pub lincomb_form: c_int,
    pub pairing_lane: c_int,
    pub pairing_two_wave_upto: c_int,
    pub lc_chain_from: c_int,
    pub rhash_lanes_from: c_int,
    pub beside_max_blobs: c_int,
    pub split_parts: c_int,
    pub split_streams: c_int,
    pub chunk_mb: c_int,
    pub chunks_in_flight: c_int,
    pub staging_ring: c_int,
    pub exchange: c_int,
    pub verify_only: c_int,
    pub msm_glv: c_int,
    pub msm_eager: c_int,
    pub pairing_hard12_from: c_int,
    pub submit_sets: c_int,
    pub host_hash_device_max_blobs: c_int,
    pub quotient_form: c_int,
    pub miller_segments: c_int,
    pub force_multi: c_int,
    pub force_sharded: c_int,
}

extern "C" {
    pub fn kzg355_load_trusted_setup(g1: *const u8, n1: usize, g2: *const u8, n2: usize, out: *mut *mut kzg355_settings) -> c_int;
    pub fn kzg355_load_trusted_setup_devices(g1: *const u8, n1: usize, g2: *const u8, n2: usize, devices: *const c_int, n_devices: usize,
                                             out: *mut *mut kzg355_settings) -> c_int;
    pub fn kzg355_options_default(options: *mut kzg355_options);
    pub fn kzg355_options_from_env(options: *mut kzg355_options);
    pub fn kzg355_load_trusted_setup_ex(g1: *const u8, n1: usize, g2: *const u8, n2: usize, devices: *const c_int, n_devices: usize,
                                        options: *const kzg355_options, out: *mut *mut kzg355_settings) -> c_int;
    pub fn kzg355_load_trusted_setup_file(path: *const c_char, out: *mut *mut kzg355_settings) -> c_int;
    pub fn kzg355_lagrange_setup_from_monomial(out: *mut u8, monomial_g1: *const u8, n: usize) -> c_int;
    pub fn kzg355_free_trusted_setup(s: *mut kzg355_settings);

    pub fn kzg355_blob_to_kzg_commitment(out: *mut u8, blob: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_kzg_proof(proof: *mut u8, y: *mut u8, blob: *const u8, z: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_blob_kzg_proof(proof: *mut u8, blob: *const u8, commitment: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_kzg_proof(ok: *mut bool, commitment: *const u8, z: *const u8, y: *const u8, proof: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_kzg_proof(ok: *mut bool, blob: *const u8, commitment: *const u8, proof: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_kzg_proof_batch(ok: *mut bool, blobs: *const u8, n_blobs: usize, commitments: *const u8, n_commitments: usize,
                                              proofs: *const u8, n_proofs: usize, s: *const kzg355_settings) -> c_int;

    pub fn kzg355_blob_to_kzg_commitment_many(out: *mut u8, status: *mut c_int, blobs: *const u8, n: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_blob_kzg_proof_many(out: *mut u8, status: *mut c_int, blobs: *const u8, commitments: *const u8, n: usize,
                                              s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_kzg_proof_batch_many(ok: *mut bool, status: *mut c_int, blobs: *const u8, commitments: *const u8, proofs: *const u8,
                                                   n_per_group: usize, groups: usize, s: *const kzg355_settings) -> c_int;
    // EIP-7594 cells: commitments n*48, cell_indices n, cells n*2048, proofs n*48
    pub fn kzg355_verify_cell_kzg_proof_batch(ok: *mut bool, commitments: *const u8, cell_indices: *const usize, cells: *const u8, proofs: *const u8, n: usize,
                                              s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_cell_kzg_proof_batch_many(ok: *mut bool, status: *mut c_int, commitments: *const u8, cell_indices: *const usize, cells: *const u8,
                                                   proofs: *const u8, n_per_group: usize, groups: usize, s: *const kzg355_settings) -> c_int;
    // groups of different sizes: group g is cell_counts[g] entries of the four arrays, after those of group g - 1
    pub fn kzg355_verify_cell_kzg_proof_batch_many_sets(ok: *mut bool, status: *mut c_int, cell_counts: *const usize, commitments: *const u8,
                                                        cell_indices: *const usize, cells: *const u8, proofs: *const u8, groups: usize,
                                                        s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_cell_batch_intermediates_sets(out: *mut u8, ok: *mut bool, status: *mut c_int, cell_counts: *const usize, commitments: *const u8,
                                                      cell_indices: *const usize, cells: *const u8, proofs: *const u8, groups: usize,
                                                      s: *const kzg355_settings) -> c_int;
    // EIP-7594 cells and their proofs: cells_out 128*2048 (n*128*2048), proofs_out 128*48 (n*128*48), either may be null
    pub fn kzg355_compute_cells_and_kzg_proofs(cells_out: *mut u8, proofs_out: *mut u8, blob: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_cells_and_kzg_proofs_many(cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int, blobs: *const u8, n: usize,
                                                    s: *const kzg355_settings) -> c_int;
    // EIP-7594 recovery: cell_indices n (64..128, strictly ascending), cells n*2048 (m*n*2048, blob after blob, one index set for all blobs)
    pub fn kzg355_recover_cells_and_kzg_proofs(cells_out: *mut u8, proofs_out: *mut u8, cell_indices: *const usize, cells: *const u8, n: usize,
                                               s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_cells_and_kzg_proofs_many(cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int, cell_indices: *const usize, cells: *const u8,
                                                    n: usize, m: usize, s: *const kzg355_settings) -> c_int;
    // blob i known at cell_counts[i] cells: its indices and its cells follow those of blob i - 1 in cell_indices and cells
    pub fn kzg355_recover_cells_and_kzg_proofs_many_sets(cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int, cell_counts: *const usize,
                                                         cell_indices: *const usize, cells: *const u8, m: usize, s: *const kzg355_settings) -> c_int;
    // the cells of a blob at chosen indices and their proofs, each pair through its own quotient and one MSM: blob i asks for cell_counts[i] cells,
    // its indices follow those of blob i - 1 in cell_indices, and output slot j belongs to entry j of cell_indices
    pub fn kzg355_compute_cell_kzg_proofs_at(cells_out: *mut u8, proofs_out: *mut u8, blob: *const u8, cell_indices: *const usize, k: usize,
                                             s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_cell_kzg_proofs_at_many(cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int, blobs: *const u8, n: usize,
                                                  cell_counts: *const usize, cell_indices: *const usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_cell_kzg_proofs_at_many_device(d_cells_out: *mut u8, d_proofs_out: *mut u8, status: *mut c_int, d_blobs: *const u8, n: usize,
                                                         cell_counts: *const usize, cell_indices: *const usize, s: *const kzg355_settings) -> c_int;
    // openings of a blob at chosen points, each pair through its own quotient and one MSM: blob i is opened at point_counts[i] points, its points
    // (32 bytes each) follow those of blob i - 1 in zs, and output slot j receives the proof and y of point j of zs
    pub fn kzg355_compute_kzg_proofs_at(proofs_out: *mut u8, ys_out: *mut u8, blob: *const u8, zs: *const u8, k: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_kzg_proofs_at_many(proofs_out: *mut u8, ys_out: *mut u8, status: *mut c_int, blobs: *const u8, n: usize,
                                             point_counts: *const usize, zs: *const u8, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_kzg_proofs_at_many_device(d_proofs_out: *mut u8, d_ys_out: *mut u8, status: *mut c_int, d_blobs: *const u8, n: usize,
                                                    point_counts: *const usize, zs: *const u8, s: *const kzg355_settings) -> c_int;
    // chosen cells of recovered blobs and their proofs: the input of recover_cells_and_kzg_proofs_many_sets (blob i known at cell_counts[i] cells),
    // the output of compute_cell_kzg_proofs_at_many (blob i asks for want_counts[i] cells; output slot j belongs to entry j of want_indices)
    pub fn kzg355_recover_cells_and_kzg_proofs_at(cells_out: *mut u8, proofs_out: *mut u8, cell_indices: *const usize, cells: *const u8, n: usize,
                                                  want_indices: *const usize, k: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_cells_and_kzg_proofs_at_many_sets(cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int, cell_counts: *const usize,
                                                            cell_indices: *const usize, cells: *const u8, want_counts: *const usize,
                                                            want_indices: *const usize, m: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_cells_and_kzg_proofs_at_many_sets_device(d_cells_out: *mut u8, d_proofs_out: *mut u8, status: *mut c_int,
                                                                   cell_counts: *const usize, cell_indices: *const usize, d_cells: *const u8,
                                                                   want_counts: *const usize, want_indices: *const usize, m: usize,
                                                                   s: *const kzg355_settings) -> c_int;
    // the three cell calls on device-resident data: d_* are device pointers (byte buffers 16-byte aligned, indices 8-byte aligned); the index set
    // of the recovery stays in host memory; prep_form: 0 by shape, 1 device preparation, 2 host preparation
    pub fn kzg355_verify_cell_kzg_proof_batch_many_device(ok: *mut bool, status: *mut c_int, d_commitments: *const u8, d_cell_indices: *const usize,
                                                          d_cells: *const u8, d_proofs: *const u8, n_per_group: usize, groups: usize,
                                                          s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_cells_and_kzg_proofs_many_device(d_cells_out: *mut u8, d_proofs_out: *mut u8, status: *mut c_int, d_blobs: *const u8, n: usize,
                                                           s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_cells_and_kzg_proofs_many_device(d_cells_out: *mut u8, d_proofs_out: *mut u8, status: *mut c_int, cell_indices: *const usize,
                                                           d_cells: *const u8, n: usize, m: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_cells_and_kzg_proofs_many_sets_device(d_cells_out: *mut u8, d_proofs_out: *mut u8, status: *mut c_int, cell_counts: *const usize,
                                                                cell_indices: *const usize, d_cells: *const u8, m: usize,
                                                                s: *const kzg355_settings) -> c_int;
    // the compute and recover calls with the blobs' commitments (48 bytes per blob, slot 63 of the FK20 convolution) as one more output in front:
    // any of the three outputs may be null, not all; with commitments_out null they are the calls they are named after
    pub fn kzg355_compute_commitments_cells_and_kzg_proofs_many(commitments_out: *mut u8, cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int,
                                                                blobs: *const u8, n: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_commitments_cells_and_kzg_proofs_many_device(d_commitments_out: *mut u8, d_cells_out: *mut u8, d_proofs_out: *mut u8,
                                                                       status: *mut c_int, d_blobs: *const u8, n: usize,
                                                                       s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_commitments_cells_and_kzg_proofs_many(commitments_out: *mut u8, cells_out: *mut u8, proofs_out: *mut u8, status: *mut c_int,
                                                                cell_indices: *const usize, cells: *const u8, n: usize, m: usize,
                                                                s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_commitments_cells_and_kzg_proofs_many_device(d_commitments_out: *mut u8, d_cells_out: *mut u8, d_proofs_out: *mut u8,
                                                                       status: *mut c_int, cell_indices: *const usize, d_cells: *const u8, n: usize,
                                                                       m: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(commitments_out: *mut u8, cells_out: *mut u8, proofs_out: *mut u8,
                                                                     status: *mut c_int, cell_counts: *const usize, cell_indices: *const usize,
                                                                     cells: *const u8, m: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(d_commitments_out: *mut u8, d_cells_out: *mut u8, d_proofs_out: *mut u8,
                                                                            status: *mut c_int, cell_counts: *const usize,
                                                                            cell_indices: *const usize, d_cells: *const u8, m: usize,
                                                                            s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_cell_batch_intermediates_device(out: *mut u8, ok: *mut bool, status: *mut c_int, d_commitments: *const u8,
                                                        d_cell_indices: *const usize, d_cells: *const u8, d_proofs: *const u8, n_per_group: usize,
                                                        groups: usize, prep_form: c_int, s: *const kzg355_settings) -> c_int;
    // groups of different sizes on device-resident data: cell_counts stays in host memory, the four arrays hold the sum of the counts entries
    pub fn kzg355_verify_cell_kzg_proof_batch_many_sets_device(ok: *mut bool, status: *mut c_int, cell_counts: *const usize, d_commitments: *const u8,
                                                               d_cell_indices: *const usize, d_cells: *const u8, d_proofs: *const u8, groups: usize,
                                                               s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_cell_batch_intermediates_sets_device(out: *mut u8, ok: *mut bool, status: *mut c_int, cell_counts: *const usize,
                                                             d_commitments: *const u8, d_cell_indices: *const usize, d_cells: *const u8,
                                                             d_proofs: *const u8, groups: usize, prep_form: c_int, s: *const kzg355_settings) -> c_int;
    // blobs against their EIP-7594 cell proofs (the Fulu counterpart of verify_blob_kzg_proof_batch): blobs n*131072, commitments n*48, cell_proofs
    // n*128*48; interp_form: 0 what the call does, 1 from the blobs' coefficients, 2 the column kernel over the computed cells
    pub fn kzg355_verify_blob_cell_proofs_batch(ok: *mut bool, blobs: *const u8, n_blobs: usize, commitments: *const u8, n_commitments: usize,
                                                cell_proofs: *const u8, n_cell_proofs: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_cell_proofs_batch_many(ok: *mut bool, status: *mut c_int, blobs: *const u8, commitments: *const u8, cell_proofs: *const u8,
                                                     n_per_group: usize, groups: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_cell_proofs_batch_many_device(ok: *mut bool, status: *mut c_int, d_blobs: *const u8, d_commitments: *const u8,
                                                            d_cell_proofs: *const u8, n_per_group: usize, groups: usize,
                                                            s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_blob_cell_batch_intermediates(out: *mut u8, ok: *mut bool, status: *mut c_int, blobs: *const u8, commitments: *const u8,
                                                      cell_proofs: *const u8, n_per_group: usize, groups: usize, interp_form: c_int,
                                                      s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_blob_cell_batch_intermediates_device(out: *mut u8, ok: *mut bool, status: *mut c_int, d_blobs: *const u8, d_commitments: *const u8,
                                                             d_cell_proofs: *const u8, n_per_group: usize, groups: usize, interp_form: c_int,
                                                             prep_form: c_int, s: *const kzg355_settings) -> c_int;
    // groups of different blob counts: blob_counts (host, `groups` entries), the three arrays group after group with no padding
    pub fn kzg355_verify_blob_cell_proofs_batch_many_sets(ok: *mut bool, status: *mut c_int, blob_counts: *const usize, blobs: *const u8,
                                                          commitments: *const u8, cell_proofs: *const u8, groups: usize,
                                                          s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_cell_proofs_batch_many_sets_device(ok: *mut bool, status: *mut c_int, blob_counts: *const usize, d_blobs: *const u8,
                                                                 d_commitments: *const u8, d_cell_proofs: *const u8, groups: usize,
                                                                 s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_blob_cell_batch_intermediates_sets(out: *mut u8, ok: *mut bool, status: *mut c_int, blob_counts: *const usize, blobs: *const u8,
                                                           commitments: *const u8, cell_proofs: *const u8, groups: usize, interp_form: c_int,
                                                           s: *const kzg355_settings) -> c_int;
    pub fn kzg355_debug_blob_cell_batch_intermediates_sets_device(out: *mut u8, ok: *mut bool, status: *mut c_int, blob_counts: *const usize,
                                                                  d_blobs: *const u8, d_commitments: *const u8, d_cell_proofs: *const u8, groups: usize,
                                                                  interp_form: c_int, prep_form: c_int, s: *const kzg355_settings) -> c_int;
    // verify_blob_kzg_proof_batch on batches of different blob counts: blob_counts (host, `groups` entries), the three arrays batch after batch
    pub fn kzg355_verify_blob_kzg_proof_batch_many_sets(ok: *mut bool, status: *mut c_int, blob_counts: *const usize, blobs: *const u8,
                                                        commitments: *const u8, proofs: *const u8, groups: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_kzg_proof_batch_many_sets_device(ok: *mut bool, status: *mut c_int, blob_counts: *const usize, d_blobs: *const u8,
                                                               d_commitments: *const u8, d_proofs: *const u8, groups: usize,
                                                               s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_kzg_proof_many(ok: *mut bool, status: *mut c_int, commitments: *const u8, zs: *const u8, ys: *const u8, proofs: *const u8, n: usize,
                                        s: *const kzg355_settings) -> c_int;
    pub fn kzg355_verify_blob_kzg_proof_many(ok: *mut bool, status: *mut c_int, blobs: *const u8, commitments: *const u8, proofs: *const u8, n: usize,
                                             s: *const kzg355_settings) -> c_int;
    pub fn kzg355_compute_kzg_proof_many(proofs_out: *mut u8, ys_out: *mut u8, status: *mut c_int, blobs: *const u8, zs: *const u8, n: usize,
                                         s: *const kzg355_settings) -> c_int;
    // the EIP-4844 point-evaluation precompile: inputs n*192 (versioned_hash | z | y | commitment | proof); status and hash_match may be null;
    // the versioned hashes (n*32 from n*48) on host memory without a handle, or on device memory
    pub fn kzg355_kzg_to_versioned_hash_many(out: *mut u8, commitments: *const u8, n: usize) -> c_int;
    pub fn kzg355_kzg_to_versioned_hash_many_device(d_out: *mut u8, d_commitments: *const u8, n: usize, s: *const kzg355_settings) -> c_int;
    pub fn kzg355_point_evaluation_many(ok: *mut bool, status: *mut c_int, hash_match: *mut bool, inputs: *const u8, n: usize,
                                        s: *const kzg355_settings) -> c_int;
    pub fn kzg355_point_evaluation_many_device(ok: *mut bool, status: *mut c_int, hash_match: *mut bool, d_inputs: *const u8, n: usize,
                                               s: *const kzg355_settings) -> c_int;
    pub fn kzg355_point_evaluation(out: *mut u8, input: *const u8, input_len: usize, s: *const kzg355_settings) -> c_int;

    pub fn kzg355_settings_device(s: *const kzg355_settings) -> c_int;
    pub fn kzg355_settings_device_count(s: *const kzg355_settings) -> c_int;
    pub fn kzg355_settings_field_elements_per_blob(s: *const kzg355_settings) -> c_int;
    pub fn kzg355_settings_msm_form(s: *const kzg355_settings) -> c_int;
    pub fn kzg355_settings_msm_shape(s: *const kzg355_settings, bits: *mut c_int, windows: *mut c_int, glv: *mut c_int, table_bytes: *mut usize) -> c_int;
    pub fn kzg355_settings_build_msm_table(s: *const kzg355_settings) -> c_int;
    pub fn kzg355_settings_exchange_stats(s: *const kzg355_settings, allgathers: *mut c_long, peer_exchanges: *mut c_long) -> c_int;
    pub fn kzg355_settings_set_host_hash(s: *mut kzg355_settings, mode: c_int, max_blobs: c_int) -> c_int;
    pub fn kzg355_settings_host_hashed_calls(s: *const kzg355_settings) -> c_long;
    pub fn kzg355_settings_cell_device_prep_calls(s: *const kzg355_settings) -> c_long;
    pub fn kzg355_settings_cell_calls_per_device(s: *const kzg355_settings, out: *mut c_long, cap: usize) -> c_int;
    pub fn kzg355_settings_host_threads(s: *const kzg355_settings) -> c_int;
    pub fn kzg355_version() -> *const c_char;
}
