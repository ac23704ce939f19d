//! The public surface of the reference crate (src/kzg.rs:10-22, 28-79, 101-204, 983-1079) with every body forwarded through
//! `ffi` to libkzg355.so.  The byte newtypes raise their length / hex errors on this side, before any FFI call, exactly as the
//! reference's do; the engine decides everything else (Ok vs Err, the returned bytes, the verdicts).
use crate::consts::*;
use crate::ffi;
use std::ffi::CString;
use std::ops::{Deref, DerefMut};
use std::path::Path;

#[derive(Debug)]
pub enum Error {
    /// The supplied data is invalid in some way.
    BadArgs(String),
    /// Internal error - this should never occur (also: no usable HIP device, allocation failure; there is no CPU fallback).
    InternalError,
    /// The provided bytes are of incorrect length.
    InvalidBytesLength(String),
    /// Error when converting from hex to bytes.
    InvalidHexFormat(String),
    /// The provided trusted setup params are invalid.
    InvalidTrustedSetup(String),
}

fn check(rc: i32, what: &str) -> Result<(), Error> {
    match rc {
        ffi::KZG355_OK => Ok(()),
        ffi::KZG355_BADARGS => Err(Error::BadArgs(what.into())),
        ffi::KZG355_INVALID_BYTES_LENGTH => Err(Error::InvalidBytesLength(what.into())),
        ffi::KZG355_INVALID_HEX => Err(Error::InvalidHexFormat(what.into())),
        ffi::KZG355_INVALID_TRUSTED_SETUP => Err(Error::InvalidTrustedSetup(what.into())),
        _ => Err(Error::InternalError), // INTERNAL, NO_DEVICE, NO_MEMORY, DEVICE_ERROR: no reference counterpart (there is no CPU fallback)
    }
}

/// Opaque handle to the device-resident trusted setup; replaces the `Vec`s of the reference's `KzgSettings`.
#[derive(Debug)]
pub struct KzgSettings {
    raw: *mut ffi::kzg355_settings,
}
// The handle is immutable after creation and the engine takes a private workspace + stream per call.
unsafe impl Send for KzgSettings {}
unsafe impl Sync for KzgSettings {}

impl Drop for KzgSettings {
    fn drop(&mut self) {
        unsafe { ffi::kzg355_free_trusted_setup(self.raw) }
    }
}

impl KzgSettings {
    pub fn load_trusted_setup(g1_bytes: Vec<[u8; BYTES_PER_G1]>, g2_bytes: Vec<[u8; BYTES_PER_G2]>) -> Result<Self, Error> {
        let g1: Vec<u8> = g1_bytes.iter().flatten().copied().collect();
        let g2: Vec<u8> = g2_bytes.iter().flatten().copied().collect();
        let mut raw = std::ptr::null_mut();
        check(
            unsafe { ffi::kzg355_load_trusted_setup(g1.as_ptr(), g1_bytes.len(), g2.as_ptr(), g2_bytes.len(), &mut raw) },
            "load_trusted_setup",
        )?;
        Ok(Self { raw })
    }

    /// Extension: the handle spans several GPUs of the node; calls spread their work inside the library.
    pub fn load_trusted_setup_on_devices(g1_bytes: Vec<[u8; BYTES_PER_G1]>, g2_bytes: Vec<[u8; BYTES_PER_G2]>, devices: &[i32]) -> Result<Self, Error> {
        let g1: Vec<u8> = g1_bytes.iter().flatten().copied().collect();
        let g2: Vec<u8> = g2_bytes.iter().flatten().copied().collect();
        let mut raw = std::ptr::null_mut();
        check(
            unsafe {
                ffi::kzg355_load_trusted_setup_devices(g1.as_ptr(), g1_bytes.len(), g2.as_ptr(), g2_bytes.len(), devices.as_ptr(), devices.len(), &mut raw)
            },
            "load_trusted_setup_on_devices",
        )?;
        Ok(Self { raw })
    }

    /// Extension: explicit engine options (`ffi::kzg355_options`, filled from `KzgSettings::default_options()`); no environment
    /// variable is read on this path.
    pub fn load_trusted_setup_with_options(
        g1_bytes: Vec<[u8; BYTES_PER_G1]>,
        g2_bytes: Vec<[u8; BYTES_PER_G2]>,
        devices: &[i32],
        options: &ffi::kzg355_options,
    ) -> Result<Self, Error> {
        let g1: Vec<u8> = g1_bytes.iter().flatten().copied().collect();
        let g2: Vec<u8> = g2_bytes.iter().flatten().copied().collect();
        let mut raw = std::ptr::null_mut();
        let devs = if devices.is_empty() { std::ptr::null() } else { devices.as_ptr() };
        check(
            unsafe { ffi::kzg355_load_trusted_setup_ex(g1.as_ptr(), g1_bytes.len(), g2.as_ptr(), g2_bytes.len(), devs, devices.len(), options, &mut raw) },
            "load_trusted_setup_with_options",
        )?;
        Ok(Self { raw })
    }

    /// Defaults of every engine knob (`kzg355_options_default`).  E.g. `o.verify_only = 1` for a handle that never builds the MSM table,
    /// `o.msm_bits = 16` for the widest one (143.5 GB), `o.msm_eager = 1` to build it inside the load instead of on the first commitment.
    pub fn default_options() -> ffi::kzg355_options {
        let mut o = std::mem::MaybeUninit::<ffi::kzg355_options>::zeroed();
        unsafe {
            ffi::kzg355_options_default(o.as_mut_ptr());
            o.assume_init()
        }
    }

    /// FIELD_ELEMENTS_PER_BLOB of this handle (4096, or 4 for a minimal-preset setup).
    pub fn field_elements_per_blob(&self) -> usize {
        unsafe { ffi::kzg355_settings_field_elements_per_blob(self.raw) as usize }
    }

    /// Extension: one count per device of the handle, the EIP-7594 cell launch sets (verify, compute, recover) that device has run so far.
    pub fn cell_calls_per_device(&self) -> Vec<i64> {
        let n = unsafe { ffi::kzg355_settings_cell_calls_per_device(self.raw, std::ptr::null_mut(), 0) };
        let mut out = vec![0 as std::os::raw::c_long; if n > 0 { n as usize } else { 0 }];
        unsafe { ffi::kzg355_settings_cell_calls_per_device(self.raw, out.as_mut_ptr(), out.len()) };
        out.into_iter().map(|v| v as i64).collect()
    }

    pub fn load_trusted_setup_file<P: AsRef<Path>>(trusted_setup_file: P) -> Result<Self, Error> {
        let p = trusted_setup_file.as_ref().to_str().ok_or_else(|| Error::InvalidTrustedSetup("path is not UTF-8".into()))?;
        let c = CString::new(p).map_err(|_| Error::InvalidTrustedSetup("path contains NUL".into()))?;
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::kzg355_load_trusted_setup_file(c.as_ptr(), &mut raw) }, "load_trusted_setup_file")?;
        Ok(Self { raw })
    }
}

pub(crate) fn hex_to_bytes(hex_str: &str) -> Result<Vec<u8>, Error> {
    let trimmed = hex_str.strip_prefix("0x").unwrap_or(hex_str);
    hex::decode(trimmed).map_err(|e| Error::InvalidHexFormat(format!("Failed to decode hex: {}", e)))
}

macro_rules! fixed_bytes {
    ($name:ident, $n:expr, $len_err:expr) => {
        #[derive(Debug, Copy, Clone, PartialEq)]
        pub struct $name {
            pub(crate) bytes: [u8; $n],
        }
        impl $name {
            pub fn from_bytes(b: &[u8]) -> Result<Self, Error> {
                if b.len() != $n {
                    return Err($len_err(format!("Invalid byte length. Expected {} got {}", $n, b.len())));
                }
                let mut bytes = [0u8; $n];
                bytes.copy_from_slice(b);
                Ok(Self { bytes })
            }
            pub fn from_hex(hex_str: &str) -> Result<Self, Error> {
                Self::from_bytes(&hex_to_bytes(hex_str)?)
            }
        }
        impl Default for $name {
            fn default() -> Self {
                Self { bytes: [0u8; $n] }
            }
        }
        impl Deref for $name {
            type Target = [u8; $n];
            fn deref(&self) -> &Self::Target {
                &self.bytes
            }
        }
        impl From<[u8; $n]> for $name {
            fn from(bytes: [u8; $n]) -> Self {
                Self { bytes }
            }
        }
    };
}
fixed_bytes!(Bytes32, 32, Error::BadArgs); // the reference reports a wrong Bytes32 length as BadArgs (kzg.rs:107-112)
fixed_bytes!(Bytes48, 48, Error::InvalidBytesLength);

#[derive(Debug, Clone, PartialEq)]
pub struct Blob {
    bytes: Box<[u8; BYTES_PER_BLOB]>,
}
impl Blob {
    pub fn from_bytes(bytes: &[u8]) -> Result<Self, Error> {
        if bytes.len() != BYTES_PER_BLOB {
            return Err(Error::InvalidBytesLength(format!("Invalid byte length. Expected {} got {}", BYTES_PER_BLOB, bytes.len())));
        }
        let mut v = vec![0u8; BYTES_PER_BLOB].into_boxed_slice();
        v.copy_from_slice(bytes);
        let bytes: Box<[u8; BYTES_PER_BLOB]> = v.try_into().map_err(|_| Error::InternalError)?;
        Ok(Self { bytes })
    }
    pub fn from_hex(hex_str: &str) -> Result<Self, Error> {
        Self::from_bytes(&hex_to_bytes(hex_str)?)
    }
}
impl Deref for Blob {
    type Target = [u8; BYTES_PER_BLOB];
    fn deref(&self) -> &Self::Target {
        &self.bytes
    }
}
// the reference lets callers build and edit blobs in place (kzg.rs:222-228, 262-266: the bench fills arrays and converts them)
impl DerefMut for Blob {
    fn deref_mut(&mut self) -> &mut Self::Target {
        &mut self.bytes
    }
}
impl From<[u8; BYTES_PER_BLOB]> for Blob {
    fn from(value: [u8; BYTES_PER_BLOB]) -> Self {
        Self { bytes: Box::new(value) }
    }
}

/// One EIP-7594 cell: 64 big-endian field elements of the 2x extended blob.
#[derive(Debug, Clone, PartialEq)]
pub struct Cell {
    bytes: Box<[u8; BYTES_PER_CELL]>,
}
impl Cell {
    pub fn from_bytes(bytes: &[u8]) -> Result<Self, Error> {
        if bytes.len() != BYTES_PER_CELL {
            return Err(Error::InvalidBytesLength(format!("Invalid byte length. Expected {} got {}", BYTES_PER_CELL, bytes.len())));
        }
        let mut v = vec![0u8; BYTES_PER_CELL].into_boxed_slice();
        v.copy_from_slice(bytes);
        let bytes: Box<[u8; BYTES_PER_CELL]> = v.try_into().map_err(|_| Error::InternalError)?;
        Ok(Self { bytes })
    }
    pub fn from_hex(hex_str: &str) -> Result<Self, Error> {
        Self::from_bytes(&hex_to_bytes(hex_str)?)
    }
}
impl Deref for Cell {
    type Target = [u8; BYTES_PER_CELL];
    fn deref(&self) -> &Self::Target {
        &self.bytes
    }
}

macro_rules! g1_newtype {
    ($name:ident, $n:expr) => {
        #[derive(Debug, Copy, Clone, PartialEq)]
        pub struct $name(pub Bytes48);
        impl $name {
            pub fn from_hex(hex_str: &str) -> Result<Self, Error> {
                Ok(Self(Bytes48::from_bytes(&hex_to_bytes(hex_str)?)?))
            }
            pub fn to_bytes(self) -> [u8; $n] {
                self.0.bytes
            }
        }
        impl From<Bytes48> for $name {
            fn from(b: Bytes48) -> Self {
                Self(b)
            }
        }
        impl From<[u8; $n]> for $name {
            fn from(b: [u8; $n]) -> Self {
                Self(Bytes48 { bytes: b })
            }
        }
        impl Deref for $name {
            type Target = [u8; $n];
            fn deref(&self) -> &Self::Target {
                &self.0.bytes
            }
        }
    };
}
g1_newtype!(KzgCommitment, BYTES_PER_COMMITMENT);
g1_newtype!(KzgProof, BYTES_PER_PROOF);

pub struct Kzg;

impl Kzg {
    pub fn load_trusted_setup_file<P: AsRef<Path>>(trusted_setup_file: P) -> Result<KzgSettings, Error> {
        KzgSettings::load_trusted_setup_file(trusted_setup_file)
    }

    pub fn load_trusted_setup(g1_bytes: Vec<[u8; BYTES_PER_G1]>, g2_bytes: Vec<[u8; BYTES_PER_G2]>) -> Result<KzgSettings, Error> {
        KzgSettings::load_trusted_setup(g1_bytes, g2_bytes)
    }

    pub fn blob_to_kzg_commitment(blob: &Blob, s: &KzgSettings) -> Result<KzgCommitment, Error> {
        let mut out = [0u8; BYTES_PER_COMMITMENT];
        check(unsafe { ffi::kzg355_blob_to_kzg_commitment(out.as_mut_ptr(), blob.as_ptr(), s.raw) }, "blob_to_kzg_commitment")?;
        Ok(out.into())
    }

    pub fn compute_kzg_proof(blob: &Blob, z_bytes: &Bytes32, s: &KzgSettings) -> Result<(KzgProof, Bytes32), Error> {
        let (mut proof, mut y) = ([0u8; BYTES_PER_PROOF], [0u8; 32]);
        check(
            unsafe { ffi::kzg355_compute_kzg_proof(proof.as_mut_ptr(), y.as_mut_ptr(), blob.as_ptr(), z_bytes.as_ptr(), s.raw) },
            "compute_kzg_proof",
        )?;
        Ok((proof.into(), y.into()))
    }

    pub fn compute_blob_kzg_proof(blob: &Blob, commitment_bytes: &KzgCommitment, s: &KzgSettings) -> Result<KzgProof, Error> {
        let mut proof = [0u8; BYTES_PER_PROOF];
        check(
            unsafe { ffi::kzg355_compute_blob_kzg_proof(proof.as_mut_ptr(), blob.as_ptr(), commitment_bytes.as_ptr(), s.raw) },
            "compute_blob_kzg_proof",
        )?;
        Ok(proof.into())
    }

    pub fn verify_kzg_proof(
        commitment_bytes: &KzgCommitment,
        z_bytes: &Bytes32,
        y_bytes: &Bytes32,
        proof_bytes: &KzgProof,
        s: &KzgSettings,
    ) -> Result<bool, Error> {
        let mut ok = false;
        check(
            unsafe { ffi::kzg355_verify_kzg_proof(&mut ok, commitment_bytes.as_ptr(), z_bytes.as_ptr(), y_bytes.as_ptr(), proof_bytes.as_ptr(), s.raw) },
            "verify_kzg_proof",
        )?;
        Ok(ok)
    }

    pub fn verify_blob_kzg_proof(blob: &Blob, commitment_bytes: &KzgCommitment, proof_bytes: &KzgProof, s: &KzgSettings) -> Result<bool, Error> {
        let mut ok = false;
        check(
            unsafe { ffi::kzg355_verify_blob_kzg_proof(&mut ok, blob.as_ptr(), commitment_bytes.as_ptr(), proof_bytes.as_ptr(), s.raw) },
            "verify_blob_kzg_proof",
        )?;
        Ok(ok)
    }

    pub fn verify_blob_kzg_proof_batch(blobs: &[Blob], commitment_bytes: &[KzgCommitment], proof_bytes: &[KzgProof], s: &KzgSettings) -> Result<bool, Error> {
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitment_bytes.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = proof_bytes.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = false;
        // all three lengths cross the boundary: the mismatch check of the reference (kzg.rs:644-651) is the library's
        check(
            unsafe {
                ffi::kzg355_verify_blob_kzg_proof_batch(&mut ok, staged.as_ptr(), blobs.len(), c.as_ptr(), commitment_bytes.len(), p.as_ptr(), proof_bytes.len(), s.raw)
            },
            "verify_blob_kzg_proof_batch",
        )?;
        Ok(ok)
    }

    // ---- throughput extensions (no reference counterpart): many independent units per call, one set of kernel launches ----

    /// `blobs.len()` independent `blob_to_kzg_commitment` calls; one `Result` per blob.
    pub fn blob_to_kzg_commitment_many(blobs: &[Blob], s: &KzgSettings) -> Result<Vec<Result<KzgCommitment, Error>>, Error> {
        let n = blobs.len();
        let staged = stage_blobs(blobs);
        let mut out = vec![0u8; BYTES_PER_COMMITMENT * n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe { ffi::kzg355_blob_to_kzg_commitment_many(out.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), n, s.raw) };
        whole_call(rc, &st[..n], "blob_to_kzg_commitment_many")?;
        Ok((0..n)
            .map(|i| check(st[i], "commit").map(|_| KzgCommitment::from(<[u8; BYTES_PER_COMMITMENT]>::try_from(&out[48 * i..48 * i + 48]).unwrap())))
            .collect())
    }

    /// `blobs.len()` independent `compute_blob_kzg_proof` calls.
    pub fn compute_blob_kzg_proof_many(blobs: &[Blob], commitments: &[KzgCommitment], s: &KzgSettings) -> Result<Vec<Result<KzgProof, Error>>, Error> {
        if blobs.len() != commitments.len() {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let n = blobs.len();
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let mut out = vec![0u8; BYTES_PER_PROOF * n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe { ffi::kzg355_compute_blob_kzg_proof_many(out.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), c.as_ptr(), n, s.raw) };
        whole_call(rc, &st[..n], "compute_blob_kzg_proof_many")?;
        Ok((0..n)
            .map(|i| check(st[i], "proof").map(|_| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&out[48 * i..48 * i + 48]).unwrap())))
            .collect())
    }

    /// `groups` independent `verify_blob_kzg_proof_batch` calls of `n_per_group` blobs each (inputs group-major).
    pub fn verify_blob_kzg_proof_batch_many(
        blobs: &[Blob],
        commitments: &[KzgCommitment],
        proofs: &[KzgProof],
        n_per_group: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        if blobs.len() != commitments.len() || blobs.len() != proofs.len() || n_per_group == 0 || blobs.len() % n_per_group != 0 {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let groups = blobs.len() / n_per_group;
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = unsafe {
            ffi::kzg355_verify_blob_kzg_proof_batch_many(ok.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), c.as_ptr(), p.as_ptr(), n_per_group, groups, s.raw)
        };
        whole_call(rc, &st[..groups], "verify_blob_kzg_proof_batch_many")?;
        Ok((0..groups).map(|g| check(st[g], "verify").map(|_| ok[g])).collect())
    }

    /// EIP-7594 `verify_cell_kzg_proof_batch` (consensus specs fulu/polynomial-commitments-sampling.md): one commitment, cell index (< 128),
    /// cell and proof per cell.
    pub fn verify_cell_kzg_proof_batch(
        commitments: &[KzgCommitment],
        cell_indices: &[usize],
        cells: &[Cell],
        proofs: &[KzgProof],
        s: &KzgSettings,
    ) -> Result<bool, Error> {
        let n = commitments.len();
        if cell_indices.len() != n || cells.len() != n || proofs.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let cl: Vec<u8> = cells.iter().flat_map(|x| x.iter().copied()).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = false;
        check(
            unsafe { ffi::kzg355_verify_cell_kzg_proof_batch(&mut ok, c.as_ptr(), cell_indices.as_ptr(), cl.as_ptr(), p.as_ptr(), n, s.raw) },
            "verify_cell_kzg_proof_batch",
        )?;
        Ok(ok)
    }

    /// `groups` independent `verify_cell_kzg_proof_batch` calls of `n_per_group` cells each (inputs group-major): one verdict per sidecar.
    pub fn verify_cell_kzg_proof_batch_many(
        commitments: &[KzgCommitment],
        cell_indices: &[usize],
        cells: &[Cell],
        proofs: &[KzgProof],
        n_per_group: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = commitments.len();
        if cell_indices.len() != n || cells.len() != n || proofs.len() != n || n_per_group == 0 || n % n_per_group != 0 {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let groups = n / n_per_group;
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let cl: Vec<u8> = cells.iter().flat_map(|x| x.iter().copied()).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = unsafe {
            ffi::kzg355_verify_cell_kzg_proof_batch_many(ok.as_mut_ptr(), st.as_mut_ptr(), c.as_ptr(), cell_indices.as_ptr(), cl.as_ptr(), p.as_ptr(),
                                                         n_per_group, groups, s.raw)
        };
        whole_call(rc, &st[..groups], "verify_cell_kzg_proof_batch_many")?;
        Ok((0..groups).map(|g| check(st[g], "verify_cell").map(|_| ok[g])).collect())
    }

    /// `verify_cell_kzg_proof_batch_many` for groups of different sizes: group `g` is `cell_counts[g]` entries of the four slices, after those of
    /// group `g - 1`; an empty group is `Ok(true)`.  All non-empty groups run in one set of launches.
    pub fn verify_cell_kzg_proof_batch_many_sets(
        cell_counts: &[usize],
        commitments: &[KzgCommitment],
        cell_indices: &[usize],
        cells: &[Cell],
        proofs: &[KzgProof],
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = commitments.len();
        let total = cell_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c));
        if cell_indices.len() != n || cells.len() != n || proofs.len() != n || total != Some(n) {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let groups = cell_counts.len();
        // (one spare entry each: the pointer of an empty Vec is not one the library may be handed)
        let mut counts = cell_counts.to_vec();
        counts.push(0);
        let mut idx = cell_indices.to_vec();
        idx.push(0);
        let mut c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        c.push(0);
        let mut cl: Vec<u8> = cells.iter().flat_map(|x| x.iter().copied()).collect();
        cl.push(0);
        let mut p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        p.push(0);
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = unsafe {
            ffi::kzg355_verify_cell_kzg_proof_batch_many_sets(ok.as_mut_ptr(), st.as_mut_ptr(), counts.as_ptr(), c.as_ptr(), idx.as_ptr(), cl.as_ptr(),
                                                              p.as_ptr(), groups, s.raw)
        };
        whole_call(rc, &st[..groups], "verify_cell_kzg_proof_batch_many_sets")?;
        Ok((0..groups).map(|g| check(st[g], "verify_cell").map(|_| ok[g])).collect())
    }

    /// Blobs against their EIP-7594 cell proofs, the Fulu counterpart of `verify_blob_kzg_proof_batch`: `cell_proofs` holds the 128 proofs of
    /// every blob, blob after blob in cell order.  Exactly `verify_cell_kzg_proof_batch` over all 128 cells of every blob, the cells computed on
    /// the device.
    pub fn verify_blob_cell_proofs_batch(blobs: &[Blob], commitments: &[KzgCommitment], cell_proofs: &[KzgProof], s: &KzgSettings) -> Result<bool, Error> {
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = cell_proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = false;
        // all three lengths cross the boundary: the mismatch check is the library's
        check(
            unsafe {
                ffi::kzg355_verify_blob_cell_proofs_batch(&mut ok, staged.as_ptr(), blobs.len(), c.as_ptr(), commitments.len(), p.as_ptr(), cell_proofs.len(), s.raw)
            },
            "verify_blob_cell_proofs_batch",
        )?;
        Ok(ok)
    }

    /// `groups` independent `verify_blob_cell_proofs_batch` calls of `n_per_group` blobs each (inputs group-major): one verdict per transaction.
    pub fn verify_blob_cell_proofs_batch_many(
        blobs: &[Blob],
        commitments: &[KzgCommitment],
        cell_proofs: &[KzgProof],
        n_per_group: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = blobs.len();
        if commitments.len() != n || cell_proofs.len() != CELLS_PER_EXT_BLOB * n || n_per_group == 0 || n % n_per_group != 0 {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let groups = n / n_per_group;
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = cell_proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = unsafe {
            ffi::kzg355_verify_blob_cell_proofs_batch_many(ok.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), c.as_ptr(), p.as_ptr(), n_per_group, groups, s.raw)
        };
        whole_call(rc, &st[..groups], "verify_blob_cell_proofs_batch_many")?;
        Ok((0..groups).map(|g| check(st[g], "verify_blob_cells").map(|_| ok[g])).collect())
    }

    /// Blob transactions of different blob counts in one call: group `g` is the next `blob_counts[g]` blobs and commitments and the next
    /// `128 * blob_counts[g]` proofs of the three slices, which hold the groups one after the other with no padding.  One independent
    /// `verify_blob_cell_proofs_batch` per group, all non-empty groups in one set of launches; an empty group is `Ok(true)`.
    pub fn verify_blob_cell_proofs_batch_many_sets(
        blobs: &[Blob],
        commitments: &[KzgCommitment],
        cell_proofs: &[KzgProof],
        blob_counts: &[usize],
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = blobs.len();
        let total = blob_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c));
        if total != Some(n) || commitments.len() != n || cell_proofs.len() != CELLS_PER_EXT_BLOB * n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let groups = blob_counts.len();
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = cell_proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = unsafe {
            ffi::kzg355_verify_blob_cell_proofs_batch_many_sets(
                ok.as_mut_ptr(),
                st.as_mut_ptr(),
                blob_counts.as_ptr(),
                staged.as_ptr(),
                c.as_ptr(),
                p.as_ptr(),
                groups,
                s.raw,
            )
        };
        whole_call(rc, &st[..groups], "verify_blob_cell_proofs_batch_many_sets")?;
        Ok((0..groups).map(|g| check(st[g], "verify_blob_cells").map(|_| ok[g])).collect())
    }

    /// `verify_blob_kzg_proof_batch` on batches of different blob counts in one call: batch `g` is the next `blob_counts[g]` entries of the three
    /// slices, which hold the batches one after the other with no padding.  Each batch has its own challenge `r`, pairing and verdict; an empty
    /// batch is `Ok(true)`.
    pub fn verify_blob_kzg_proof_batch_many_sets(
        blobs: &[Blob],
        commitments: &[KzgCommitment],
        proofs: &[KzgProof],
        blob_counts: &[usize],
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = blobs.len();
        let total = blob_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c));
        if total != Some(n) || commitments.len() != n || proofs.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let groups = blob_counts.len();
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = unsafe {
            ffi::kzg355_verify_blob_kzg_proof_batch_many_sets(
                ok.as_mut_ptr(),
                st.as_mut_ptr(),
                blob_counts.as_ptr(),
                staged.as_ptr(),
                c.as_ptr(),
                p.as_ptr(),
                groups,
                s.raw,
            )
        };
        whole_call(rc, &st[..groups], "verify_blob_kzg_proof_batch_many_sets")?;
        Ok((0..groups).map(|g| check(st[g], "verify_blob_kzg_proof_batch").map(|_| ok[g])).collect())
    }

    /// EIP-7594 `compute_cells_and_kzg_proofs`: the 128 cells of the blob's 2x extension (cells 0..63 are the blob itself) and their 128 proofs,
    /// in cell order (FK20 on the device).
    pub fn compute_cells_and_kzg_proofs(blob: &Blob, s: &KzgSettings) -> Result<(Vec<Cell>, Vec<KzgProof>), Error> {
        let mut res = Self::compute_cells_and_kzg_proofs_many(std::slice::from_ref(blob), s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// `blobs.len()` independent `compute_cells_and_kzg_proofs` calls in one set of launches; one `Result` per blob.
    pub fn compute_cells_and_kzg_proofs_many(blobs: &[Blob], s: &KzgSettings) -> Result<Vec<Result<(Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let n = blobs.len();
        let staged = stage_blobs(blobs);
        let per_cells = BYTES_PER_CELL * CELLS_PER_EXT_BLOB;
        let mut cells = vec![0u8; per_cells * n.max(1)];
        let mut proofs = vec![0u8; BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe {
            ffi::kzg355_compute_cells_and_kzg_proofs_many(cells.as_mut_ptr(), proofs.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), n, s.raw)
        };
        whole_call(rc, &st[..n], "compute_cells_and_kzg_proofs_many")?;
        Ok((0..n)
            .map(|i| {
                check(st[i], "compute_cells")?;
                let cs = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| Cell::from_bytes(&cells[per_cells * i + BYTES_PER_CELL * k..per_cells * i + BYTES_PER_CELL * (k + 1)]))
                    .collect::<Result<Vec<_>, _>>()?;
                let base = BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * i;
                let ps = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&proofs[base + 48 * k..base + 48 * (k + 1)]).unwrap()))
                    .collect();
                Ok((cs, ps))
            })
            .collect())
    }

    /// EIP-7594 `recover_cells_and_kzg_proofs`: all 128 cells and proofs of a blob from 64..128 of its cells at strictly ascending `cell_indices`.
    pub fn recover_cells_and_kzg_proofs(cell_indices: &[usize], cells: &[Cell], s: &KzgSettings) -> Result<(Vec<Cell>, Vec<KzgProof>), Error> {
        if cell_indices.len() != cells.len() {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let mut res = Self::recover_cells_and_kzg_proofs_many(cell_indices, cells, 1, s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// `m` blobs known at the same `cell_indices` (`cells`: blob after blob, `cell_indices.len()` cells each) in one set of launches; one `Result`
    /// per blob.
    pub fn recover_cells_and_kzg_proofs_many(
        cell_indices: &[usize],
        cells: &[Cell],
        m: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let n = cell_indices.len();
        if cells.len() != n * m {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let input: Vec<u8> = cells.iter().flat_map(|x| x.iter().copied()).collect();
        let per_cells = BYTES_PER_CELL * CELLS_PER_EXT_BLOB;
        let mut out_cells = vec![0u8; per_cells * m.max(1)];
        let mut proofs = vec![0u8; BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * m.max(1)];
        let mut st = vec![0i32; m.max(1)];
        let rc = unsafe {
            ffi::kzg355_recover_cells_and_kzg_proofs_many(out_cells.as_mut_ptr(), proofs.as_mut_ptr(), st.as_mut_ptr(), cell_indices.as_ptr(),
                                                          input.as_ptr(), n, m, s.raw)
        };
        whole_call(rc, &st[..m], "recover_cells_and_kzg_proofs_many")?;
        Ok((0..m)
            .map(|i| {
                check(st[i], "recover_cells")?;
                let cs = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| Cell::from_bytes(&out_cells[per_cells * i + BYTES_PER_CELL * k..per_cells * i + BYTES_PER_CELL * (k + 1)]))
                    .collect::<Result<Vec<_>, _>>()?;
                let base = BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * i;
                let ps = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&proofs[base + 48 * k..base + 48 * (k + 1)]).unwrap()))
                    .collect();
                Ok((cs, ps))
            })
            .collect())
    }

    /// One independent `recover_cells_and_kzg_proofs` per unit `(cell_indices, cells)` in one set of launches: every blob brings its own index
    /// set (blocks of a node that catches up hold different columns).  One `Result` per unit; a unit whose two lengths differ is `BadArgs` for
    /// the call.
    pub fn recover_cells_and_kzg_proofs_many_sets(
        units: &[(&[usize], &[Cell])],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let m = units.len();
        if units.iter().any(|(ix, cells)| ix.len() != cells.len()) {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let counts: Vec<usize> = units.iter().map(|(ix, _)| ix.len()).collect();
        let indices: Vec<usize> = units.iter().flat_map(|(ix, _)| ix.iter().copied()).collect();
        let input: Vec<u8> = units.iter().flat_map(|(_, cells)| cells.iter().flat_map(|x| x.iter().copied())).collect();
        let per_cells = BYTES_PER_CELL * CELLS_PER_EXT_BLOB;
        let mut out_cells = vec![0u8; per_cells * m.max(1)];
        let mut proofs = vec![0u8; BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * m.max(1)];
        let mut st = vec![0i32; m.max(1)];
        let rc = unsafe {
            ffi::kzg355_recover_cells_and_kzg_proofs_many_sets(out_cells.as_mut_ptr(), proofs.as_mut_ptr(), st.as_mut_ptr(), counts.as_ptr(),
                                                               indices.as_ptr(), input.as_ptr(), m, s.raw)
        };
        whole_call(rc, &st[..m], "recover_cells_and_kzg_proofs_many_sets")?;
        Ok((0..m)
            .map(|i| {
                check(st[i], "recover_cells")?;
                let cs = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| Cell::from_bytes(&out_cells[per_cells * i + BYTES_PER_CELL * k..per_cells * i + BYTES_PER_CELL * (k + 1)]))
                    .collect::<Result<Vec<_>, _>>()?;
                let base = BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * i;
                let ps = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&proofs[base + 48 * k..base + 48 * (k + 1)]).unwrap()))
                    .collect();
                Ok((cs, ps))
            })
            .collect())
    }

    /// `compute_cells_and_kzg_proofs` with the blob's commitment as well: the FK20 chain computes it on its way to the proofs (slot 63 of the
    /// convolution whose other slots give the proofs), so no second call and no wide MSM table is needed.
    pub fn compute_commitment_cells_and_kzg_proofs(blob: &Blob, s: &KzgSettings) -> Result<(KzgCommitment, Vec<Cell>, Vec<KzgProof>), Error> {
        let mut res = Self::compute_commitment_cells_and_kzg_proofs_many(std::slice::from_ref(blob), s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// `blobs.len()` independent calls of the above in one set of launches; one `Result` per blob.
    pub fn compute_commitment_cells_and_kzg_proofs_many(
        blobs: &[Blob],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(KzgCommitment, Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let n = blobs.len();
        let staged = stage_blobs(blobs);
        let mut out = CommitCellsProofs::new(n);
        let rc = unsafe {
            ffi::kzg355_compute_commitments_cells_and_kzg_proofs_many(out.commitments.as_mut_ptr(), out.cells.as_mut_ptr(), out.proofs.as_mut_ptr(),
                                                                      out.st.as_mut_ptr(), staged.as_ptr(), n, s.raw)
        };
        whole_call(rc, &out.st[..n], "compute_commitment_cells_and_kzg_proofs_many")?;
        Ok(out.unpack(n, "compute_cells"))
    }

    /// `recover_cells_and_kzg_proofs` with the commitment of the recovered blob as well, for the comparison with the block's
    /// `blob_kzg_commitments`: more than 64 cells that lie on no polynomial of degree < 4096 are no error, and that comparison shows them up.
    pub fn recover_commitment_cells_and_kzg_proofs(
        cell_indices: &[usize],
        cells: &[Cell],
        s: &KzgSettings,
    ) -> Result<(KzgCommitment, Vec<Cell>, Vec<KzgProof>), Error> {
        if cell_indices.len() != cells.len() {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let mut res = Self::recover_commitment_cells_and_kzg_proofs_many(cell_indices, cells, 1, s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// `m` blobs known at the same `cell_indices`, as `recover_cells_and_kzg_proofs_many`, with their commitments.
    pub fn recover_commitment_cells_and_kzg_proofs_many(
        cell_indices: &[usize],
        cells: &[Cell],
        m: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(KzgCommitment, Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let n = cell_indices.len();
        if cells.len() != n * m {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let input: Vec<u8> = cells.iter().flat_map(|x| x.iter().copied()).collect();
        let mut out = CommitCellsProofs::new(m);
        let rc = unsafe {
            ffi::kzg355_recover_commitments_cells_and_kzg_proofs_many(out.commitments.as_mut_ptr(), out.cells.as_mut_ptr(), out.proofs.as_mut_ptr(),
                                                                      out.st.as_mut_ptr(), cell_indices.as_ptr(), input.as_ptr(), n, m, s.raw)
        };
        whole_call(rc, &out.st[..m], "recover_commitment_cells_and_kzg_proofs_many")?;
        Ok(out.unpack(m, "recover_cells"))
    }

    /// One unit `(cell_indices, cells)` per blob, as `recover_cells_and_kzg_proofs_many_sets`, with their commitments.
    pub fn recover_commitment_cells_and_kzg_proofs_many_sets(
        units: &[(&[usize], &[Cell])],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(KzgCommitment, Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let m = units.len();
        if units.iter().any(|(ix, cells)| ix.len() != cells.len()) {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let counts: Vec<usize> = units.iter().map(|(ix, _)| ix.len()).collect();
        let indices: Vec<usize> = units.iter().flat_map(|(ix, _)| ix.iter().copied()).collect();
        let input: Vec<u8> = units.iter().flat_map(|(_, cells)| cells.iter().flat_map(|x| x.iter().copied())).collect();
        let mut out = CommitCellsProofs::new(m);
        let rc = unsafe {
            ffi::kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(out.commitments.as_mut_ptr(), out.cells.as_mut_ptr(),
                                                                           out.proofs.as_mut_ptr(), out.st.as_mut_ptr(), counts.as_ptr(),
                                                                           indices.as_ptr(), input.as_ptr(), m, s.raw)
        };
        whole_call(rc, &out.st[..m], "recover_commitment_cells_and_kzg_proofs_many_sets")?;
        Ok(out.unpack(m, "recover_cells"))
    }

    /// The cells of the blob at `cell_indices` (each < 128, any order, repeats allowed) and their proofs: entry `j` is what
    /// `compute_cells_and_kzg_proofs` returns at index `cell_indices[j]`, at the price of one MSM per index instead of the FK20 chain.
    pub fn compute_cell_kzg_proofs_at(blob: &Blob, cell_indices: &[usize], s: &KzgSettings) -> Result<(Vec<Cell>, Vec<KzgProof>), Error> {
        let mut res = Self::compute_cell_kzg_proofs_at_many(std::slice::from_ref(blob), &[cell_indices], s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// One independent `compute_cell_kzg_proofs_at` per blob, each with its own index list (which may be empty), in one set of launches.  One
    /// `Result` per blob; `blobs` and `index_lists` of different lengths are `BadArgs` for the call.
    pub fn compute_cell_kzg_proofs_at_many(
        blobs: &[Blob],
        index_lists: &[&[usize]],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let n = blobs.len();
        if index_lists.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let staged = stage_blobs(blobs);
        let counts: Vec<usize> = index_lists.iter().map(|ix| ix.len()).collect();
        let indices: Vec<usize> = index_lists.iter().flat_map(|ix| ix.iter().copied()).collect();
        let total = indices.len();
        let mut cells = vec![0u8; BYTES_PER_CELL * total.max(1)];
        let mut proofs = vec![0u8; BYTES_PER_PROOF * total.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe {
            ffi::kzg355_compute_cell_kzg_proofs_at_many(cells.as_mut_ptr(), proofs.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), n, counts.as_ptr(),
                                                        indices.as_ptr(), s.raw)
        };
        whole_call(rc, &st[..n], "compute_cell_kzg_proofs_at_many")?;
        let mut off = 0usize;
        Ok((0..n)
            .map(|i| {
                let (lo, hi) = (off, off + counts[i]);
                off = hi;
                check(st[i], "compute_cell_kzg_proofs_at")?;
                let cs = (lo..hi).map(|j| Cell::from_bytes(&cells[BYTES_PER_CELL * j..BYTES_PER_CELL * (j + 1)])).collect::<Result<Vec<_>, _>>()?;
                let ps = (lo..hi).map(|j| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&proofs[48 * j..48 * (j + 1)]).unwrap())).collect();
                Ok((cs, ps))
            })
            .collect())
    }

    /// The cells of the recovered blob at `want_indices` (each < 128, any order, repeats allowed) and their proofs: entry `j` is what
    /// `recover_cells_and_kzg_proofs` returns at index `want_indices[j]` for the same input, at the price of one MSM per wanted index instead
    /// of the FK20 chain.
    pub fn recover_cells_and_kzg_proofs_at(
        cell_indices: &[usize],
        cells: &[Cell],
        want_indices: &[usize],
        s: &KzgSettings,
    ) -> Result<(Vec<Cell>, Vec<KzgProof>), Error> {
        let mut res = Self::recover_cells_and_kzg_proofs_at_many_sets(&[(cell_indices, cells, want_indices)], s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// One independent `recover_cells_and_kzg_proofs_at` per unit `(cell_indices, cells, want_indices)` in one set of launches (`want_indices`
    /// may be empty: the blob is still recovered and checked).  One `Result` per unit; a unit whose first two lengths differ is `BadArgs` for
    /// the call.
    pub fn recover_cells_and_kzg_proofs_at_many_sets(
        units: &[(&[usize], &[Cell], &[usize])],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(Vec<Cell>, Vec<KzgProof>), Error>>, Error> {
        let m = units.len();
        if units.iter().any(|(ix, cells, _)| ix.len() != cells.len()) {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let counts: Vec<usize> = units.iter().map(|(ix, _, _)| ix.len()).collect();
        let indices: Vec<usize> = units.iter().flat_map(|(ix, _, _)| ix.iter().copied()).collect();
        let input: Vec<u8> = units.iter().flat_map(|(_, cells, _)| cells.iter().flat_map(|x| x.iter().copied())).collect();
        let want_counts: Vec<usize> = units.iter().map(|(_, _, want)| want.len()).collect();
        let want: Vec<usize> = units.iter().flat_map(|(_, _, want)| want.iter().copied()).collect();
        let total = want.len();
        let mut out_cells = vec![0u8; BYTES_PER_CELL * total.max(1)];
        let mut proofs = vec![0u8; BYTES_PER_PROOF * total.max(1)];
        let mut st = vec![0i32; m.max(1)];
        let rc = unsafe {
            ffi::kzg355_recover_cells_and_kzg_proofs_at_many_sets(out_cells.as_mut_ptr(), proofs.as_mut_ptr(), st.as_mut_ptr(), counts.as_ptr(),
                                                                  indices.as_ptr(), input.as_ptr(), want_counts.as_ptr(), want.as_ptr(), m, s.raw)
        };
        whole_call(rc, &st[..m], "recover_cells_and_kzg_proofs_at_many_sets")?;
        let mut off = 0usize;
        Ok((0..m)
            .map(|i| {
                let (lo, hi) = (off, off + want_counts[i]);
                off = hi;
                check(st[i], "recover_cells_and_kzg_proofs_at")?;
                let cs = (lo..hi).map(|j| Cell::from_bytes(&out_cells[BYTES_PER_CELL * j..BYTES_PER_CELL * (j + 1)])).collect::<Result<Vec<_>, _>>()?;
                let ps = (lo..hi).map(|j| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&proofs[48 * j..48 * (j + 1)]).unwrap())).collect();
                Ok((cs, ps))
            })
            .collect())
    }

    /// `recover_cells_and_kzg_proofs_at_many_sets` of resident blobs: the known cells (device memory) follow `cell_counts`, and slot `j` of the
    /// device outputs receives the cell and proof of entry `j` of `want_indices`; the counts and both index lists are host memory.
    ///
    /// # Safety
    /// `d_cells` holds `cell_indices.len()` cells on the handle's device; the outputs `want_indices.len()` cells / proofs; all 16-byte aligned.
    pub unsafe fn recover_cells_and_kzg_proofs_at_many_sets_device(
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        cell_counts: &[usize],
        cell_indices: &[usize],
        d_cells: *const u8,
        want_counts: &[usize],
        want_indices: &[usize],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let m = cell_counts.len();
        if want_counts.len() != m
            || cell_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c)) != Some(cell_indices.len())
            || want_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c)) != Some(want_indices.len())
        {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let mut st = vec![0i32; m.max(1)];
        let rc = ffi::kzg355_recover_cells_and_kzg_proofs_at_many_sets_device(d_cells_out, d_proofs_out, st.as_mut_ptr(), cell_counts.as_ptr(),
                                                                              cell_indices.as_ptr(), d_cells, want_counts.as_ptr(),
                                                                              want_indices.as_ptr(), m, s.raw);
        whole_call(rc, &st[..m], "recover_cells_and_kzg_proofs_at_many_sets_device")?;
        Ok((0..m).map(|i| check(st[i], "recover_cells_and_kzg_proofs_at")).collect())
    }

    /// `verify_cell_kzg_proof_batch_many` on device-resident data: the four pointers are DEVICE pointers on the handle's device (byte buffers
    /// 16-byte aligned, the indices 8-byte aligned), group-major, `n_per_group` cells per group; only the verdicts cross PCIe.
    ///
    /// # Safety
    /// The pointers must be valid device allocations of `groups * n_per_group` entries each, untouched until the call returns.
    pub unsafe fn verify_cell_kzg_proof_batch_many_device(
        d_commitments: *const u8,
        d_cell_indices: *const usize,
        d_cells: *const u8,
        d_proofs: *const u8,
        n_per_group: usize,
        groups: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = ffi::kzg355_verify_cell_kzg_proof_batch_many_device(ok.as_mut_ptr(), st.as_mut_ptr(), d_commitments, d_cell_indices, d_cells, d_proofs,
                                                                     n_per_group, groups, s.raw);
        whole_call(rc, &st[..groups], "verify_cell_kzg_proof_batch_many_device")?;
        Ok((0..groups).map(|g| check(st[g], "verify_cell").map(|_| ok[g])).collect())
    }

    /// `verify_cell_kzg_proof_batch_many_sets` on device-resident data: group `g` is `cell_counts[g]` entries of the four DEVICE arrays (byte
    /// buffers 16-byte aligned, the indices 8-byte aligned), group after group; `cell_counts` is host memory.  An empty group is `Ok(true)`.
    ///
    /// # Safety
    /// The pointers must be valid device allocations of the sum of the counts entries each, untouched until the call returns.
    pub unsafe fn verify_cell_kzg_proof_batch_many_sets_device(
        cell_counts: &[usize],
        d_commitments: *const u8,
        d_cell_indices: *const usize,
        d_cells: *const u8,
        d_proofs: *const u8,
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let groups = cell_counts.len();
        let mut ok = vec![false; groups.max(1)];
        let mut st = vec![0i32; groups.max(1)];
        let rc = ffi::kzg355_verify_cell_kzg_proof_batch_many_sets_device(ok.as_mut_ptr(), st.as_mut_ptr(), cell_counts.as_ptr(), d_commitments,
                                                                          d_cell_indices, d_cells, d_proofs, groups, s.raw);
        whole_call(rc, &st[..groups], "verify_cell_kzg_proof_batch_many_sets_device")?;
        Ok((0..groups).map(|g| check(st[g], "verify_cell").map(|_| ok[g])).collect())
    }

    /// `compute_cells_and_kzg_proofs` of `n` resident blobs into the caller's device buffers (either may be null, not both); one `Result` per
    /// blob, the output slots of a failed blob unspecified.
    ///
    /// # Safety
    /// Device pointers on the handle's device, 16-byte aligned, of `n` blobs / `n * 128` cells / `n * 128` proofs; outputs must not overlap the input.
    pub unsafe fn compute_cells_and_kzg_proofs_many_device(
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        d_blobs: *const u8,
        n: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let mut st = vec![0i32; n.max(1)];
        let rc = ffi::kzg355_compute_cells_and_kzg_proofs_many_device(d_cells_out, d_proofs_out, st.as_mut_ptr(), d_blobs, n, s.raw);
        whole_call(rc, &st[..n], "compute_cells_and_kzg_proofs_many_device")?;
        Ok((0..n).map(|i| check(st[i], "compute_cells")).collect())
    }

    /// `recover_cells_and_kzg_proofs` of `m` resident blobs known at the same `cell_indices` (host memory); outputs as above.
    ///
    /// # Safety
    /// `d_cells` holds `m * cell_indices.len()` cells on the handle's device; the outputs `m * 128` cells / proofs; all 16-byte aligned.
    pub unsafe fn recover_cells_and_kzg_proofs_many_device(
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        cell_indices: &[usize],
        d_cells: *const u8,
        m: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let mut st = vec![0i32; m.max(1)];
        let rc = ffi::kzg355_recover_cells_and_kzg_proofs_many_device(d_cells_out, d_proofs_out, st.as_mut_ptr(), cell_indices.as_ptr(), d_cells,
                                                                      cell_indices.len(), m, s.raw);
        whole_call(rc, &st[..m], "recover_cells_and_kzg_proofs_many_device")?;
        Ok((0..m).map(|i| check(st[i], "recover_cells")).collect())
    }

    /// `recover_cells_and_kzg_proofs_many_sets` of resident blobs: blob `i` is known at `cell_counts[i]` cells, its indices (host memory) and its
    /// cells (device memory) following those of blob `i - 1`; outputs as above.
    ///
    /// # Safety
    /// `d_cells` holds `cell_indices.len()` cells on the handle's device; the outputs `cell_counts.len() * 128` cells / proofs; all 16-byte aligned.
    pub unsafe fn recover_cells_and_kzg_proofs_many_sets_device(
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        cell_counts: &[usize],
        cell_indices: &[usize],
        d_cells: *const u8,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let m = cell_counts.len();
        if cell_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c)) != Some(cell_indices.len()) {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let mut st = vec![0i32; m.max(1)];
        let rc = ffi::kzg355_recover_cells_and_kzg_proofs_many_sets_device(d_cells_out, d_proofs_out, st.as_mut_ptr(), cell_counts.as_ptr(),
                                                                           cell_indices.as_ptr(), d_cells, m, s.raw);
        whole_call(rc, &st[..m], "recover_cells_and_kzg_proofs_many_sets_device")?;
        Ok((0..m).map(|i| check(st[i], "recover_cells")).collect())
    }

    /// `compute_cells_and_kzg_proofs_many_device` with the commitments (48 bytes per blob) written to `d_commitments_out` as well; any of the
    /// three outputs may be null, not all.
    ///
    /// # Safety
    /// As `compute_cells_and_kzg_proofs_many_device`; `d_commitments_out` holds `n * 48` bytes on the handle's device, 16-byte aligned.
    pub unsafe fn compute_commitment_cells_and_kzg_proofs_many_device(
        d_commitments_out: *mut u8,
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        d_blobs: *const u8,
        n: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let mut st = vec![0i32; n.max(1)];
        let rc = ffi::kzg355_compute_commitments_cells_and_kzg_proofs_many_device(d_commitments_out, d_cells_out, d_proofs_out, st.as_mut_ptr(),
                                                                                  d_blobs, n, s.raw);
        whole_call(rc, &st[..n], "compute_commitment_cells_and_kzg_proofs_many_device")?;
        Ok((0..n).map(|i| check(st[i], "compute_cells")).collect())
    }

    /// `recover_cells_and_kzg_proofs_many_device` with the commitments of the recovered blobs written to `d_commitments_out` as well.
    ///
    /// # Safety
    /// As `recover_cells_and_kzg_proofs_many_device`; `d_commitments_out` holds `m * 48` bytes on the handle's device, 16-byte aligned.
    pub unsafe fn recover_commitment_cells_and_kzg_proofs_many_device(
        d_commitments_out: *mut u8,
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        cell_indices: &[usize],
        d_cells: *const u8,
        m: usize,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let mut st = vec![0i32; m.max(1)];
        let rc = ffi::kzg355_recover_commitments_cells_and_kzg_proofs_many_device(d_commitments_out, d_cells_out, d_proofs_out, st.as_mut_ptr(),
                                                                                  cell_indices.as_ptr(), d_cells, cell_indices.len(), m, s.raw);
        whole_call(rc, &st[..m], "recover_commitment_cells_and_kzg_proofs_many_device")?;
        Ok((0..m).map(|i| check(st[i], "recover_cells")).collect())
    }

    /// `recover_cells_and_kzg_proofs_many_sets_device` with the commitments of the recovered blobs written to `d_commitments_out` as well.
    ///
    /// # Safety
    /// As `recover_cells_and_kzg_proofs_many_sets_device`; `d_commitments_out` holds `cell_counts.len() * 48` bytes, 16-byte aligned.
    pub unsafe fn recover_commitment_cells_and_kzg_proofs_many_sets_device(
        d_commitments_out: *mut u8,
        d_cells_out: *mut u8,
        d_proofs_out: *mut u8,
        cell_counts: &[usize],
        cell_indices: &[usize],
        d_cells: *const u8,
        s: &KzgSettings,
    ) -> Result<Vec<Result<(), Error>>, Error> {
        let m = cell_counts.len();
        if cell_counts.iter().try_fold(0usize, |a, &c| a.checked_add(c)) != Some(cell_indices.len()) {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let mut st = vec![0i32; m.max(1)];
        let rc = ffi::kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(d_commitments_out, d_cells_out, d_proofs_out,
                                                                                       st.as_mut_ptr(), cell_counts.as_ptr(), cell_indices.as_ptr(),
                                                                                       d_cells, m, s.raw);
        whole_call(rc, &st[..m], "recover_commitment_cells_and_kzg_proofs_many_sets_device")?;
        Ok((0..m).map(|i| check(st[i], "recover_cells")).collect())
    }

    /// `commitments.len()` independent `verify_kzg_proof` checks (one proof per call is what benches/kzg_benches.rs:70-81 times).
    pub fn verify_kzg_proof_many(
        commitments: &[KzgCommitment],
        zs: &[Bytes32],
        ys: &[Bytes32],
        proofs: &[KzgProof],
        s: &KzgSettings,
    ) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = commitments.len();
        if zs.len() != n || ys.len() != n || proofs.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let z: Vec<u8> = zs.iter().flat_map(|x| x.bytes).collect();
        let y: Vec<u8> = ys.iter().flat_map(|x| x.bytes).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe { ffi::kzg355_verify_kzg_proof_many(ok.as_mut_ptr(), st.as_mut_ptr(), c.as_ptr(), z.as_ptr(), y.as_ptr(), p.as_ptr(), n, s.raw) };
        whole_call(rc, &st[..n], "verify_kzg_proof_many")?;
        Ok((0..n).map(|i| check(st[i], "verify").map(|_| ok[i])).collect())
    }

    /// `blobs.len()` independent `verify_blob_kzg_proof` checks.
    pub fn verify_blob_kzg_proof_many(blobs: &[Blob], commitments: &[KzgCommitment], proofs: &[KzgProof], s: &KzgSettings) -> Result<Vec<Result<bool, Error>>, Error> {
        let n = blobs.len();
        if commitments.len() != n || proofs.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let staged = stage_blobs(blobs);
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|x| x.to_bytes()).collect();
        let mut ok = vec![false; n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe { ffi::kzg355_verify_blob_kzg_proof_many(ok.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), c.as_ptr(), p.as_ptr(), n, s.raw) };
        whole_call(rc, &st[..n], "verify_blob_kzg_proof_many")?;
        Ok((0..n).map(|i| check(st[i], "verify").map(|_| ok[i])).collect())
    }

    /// `blobs.len()` independent `compute_kzg_proof` calls: proof and y = p(z) per blob at the caller's points.
    pub fn compute_kzg_proof_many(blobs: &[Blob], zs: &[Bytes32], s: &KzgSettings) -> Result<Vec<Result<(KzgProof, Bytes32), Error>>, Error> {
        let n = blobs.len();
        if zs.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let staged = stage_blobs(blobs);
        let z: Vec<u8> = zs.iter().flat_map(|x| x.bytes).collect();
        let mut out = vec![0u8; BYTES_PER_PROOF * n.max(1)];
        let mut ys = vec![0u8; 32 * n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe { ffi::kzg355_compute_kzg_proof_many(out.as_mut_ptr(), ys.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), z.as_ptr(), n, s.raw) };
        whole_call(rc, &st[..n], "compute_kzg_proof_many")?;
        Ok((0..n)
            .map(|i| {
                check(st[i], "proof").map(|_| {
                    (
                        KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&out[48 * i..48 * i + 48]).unwrap()),
                        Bytes32::from(<[u8; 32]>::try_from(&ys[32 * i..32 * i + 32]).unwrap()),
                    )
                })
            })
            .collect())
    }

    /// The blob opened at the points `zs` (any order, repeats allowed, inside the domain or not; at most 4096): entry `j` is what
    /// `compute_kzg_proof` returns for `(blob, zs[j])`, and the blob is handed over once.
    pub fn compute_kzg_proofs_at(blob: &Blob, zs: &[Bytes32], s: &KzgSettings) -> Result<(Vec<KzgProof>, Vec<Bytes32>), Error> {
        let mut res = Self::compute_kzg_proofs_at_many(std::slice::from_ref(blob), &[zs], s)?;
        res.pop().unwrap_or(Err(Error::InternalError))
    }

    /// One independent `compute_kzg_proofs_at` per blob, each with its own list of points (which may be empty), in one set of launches.  One
    /// `Result` per blob; `blobs` and `point_lists` of different lengths are `BadArgs` for the call.
    pub fn compute_kzg_proofs_at_many(
        blobs: &[Blob],
        point_lists: &[&[Bytes32]],
        s: &KzgSettings,
    ) -> Result<Vec<Result<(Vec<KzgProof>, Vec<Bytes32>), Error>>, Error> {
        let n = blobs.len();
        if point_lists.len() != n {
            return Err(Error::BadArgs("length mismatch".into()));
        }
        let staged = stage_blobs(blobs);
        let counts: Vec<usize> = point_lists.iter().map(|zs| zs.len()).collect();
        let z: Vec<u8> = point_lists.iter().flat_map(|zs| zs.iter().flat_map(|x| x.bytes)).collect();
        let total = z.len() / 32;
        let mut proofs = vec![0u8; BYTES_PER_PROOF * total.max(1)];
        let mut ys = vec![0u8; 32 * total.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe {
            ffi::kzg355_compute_kzg_proofs_at_many(proofs.as_mut_ptr(), ys.as_mut_ptr(), st.as_mut_ptr(), staged.as_ptr(), n, counts.as_ptr(), z.as_ptr(),
                                                   s.raw)
        };
        whole_call(rc, &st[..n], "compute_kzg_proofs_at_many")?;
        let mut off = 0usize;
        Ok((0..n)
            .map(|i| {
                let (lo, hi) = (off, off + counts[i]);
                off = hi;
                check(st[i], "compute_kzg_proofs_at")?;
                let ps = (lo..hi).map(|j| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&proofs[48 * j..48 * (j + 1)]).unwrap())).collect();
                let vs = (lo..hi).map(|j| Bytes32::from(<[u8; 32]>::try_from(&ys[32 * j..32 * (j + 1)]).unwrap())).collect();
                Ok((ps, vs))
            })
            .collect())
    }

    /// `kzg_to_versioned_hash` of EIP-4844 per commitment, on the host: `0x01 || sha256(commitment)[1..]`.  No handle, no device; nothing is validated.
    pub fn kzg_to_versioned_hash_many(commitments: &[KzgCommitment]) -> Result<Vec<Bytes32>, Error> {
        let n = commitments.len();
        let c: Vec<u8> = commitments.iter().flat_map(|x| x.to_bytes()).collect();
        let mut out = vec![0u8; 32 * n.max(1)];
        check(unsafe { ffi::kzg355_kzg_to_versioned_hash_many(out.as_mut_ptr(), c.as_ptr(), n) }, "kzg_to_versioned_hash_many")?;
        Ok((0..n).map(|i| Bytes32::from(<[u8; 32]>::try_from(&out[32 * i..32 * i + 32]).unwrap())).collect())
    }

    /// The versioned hash of one commitment.
    pub fn kzg_to_versioned_hash(commitment: &KzgCommitment) -> Result<Bytes32, Error> {
        Ok(Self::kzg_to_versioned_hash_many(std::slice::from_ref(commitment))?.remove(0))
    }

    /// The same on device memory: `d_commitments` (`n * 48` bytes) to `d_out` (`n * 32` bytes).
    ///
    /// # Safety
    /// Both are device pointers on the handle's first device, `d_out` 16-byte and `d_commitments` 4-byte aligned, valid for the call.
    pub unsafe fn kzg_to_versioned_hash_many_device(d_out: *mut u8, d_commitments: *const u8, n: usize, s: &KzgSettings) -> Result<(), Error> {
        check(ffi::kzg355_kzg_to_versioned_hash_many_device(d_out, d_commitments, n, s.raw), "kzg_to_versioned_hash_many_device")
    }

    /// `inputs.len()` inputs of the EIP-4844 point-evaluation precompile (`versioned_hash | z | y | commitment | proof`) in one call.  Per input:
    /// what `verify_kzg_proof_many` gives for its four fields, and whether its versioned hash is that of its commitment.  An input whose hash
    /// does not match is `Ok(false)` and nothing else about it is reported: the precompile fails at the hash before it looks at the rest.
    pub fn point_evaluation_many(inputs: &[[u8; BYTES_PER_POINT_EVALUATION_INPUT]], s: &KzgSettings) -> Result<Vec<(Result<bool, Error>, bool)>, Error> {
        let n = inputs.len();
        let staged: Vec<u8> = inputs.iter().flat_map(|x| x.iter().copied()).collect();
        let mut ok = vec![false; n.max(1)];
        let mut matched = vec![false; n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = unsafe { ffi::kzg355_point_evaluation_many(ok.as_mut_ptr(), st.as_mut_ptr(), matched.as_mut_ptr(), staged.as_ptr(), n, s.raw) };
        whole_call(rc, &st[..n], "point_evaluation_many")?;
        Ok((0..n).map(|i| (check(st[i], "point_evaluation").map(|_| ok[i]), matched[i])).collect())
    }

    /// `point_evaluation_many` on `n` inputs in device memory.
    ///
    /// # Safety
    /// `d_inputs` is a device pointer on the handle's first device to `n * 192` bytes, 16-byte aligned, valid for the call; it is only read.
    pub unsafe fn point_evaluation_many_device(d_inputs: *const u8, n: usize, s: &KzgSettings) -> Result<Vec<(Result<bool, Error>, bool)>, Error> {
        let mut ok = vec![false; n.max(1)];
        let mut matched = vec![false; n.max(1)];
        let mut st = vec![0i32; n.max(1)];
        let rc = ffi::kzg355_point_evaluation_many_device(ok.as_mut_ptr(), st.as_mut_ptr(), matched.as_mut_ptr(), d_inputs, n, s.raw);
        whole_call(rc, &st[..n], "point_evaluation_many_device")?;
        Ok((0..n).map(|i| (check(st[i], "point_evaluation").map(|_| ok[i]), matched[i])).collect())
    }

    /// One precompile call as EIP-4844 words it: `u256be(FIELD_ELEMENTS_PER_BLOB) | u256be(BLS_MODULUS)` on success; `BadArgs` on an input that
    /// is not 192 bytes, a hash mismatch, an invalid input or a false proof.
    pub fn point_evaluation(input: &[u8], s: &KzgSettings) -> Result<[u8; 64], Error> {
        let mut out = [0u8; 64];
        check(unsafe { ffi::kzg355_point_evaluation(out.as_mut_ptr(), input.as_ptr(), input.len(), s.raw) }, "point_evaluation")?;
        Ok(out)
    }
}

/// `&[Blob]` is a slice of boxes: the blobs are not contiguous in memory, the ABI wants one buffer.
fn stage_blobs(blobs: &[Blob]) -> Vec<u8> {
    let mut staged = Vec::with_capacity(blobs.len() * BYTES_PER_BLOB);
    for b in blobs {
        staged.extend_from_slice(&b[..]);
    }
    staged
}

/// The host output buffers of a `*_commitment_cells_and_kzg_proofs_many*` call of `n` blobs, and their way into one `Result` per blob.
struct CommitCellsProofs {
    commitments: Vec<u8>,
    cells: Vec<u8>,
    proofs: Vec<u8>,
    st: Vec<i32>,
}

impl CommitCellsProofs {
    fn new(n: usize) -> Self {
        CommitCellsProofs {
            commitments: vec![0u8; BYTES_PER_COMMITMENT * n.max(1)],
            cells: vec![0u8; BYTES_PER_CELL * CELLS_PER_EXT_BLOB * n.max(1)],
            proofs: vec![0u8; BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * n.max(1)],
            st: vec![0i32; n.max(1)],
        }
    }

    fn unpack(&self, n: usize, what: &str) -> Vec<Result<(KzgCommitment, Vec<Cell>, Vec<KzgProof>), Error>> {
        let per_cells = BYTES_PER_CELL * CELLS_PER_EXT_BLOB;
        (0..n)
            .map(|i| {
                check(self.st[i], what)?;
                let c = KzgCommitment::from(<[u8; BYTES_PER_COMMITMENT]>::try_from(&self.commitments[48 * i..48 * i + 48]).unwrap());
                let cs = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| Cell::from_bytes(&self.cells[per_cells * i + BYTES_PER_CELL * k..per_cells * i + BYTES_PER_CELL * (k + 1)]))
                    .collect::<Result<Vec<_>, _>>()?;
                let base = BYTES_PER_PROOF * CELLS_PER_EXT_BLOB * i;
                let ps = (0..CELLS_PER_EXT_BLOB)
                    .map(|k| KzgProof::from(<[u8; BYTES_PER_PROOF]>::try_from(&self.proofs[base + 48 * k..base + 48 * (k + 1)]).unwrap()))
                    .collect();
                Ok((c, cs, ps))
            })
            .collect()
    }
}

/// A `*_many` call that failed as a whole (device, allocation or library failure -- or a non-zero return with no unit carrying a
/// status) is an `Err` of the call; per-unit statuses are then not to be trusted.
fn whole_call(rc: i32, st: &[i32], what: &str) -> Result<(), Error> {
    let whole = matches!(rc, ffi::KZG355_INTERNAL | ffi::KZG355_NO_DEVICE | ffi::KZG355_NO_MEMORY | ffi::KZG355_DEVICE_ERROR);
    if whole || (rc != ffi::KZG355_OK && st.iter().all(|&x| x == 0)) {
        return check(rc, what);
    }
    Ok(())
}
