"""Host-side mirror of the reference's public surface (pawanjay176/kzg_rust src/kzg.rs:10-22, 88-279,
983-1079) over the C ABI of libkzg355.so.  Same names, same argument meaning, same error behaviour, so the
parity tests read like the reference's own (src/lib.rs:30-203).  All arithmetic happens in the HIP library;
this module only checks lengths / hex (as the Rust newtypes do before any FFI) and forwards.

The reference's host language is Rust; no Rust toolchain exists in this image, so the shim a maintainer
would compile is in rust/ (source only, see rust/README.md) -- this Python mirror is what the test-suite drives.
"""
import ctypes as C
import os

from . import _lib

BYTES_PER_FIELD_ELEMENT = 32      # consts.rs:5
BYTES_PER_COMMITMENT = 48         # consts.rs:8
BYTES_PER_PROOF = 48              # consts.rs:11
FIELD_ELEMENTS_PER_BLOB = 4096    # consts.rs:13
BYTES_PER_BLOB = 131072           # consts.rs:16
BYTES_PER_G1 = 48                 # consts.rs:31
BYTES_PER_G2 = 96                 # consts.rs:34
TRUSTED_SETUP_NUM_G2_POINTS = 65  # consts.rs:37
# EIP-7594 (PeerDAS) cells: 64 field elements of a blob's 2x Reed-Solomon extension
FIELD_ELEMENTS_PER_CELL = 64
BYTES_PER_CELL = 2048
BYTES_PER_POINT_EVALUATION_INPUT = 192   # versioned_hash | z | y | commitment | proof (EIP-4844, point_evaluation_precompile)
CELLS_PER_EXT_BLOB = 128


class Error(Exception):
    """enum Error (kzg.rs:10-22)."""
    code = None


class BadArgs(Error):
    code = 1


class InternalError(Error):
    code = 2


class InvalidBytesLength(Error):
    code = 3


class InvalidHexFormat(Error):
    code = 4


class InvalidTrustedSetup(Error):
    code = 5


class NoDevice(Error):
    """No usable HIP device (no reference counterpart; there is no CPU fallback)."""
    code = 6


class NoMemory(Error):
    """A device or pinned-host allocation failed (no reference counterpart)."""
    code = 7


class DeviceError(Error):
    """A HIP runtime / RCCL call failed on a device that exists (no reference counterpart)."""
    code = 8


_ERRORS = {c.code: c for c in (BadArgs, InternalError, InvalidBytesLength, InvalidHexFormat, InvalidTrustedSetup, NoDevice, NoMemory, DeviceError)}
# statuses that can only describe the call as a whole (a device, allocation or library failure): a *_many call that returns one of
# them may have left units untouched, so it is raised even when earlier units carry a per-unit status
_WHOLE_CALL = (InternalError.code, NoDevice.code, NoMemory.code, DeviceError.code)


def _whole_call_failed(rc, st, n):
    return rc in _WHOLE_CALL or (rc != 0 and not any(st[i] for i in range(n)))


def _check(rc, what):
    if rc != 0:
        raise _ERRORS.get(rc, InternalError)(f"{what}: status {rc}")


def hex_to_bytes(hex_str):
    """kzg.rs:82-86: hex with or without the 0x prefix."""
    s = hex_str[2:] if hex_str.startswith("0x") else hex_str
    try:
        return bytes.fromhex(s)
    except ValueError as e:
        raise InvalidHexFormat(f"Failed to decode hex: {e}")


class _Fixed:
    SIZE = 0
    LENGTH_ERROR = InvalidBytesLength

    def __init__(self, b):
        b = bytes(b)
        if len(b) != self.SIZE:
            raise self.LENGTH_ERROR(f"Invalid byte length. Expected {self.SIZE} got {len(b)}")
        self.bytes = b

    @classmethod
    def from_bytes(cls, b):
        return cls(b)

    @classmethod
    def from_hex(cls, s):
        return cls(hex_to_bytes(s))

    def to_bytes(self):
        return self.bytes

    def __bytes__(self):
        return self.bytes

    def __eq__(self, other):
        return isinstance(other, _Fixed) and self.bytes == other.bytes

    def __hash__(self):
        return hash(self.bytes)

    def __repr__(self):
        return f"{type(self).__name__}(0x{self.bytes[:8].hex()}..)"


class Bytes32(_Fixed):
    """kzg.rs:101-122 (length error is BadArgs for this type)."""
    SIZE = 32
    LENGTH_ERROR = BadArgs


class Bytes48(_Fixed):
    """kzg.rs:124-152."""
    SIZE = 48


class Blob(_Fixed):
    """kzg.rs:154-178 (mainnet preset: 4096 field elements; kzg_rust_amd.kzg_minimal.Blob is the 4-element one)."""
    SIZE = BYTES_PER_BLOB


class Cell(_Fixed):
    """One EIP-7594 cell: 64 big-endian field elements (2048 bytes)."""
    SIZE = BYTES_PER_CELL


class KzgCommitment(Bytes48):
    """kzg.rs:180-191."""


class KzgProof(Bytes48):
    """kzg.rs:193-204."""


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _lib.load()
    return _LIB


class KzgSettings:
    """Opaque handle to the device-resident trusted setup (replaces struct KzgSettings, kzg.rs:28-40)."""

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        if self._h is None:
            raise BadArgs("KzgSettings already freed")
        return self._h

    @staticmethod
    def load_trusted_setup(g1_bytes, g2_bytes, devices=None):
        """kzg.rs:45-78: lists of 48-byte / 96-byte strings.  devices (extension): list of GPU ordinals the handle spans; the
        host-buffer calls then spread their work over them inside the library."""
        g1_bytes, g2_bytes = list(g1_bytes), list(g2_bytes)
        if any(len(x) != BYTES_PER_G1 for x in g1_bytes) or any(len(x) != BYTES_PER_G2 for x in g2_bytes):
            raise InvalidBytesLength("trusted setup point length")
        h = C.c_void_p()
        if devices is None:
            rc = lib().kzg355_load_trusted_setup(b"".join(g1_bytes), len(g1_bytes), b"".join(g2_bytes), len(g2_bytes), C.byref(h))
        else:
            devs = (C.c_int * len(devices))(*devices)
            rc = lib().kzg355_load_trusted_setup_devices(b"".join(g1_bytes), len(g1_bytes), b"".join(g2_bytes), len(g2_bytes), devs, len(devices), C.byref(h))
        _check(rc, "load_trusted_setup")
        return KzgSettings(h)

    @staticmethod
    def load_trusted_setup_ex(g1_bytes, g2_bytes, devices=None, **options):
        """kzg355_load_trusted_setup_ex: explicit options (field names of struct kzg355_options, e.g. msm_bits=14, host_hash=-1); reads no
        KZG355_* environment variable."""
        g1_bytes, g2_bytes = list(g1_bytes), list(g2_bytes)
        if any(len(x) != BYTES_PER_G1 for x in g1_bytes) or any(len(x) != BYTES_PER_G2 for x in g2_bytes):
            raise InvalidBytesLength("trusted setup point length")
        o = _lib.Options()
        lib().kzg355_options_default(C.byref(o))
        for k, v in options.items():
            if k == "struct_size" or not hasattr(o, k):
                raise BadArgs(f"unknown option {k}")
            setattr(o, k, v)
        devs = (C.c_int * len(devices))(*devices) if devices else None
        h = C.c_void_p()
        rc = lib().kzg355_load_trusted_setup_ex(b"".join(g1_bytes), len(g1_bytes), b"".join(g2_bytes), len(g2_bytes), devs, len(devices) if devices else 0,
                                                C.byref(o), C.byref(h))
        _check(rc, "load_trusted_setup_ex")
        return KzgSettings(h)

    @staticmethod
    def load_trusted_setup_file(path):
        h = C.c_void_p()
        rc = lib().kzg355_load_trusted_setup_file(os.fsencode(path), C.byref(h))
        _check(rc, "load_trusted_setup_file")
        return KzgSettings(h)

    @property
    def device(self):
        return lib().kzg355_settings_device(self.handle)

    @property
    def device_count(self):
        return lib().kzg355_settings_device_count(self.handle)

    def exchange_stats(self):
        """(exchange kind: 1 RCCL all-gather, 0 peer copies, -1 plain handle; all-gathers so far; peer exchanges so far)."""
        a, p = C.c_long(), C.c_long()
        kind = lib().kzg355_settings_exchange_stats(self.handle, C.byref(a), C.byref(p))
        return kind, a.value, p.value

    @property
    def field_elements_per_blob(self):
        """4096 (mainnet) or 4 (minimal preset): fixed by the number of G1 points the handle was loaded from."""
        return lib().kzg355_settings_field_elements_per_blob(self.handle)

    def msm_shape(self):
        """(digit width, windows per half-scalar, GLV split 0 / 1, table bytes) of the fixed-base MSM table; all 0 while it has not been built."""
        b, w, g, n = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        _check(lib().kzg355_settings_msm_shape(self.handle, C.byref(b), C.byref(w), C.byref(g), C.byref(n)), "msm_shape")
        return b.value, w.value, g.value, n.value

    def build_msm_table(self):
        """Build the fixed-base MSM table now instead of inside the first commitment / proof call."""
        _check(lib().kzg355_settings_build_msm_table(self.handle), "build_msm_table")

    @property
    def msm_form(self):
        """12 / 13 / 14: wide-window table of that digit width; 8: bucket form by request; -8: bucket form because the table
        could not be allocated."""
        return lib().kzg355_settings_msm_form(self.handle)

    def set_host_hash(self, mode, max_blobs=0):
        """Fiat-Shamir hashing of small host-buffer calls on host threads: mode 0 by size, 1 always, -1 never (kzg355.h)."""
        _check(lib().kzg355_settings_set_host_hash(self.handle, mode, max_blobs), "set_host_hash")

    @property
    def host_hashed_calls(self):
        return lib().kzg355_settings_host_hashed_calls(self.handle)

    @property
    def cell_device_prep_calls(self):
        """Device-resident cell verify calls on this handle that were prepared on the device so far."""
        return lib().kzg355_settings_cell_device_prep_calls(self.handle)

    def cell_calls_per_device(self):
        """One count per device of the handle: the cell launch sets (verify, compute, recover; a block of a verify call cut over the devices
        counts too) that device has run so far."""
        n = self.device_count
        out = (C.c_long * n)()
        if lib().kzg355_settings_cell_calls_per_device(self.handle, out, n) != n:
            raise BadArgs("cell_calls_per_device")
        return list(out)

    def set_blob_sets_max_blobs(self, max_blobs=0):
        """Blobs per launch set of verify_blob_kzg_proof_batch_many_sets and its forms on this handle (0: the default, 32768)."""
        _check(lib().kzg355_settings_set_blob_sets_max_blobs(self.handle, max_blobs), "set_blob_sets_max_blobs")

    def blob_sets_blobs_per_device(self):
        """One count per device of the handle: the blobs that device has run through verify_blob_kzg_proof_batch_many_sets and its forms."""
        n = self.device_count
        out = (C.c_long * n)()
        if lib().kzg355_settings_blob_sets_blobs_per_device(self.handle, out, n) != n:
            raise BadArgs("blob_sets_blobs_per_device")
        return list(out)

    @property
    def host_threads(self):
        """host threads that hash for one call on this handle (its workers + the calling thread)"""
        return lib().kzg355_settings_host_threads(self.handle)

    def set_kernel_timing(self, enabled=True):
        lib().kzg355_set_kernel_timing(self.handle, 1 if enabled else 0)

    def last_kernel_ms(self, family):
        return lib().kzg355_last_kernel_ms(self.handle, family.encode())

    def free(self):
        if self._h is not None:
            lib().kzg355_free_trusted_setup(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _b(x, cls):
    return x.bytes if isinstance(x, _Fixed) else cls(x).bytes


def _blob(x, s):
    """Blob bytes for the handle's preset: the newtype's length rule (kzg.rs:160-173) with BYTES_PER_BLOB = 32 * FIELD_ELEMENTS_PER_BLOB."""
    b = x.bytes if isinstance(x, _Fixed) else bytes(x)
    want = 32 * s.field_elements_per_blob
    if len(b) != want:
        raise InvalidBytesLength(f"Invalid byte length. Expected {want} got {len(b)}")
    return b


# ---- what the wrappers of the EIP-7594 cell calls share
def _size_t_arrays(counts, indices, message):
    """Host sequences as c_size_t arrays, (counts, indices), or BadArgs(message): every value is within 0 <= v < 2^64 and the counts (None: the
    call takes none) add up to the indices."""
    cn, ix = None if counts is None else [int(c) for c in counts], [int(i) for i in indices]
    if any(v < 0 or v >= 1 << 64 for v in (cn or []) + ix) or (cn is not None and sum(cn) != len(ix)):
        raise BadArgs(message)
    return None if cn is None else (C.c_size_t * max(len(cn), 1))(*cn), (C.c_size_t * max(len(ix), 1))(*ix)


def _cell_buffers(cells, proofs, slots, units):
    """(cells_out, proofs_out, statuses) of a host-form call with `slots` output slots in all; None for an output that is not asked for"""
    return (C.create_string_buffer(BYTES_PER_CELL * max(slots, 1)) if cells else None, C.create_string_buffer(48 * max(slots, 1)) if proofs else None,
            (C.c_int * max(units, 1))())


def _cell_results(rc, st, slots, c_out, p_out, call, label):
    """What a host-form call returns: per unit (cells, proofs) out of the call's output buffers, unit i owning the next slots[i] slots, or
    Error(label); a failure of the whole call raises."""
    if _whole_call_failed(rc, st, len(slots)):
        _check(rc, call)
    craw, praw = (None if b is None else b.raw for b in (c_out, p_out))      # (.raw copies the whole buffer: once)
    res, off = [], 0
    for i, k in enumerate(slots):
        if st[i] != 0:
            res.append(_ERRORS.get(st[i], InternalError)(label))
        else:
            res.append(([Cell(craw[BYTES_PER_CELL * j:BYTES_PER_CELL * (j + 1)]) for j in range(off, off + k)] if craw is not None else None,
                        [KzgProof(praw[48 * j:48 * (j + 1)]) for j in range(off, off + k)] if praw is not None else None))
        off += k
    return res


def _commitment_cell_results(rc, st, units, k_out, c_out, p_out, call, label):
    """_cell_results of a call that also returns a commitment per unit: (commitment, cells, proofs) or Error(label) per unit, None for a part
    that was not asked for"""
    res = _cell_results(rc, st, [CELLS_PER_EXT_BLOB] * units, c_out, p_out, call, label)
    kraw = None if k_out is None else k_out.raw
    return [r if isinstance(r, Error) else ((KzgCommitment(kraw[48 * i:48 * i + 48]) if kraw is not None else None,) + r) for i, r in enumerate(res)]


def _device_results(rc, st, units, call, label):
    """What a device form returns: per unit None or Error(label); a failure of the whole call raises."""
    if _whole_call_failed(rc, st, units):
        _check(rc, call)
    return [None if st[i] == 0 else _ERRORS.get(st[i], InternalError)(label) for i in range(units)]


class Kzg:
    """pub struct Kzg (kzg.rs:983-1079): the seven associated functions, forwarded to the HIP engine."""

    @staticmethod
    def load_trusted_setup_file(path):  # kzg.rs:995
        return KzgSettings.load_trusted_setup_file(path)

    @staticmethod
    def load_trusted_setup(g1_bytes, g2_bytes, devices=None):  # kzg.rs:1005
        return KzgSettings.load_trusted_setup(g1_bytes, g2_bytes, devices)

    @staticmethod
    def blob_to_kzg_commitment(blob, s):  # kzg.rs:1013
        out = C.create_string_buffer(48)
        _check(lib().kzg355_blob_to_kzg_commitment(out, _blob(blob, s), s.handle), "blob_to_kzg_commitment")
        return KzgCommitment(out.raw)

    @staticmethod
    def compute_kzg_proof(blob, z_bytes, s):  # kzg.rs:1021
        pr, y = C.create_string_buffer(48), C.create_string_buffer(32)
        _check(lib().kzg355_compute_kzg_proof(pr, y, _blob(blob, s), _b(z_bytes, Bytes32), s.handle), "compute_kzg_proof")
        return KzgProof(pr.raw), Bytes32(y.raw)

    @staticmethod
    def compute_blob_kzg_proof(blob, commitment, s):  # kzg.rs:1030
        pr = C.create_string_buffer(48)
        _check(lib().kzg355_compute_blob_kzg_proof(pr, _blob(blob, s), _b(commitment, KzgCommitment), s.handle), "compute_blob_kzg_proof")
        return KzgProof(pr.raw)

    @staticmethod
    def verify_kzg_proof(commitment, z_bytes, y_bytes, proof, s):  # kzg.rs:1039
        ok = C.c_bool()
        _check(lib().kzg355_verify_kzg_proof(C.byref(ok), _b(commitment, KzgCommitment), _b(z_bytes, Bytes32), _b(y_bytes, Bytes32),
                                             _b(proof, KzgProof), s.handle), "verify_kzg_proof")
        return bool(ok.value)

    @staticmethod
    def verify_blob_kzg_proof(blob, commitment, proof, s):  # kzg.rs:1050
        ok = C.c_bool()
        _check(lib().kzg355_verify_blob_kzg_proof(C.byref(ok), _blob(blob, s), _b(commitment, KzgCommitment), _b(proof, KzgProof), s.handle),
               "verify_blob_kzg_proof")
        return bool(ok.value)

    @staticmethod
    def verify_blob_kzg_proof_batch(blobs, commitments, proofs, s):  # kzg.rs:1066
        bl = [_blob(x, s) for x in blobs]
        cs = [_b(x, KzgCommitment) for x in commitments]
        ps = [_b(x, KzgProof) for x in proofs]
        ok = C.c_bool()
        _check(lib().kzg355_verify_blob_kzg_proof_batch(C.byref(ok), b"".join(bl), len(bl), b"".join(cs), len(cs), b"".join(ps), len(ps),
                                                        s.handle), "verify_blob_kzg_proof_batch")
        return bool(ok.value)

    # ---- throughput extensions (no reference counterpart; same semantics per unit) ----
    @staticmethod
    def blob_to_kzg_commitment_many(blobs, s):
        bl = [_blob(x, s) for x in blobs]
        n = len(bl)
        out = C.create_string_buffer(48 * max(n, 1))
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_blob_to_kzg_commitment_many(out, st, b"".join(bl), n, s.handle)
        if _whole_call_failed(rc, st, n):                         # no device, out of memory, n too large: nothing usable came back
            _check(rc, "blob_to_kzg_commitment_many")
        return [KzgCommitment(out.raw[48 * i:48 * i + 48]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("commit") for i in range(n)]

    @staticmethod
    def compute_blob_kzg_proof_many(blobs, commitments, s):
        bl = [_blob(x, s) for x in blobs]
        cs = [_b(x, KzgCommitment) for x in commitments]
        if len(bl) != len(cs):
            raise BadArgs("length mismatch")
        n = len(bl)
        out = C.create_string_buffer(48 * max(n, 1))
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_blob_kzg_proof_many(out, st, b"".join(bl), b"".join(cs), n, s.handle)
        if _whole_call_failed(rc, st, n):
            _check(rc, "compute_blob_kzg_proof_many")
        return [KzgProof(out.raw[48 * i:48 * i + 48]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("proof") for i in range(n)]

    @staticmethod
    def verify_blob_kzg_proof_batch_many(groups, s):
        """groups: list of (blobs, commitments, proofs) with equal group sizes.  Returns a list of bool / Error."""
        if not groups:
            return []
        npg = len(groups[0][0])
        flat_b, flat_c, flat_p = [], [], []
        for bl, cs, ps in groups:
            if not (len(bl) == len(cs) == len(ps) == npg):
                raise BadArgs("all groups must have the same size")
            flat_b += [_blob(x, s) for x in bl]
            flat_c += [_b(x, KzgCommitment) for x in cs]
            flat_p += [_b(x, KzgProof) for x in ps]
        G = len(groups)
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        rc = lib().kzg355_verify_blob_kzg_proof_batch_many(ok, st, b"".join(flat_b), b"".join(flat_c), b"".join(flat_p), npg, G, s.handle)
        if _whole_call_failed(rc, st, G):                         # whole-call failure: the per-batch statuses are not to be trusted
            _check(rc, "verify_blob_kzg_proof_batch_many")
        return [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify") for i in range(G)]

    @staticmethod
    def _blob_sets(groups, s, debug):
        flat = [[], [], []]
        counts = []
        for blobs, commitments, proofs in groups:
            arrs = ([_blob(x, s) for x in blobs], [_b(x, KzgCommitment) for x in commitments], [_b(x, KzgProof) for x in proofs])
            n = len(arrs[0])
            if len(arrs[1]) != n or len(arrs[2]) != n:            # kzg.rs:644-651, before any FFI call
                raise BadArgs("length mismatch")
            counts.append(n)
            for f, a in zip(flat, arrs):
                f += a
        G = len(counts)
        ok = (C.c_bool * max(G, 1))()
        st = (C.c_int * max(G, 1))()
        cnt = (C.c_size_t * max(G, 1))(*counts)
        args = (ok, st, cnt, b"".join(flat[0]), b"".join(flat[1]), b"".join(flat[2]), G, s.handle)
        out = C.create_string_buffer(128 * max(G, 1)) if debug else None
        rc = lib().kzg355_debug_batch_intermediates_sets(out, *args) if debug else lib().kzg355_verify_blob_kzg_proof_batch_many_sets(*args)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_blob_kzg_proof_batch_many_sets")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_blob_kzg_proof_batch_many_sets(groups, s):
        """verify_blob_kzg_proof_batch_many for groups of any sizes (an empty group is True): list of (blobs, commitments, proofs), one
        independent verify_blob_kzg_proof_batch per group, each with its own challenge r.  Returns a list of bool / Error."""
        return Kzg._blob_sets(groups, s, False)[0]

    @staticmethod
    def debug_batch_intermediates_sets(groups, s):
        """(verdicts as verify_blob_kzg_proof_batch_many_sets, [r (32) | proof_lincomb (48) | rhs (48) per group; zero bytes for an empty group])"""
        res, raw = Kzg._blob_sets(groups, s, True)
        return res, [raw[128 * i:128 * i + 128] for i in range(len(res))]

    @staticmethod
    def _blob_sets_device(blobs, commitments, proofs, blob_counts, s, debug):
        counts = [int(c) for c in blob_counts]
        if any(c < 0 for c in counts):
            raise BadArgs("blob_counts out of range")
        nb, G = sum(counts), len(counts)
        ptrs = (Kzg._dev(blobs, "blobs", 32 * s.field_elements_per_blob * nb, optional=nb == 0), Kzg._dev(commitments, "commitments", 48 * nb, optional=nb == 0),
                Kzg._dev(proofs, "proofs", 48 * nb, optional=nb == 0))
        if G == 0:
            return [], b""
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        cnt = (C.c_size_t * G)(*counts)
        out = C.create_string_buffer(128 * G) if debug else None
        if debug:
            rc = lib().kzg355_debug_batch_intermediates_sets_device(out, ok, st, cnt, *ptrs, G, s.handle)
        else:
            rc = lib().kzg355_verify_blob_kzg_proof_batch_many_sets_device(ok, st, cnt, *ptrs, G, s.handle)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_blob_kzg_proof_batch_many_sets_device")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_blob_kzg_proof_batch_many_sets_device(blobs, commitments, proofs, blob_counts, s):
        """verify_blob_kzg_proof_batch_many_sets on device memory: blobs (sum(blob_counts) blobs, uint8), commitments and proofs (* 48), group
        after group with no padding; blob_counts is a host list.  Returns a list of bool / Error per group."""
        return Kzg._blob_sets_device(blobs, commitments, proofs, blob_counts, s, False)[0]

    @staticmethod
    def debug_batch_intermediates_sets_device(blobs, commitments, proofs, blob_counts, s):
        """(verdicts, [128 bytes per group]) as debug_batch_intermediates_sets, on device memory"""
        res, raw = Kzg._blob_sets_device(blobs, commitments, proofs, blob_counts, s, True)
        return res, [raw[128 * i:128 * i + 128] for i in range(len(res))]

    @staticmethod
    def verify_kzg_proof_many(commitments, zs, ys, proofs, s):
        """n independent verify_kzg_proof checks (kzg.rs:1039) in one call.  Returns a list of bool / Error."""
        cs = [_b(x, KzgCommitment) for x in commitments]
        zz = [_b(x, Bytes32) for x in zs]
        yy = [_b(x, Bytes32) for x in ys]
        ps = [_b(x, KzgProof) for x in proofs]
        n = len(cs)
        if not (len(zz) == len(yy) == len(ps) == n):
            raise BadArgs("length mismatch")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_verify_kzg_proof_many(ok, st, b"".join(cs), b"".join(zz), b"".join(yy), b"".join(ps), n, s.handle)
        if _whole_call_failed(rc, st, n):
            _check(rc, "verify_kzg_proof_many")
        return [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify") for i in range(n)]

    @staticmethod
    def verify_blob_kzg_proof_many(blobs, commitments, proofs, s):
        """n independent verify_blob_kzg_proof checks (kzg.rs:1050) in one call.  Returns a list of bool / Error."""
        bl = [_blob(x, s) for x in blobs]
        cs = [_b(x, KzgCommitment) for x in commitments]
        ps = [_b(x, KzgProof) for x in proofs]
        n = len(bl)
        if not (len(cs) == len(ps) == n):
            raise BadArgs("length mismatch")
        ok = (C.c_bool * max(n, 1))()
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_verify_blob_kzg_proof_many(ok, st, b"".join(bl), b"".join(cs), b"".join(ps), n, s.handle)
        if _whole_call_failed(rc, st, n):
            _check(rc, "verify_blob_kzg_proof_many")
        return [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify") for i in range(n)]

    @staticmethod
    def compute_kzg_proof_many(blobs, zs, s):
        """n independent compute_kzg_proof calls (kzg.rs:1021) in one call.  Returns a list of (KzgProof, Bytes32) / Error."""
        bl = [_blob(x, s) for x in blobs]
        zz = [_b(x, Bytes32) for x in zs]
        n = len(bl)
        if len(zz) != n:
            raise BadArgs("length mismatch")
        out = C.create_string_buffer(48 * max(n, 1))
        ys = C.create_string_buffer(32 * max(n, 1))
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_kzg_proof_many(out, ys, st, b"".join(bl), b"".join(zz), n, s.handle)
        if _whole_call_failed(rc, st, n):
            _check(rc, "compute_kzg_proof_many")
        return [(KzgProof(out.raw[48 * i:48 * i + 48]), Bytes32(ys.raw[32 * i:32 * i + 32])) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("proof")
                for i in range(n)]

    # ---- the EIP-4844 point-evaluation precompile (address 0x0A): an input is versioned_hash (32) | z (32) | y (32) | commitment (48) | proof (48) ----
    @staticmethod
    def kzg_to_versioned_hash_many(commitments):
        """0x01 || sha256(commitment)[1:] per commitment, on the host (no handle, no device; nothing is validated).  Returns a list of 32-byte hashes."""
        cs = [_b(x, KzgCommitment) for x in commitments]
        n = len(cs)
        out = C.create_string_buffer(32 * max(n, 1))
        _check(lib().kzg355_kzg_to_versioned_hash_many(out, b"".join(cs), n), "kzg_to_versioned_hash_many")
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    @staticmethod
    def kzg_to_versioned_hash(commitment):
        """kzg_to_versioned_hash of EIP-4844: the 32-byte versioned hash of one commitment."""
        return Kzg.kzg_to_versioned_hash_many([commitment])[0]

    @staticmethod
    def kzg_to_versioned_hash_many_device(out, commitments, n, s):
        """The same on device memory: commitments (n * 48 bytes, uint8, 4-byte aligned) -> out (n * 32 bytes, uint8, 16-byte aligned), both on the
        handle's first device; out is written by a kernel of the library's own."""
        n = int(n)
        if n < 0:
            raise BadArgs("n out of range")
        ptrs = (Kzg._dev(out, "out", 32 * n, optional=n == 0), Kzg._dev(commitments, "commitments", 48 * n, optional=n == 0))
        _check(lib().kzg355_kzg_to_versioned_hash_many_device(*ptrs, n, s.handle), "kzg_to_versioned_hash_many_device")

    @staticmethod
    def _point_evaluation_results(rc, ok, st, match, n, call):
        if _whole_call_failed(rc, st, n):
            _check(rc, call)
        return [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("point_evaluation") for i in range(n)], [bool(match[i]) for i in range(n)]

    @staticmethod
    def point_evaluation_many(inputs, s):
        """n point-evaluation precompile inputs of 192 bytes in one call.  Returns (results, hash_match): per input True, False or an Error as
        verify_kzg_proof_many gives them, and whether its versioned hash is that of its commitment.  An input whose hash does not match is False
        and nothing else about it is reported (the precompile fails at the hash before it looks at the rest)."""
        data = [bytes(x) for x in inputs]
        if any(len(d) != BYTES_PER_POINT_EVALUATION_INPUT for d in data):
            raise BadArgs(f"point evaluation input: expected {BYTES_PER_POINT_EVALUATION_INPUT} bytes")
        n = len(data)
        if n == 0:
            return [], []
        ok, st, match = (C.c_bool * n)(), (C.c_int * n)(), (C.c_bool * n)()
        rc = lib().kzg355_point_evaluation_many(ok, st, match, b"".join(data), n, s.handle)
        return Kzg._point_evaluation_results(rc, ok, st, match, n, "point_evaluation_many")

    @staticmethod
    def point_evaluation_many_device(inputs, n, s):
        """point_evaluation_many on device memory: inputs (n * 192 bytes, uint8, 16-byte aligned) on the handle's first device, only read."""
        n = int(n)
        if n < 0:
            raise BadArgs("n out of range")
        ptr = Kzg._dev(inputs, "inputs", BYTES_PER_POINT_EVALUATION_INPUT * n, optional=n == 0)
        if n == 0:
            return [], []
        ok, st, match = (C.c_bool * n)(), (C.c_int * n)(), (C.c_bool * n)()
        rc = lib().kzg355_point_evaluation_many_device(ok, st, match, ptr, n, s.handle)
        return Kzg._point_evaluation_results(rc, ok, st, match, n, "point_evaluation_many_device")

    @staticmethod
    def point_evaluation(input, s):
        """One precompile call as EIP-4844 words it: the 64 bytes u256be(FIELD_ELEMENTS_PER_BLOB) | u256be(BLS_MODULUS) on success; BadArgs on an
        input that is not 192 bytes, a hash mismatch, an invalid input or a false proof."""
        data = bytes(input)
        if len(data) != BYTES_PER_POINT_EVALUATION_INPUT:
            raise BadArgs(f"point evaluation input: expected {BYTES_PER_POINT_EVALUATION_INPUT} bytes")
        out = C.create_string_buffer(64)
        _check(lib().kzg355_point_evaluation(out, data, len(data), s.handle), "point_evaluation")
        return out.raw

    # ---- EIP-7594 cell proofs (consensus specs fulu/polynomial-commitments-sampling.md; no reference counterpart) ----
    @staticmethod
    def _cell_arrays(commitments, cell_indices, cells, proofs):
        cs = [_b(x, KzgCommitment) for x in commitments]
        ix = [int(i) for i in cell_indices]
        cl = [_b(x, Cell) for x in cells]
        ps = [_b(x, KzgProof) for x in proofs]
        if not (len(cs) == len(ix) == len(cl) == len(ps)):
            raise BadArgs("length mismatch")
        if any(i < 0 or i >= 1 << 64 for i in ix):
            raise BadArgs("cell index out of range")
        return cs, ix, cl, ps

    @staticmethod
    def verify_cell_kzg_proof_batch(commitments, cell_indices, cells, proofs, s):
        """verify_cell_kzg_proof_batch: one commitment, cell index (< 128), cell and proof per cell; True / False, BadArgs on bad input."""
        cs, ix, cl, ps = Kzg._cell_arrays(commitments, cell_indices, cells, proofs)
        n = len(cs)
        ok = C.c_bool()
        idx = (C.c_size_t * max(n, 1))(*ix)
        _check(lib().kzg355_verify_cell_kzg_proof_batch(C.byref(ok), b"".join(cs), idx, b"".join(cl), b"".join(ps), n, s.handle),
               "verify_cell_kzg_proof_batch")
        return bool(ok.value)

    @staticmethod
    def _cell_many(groups, s, debug):
        if not groups:
            return [], b""
        npg = len(groups[0][0])
        flat = [[], [], [], []]
        for grp in groups:
            arrs = Kzg._cell_arrays(*grp)
            if len(arrs[0]) != npg:
                raise BadArgs("all groups must have the same size")
            for f, a in zip(flat, arrs):
                f += a
        G = len(groups)
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        idx = (C.c_size_t * max(len(flat[1]), 1))(*flat[1])
        args = (ok, st, b"".join(flat[0]), idx, b"".join(flat[2]), b"".join(flat[3]), npg, G, s.handle)
        out = C.create_string_buffer(176 * G) if debug else None
        rc = lib().kzg355_debug_cell_batch_intermediates(out, *args) if debug else lib().kzg355_verify_cell_kzg_proof_batch_many(*args)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_cell_kzg_proof_batch_many")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_cell") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_cell_kzg_proof_batch_many(groups, s):
        """groups: list of (commitments, cell_indices, cells, proofs), every group the same number of cells; one independent
        verify_cell_kzg_proof_batch per group in one call.  Returns a list of bool / Error."""
        return Kzg._cell_many(groups, s, False)[0]

    @staticmethod
    def debug_cell_batch_intermediates(groups, s):
        """(verdicts as verify_cell_kzg_proof_batch_many, [r (32) | [I(tau)]_1 | LL | RL (48 each) per group])."""
        res, raw = Kzg._cell_many(groups, s, True)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def _cell_many_sets(groups, s, debug):
        flat = [[], [], [], []]
        counts = []
        for grp in groups:
            arrs = Kzg._cell_arrays(*grp)                          # a group whose four lists differ in length: BadArgs, before any FFI call
            counts.append(len(arrs[0]))
            for f, a in zip(flat, arrs):
                f += a
        G = len(counts)
        ok = (C.c_bool * max(G, 1))()
        st = (C.c_int * max(G, 1))()
        cnt = (C.c_size_t * max(G, 1))(*counts)
        idx = (C.c_size_t * max(len(flat[1]), 1))(*flat[1])
        args = (ok, st, cnt, b"".join(flat[0]), idx, b"".join(flat[2]), b"".join(flat[3]), G, s.handle)
        out = C.create_string_buffer(176 * max(G, 1)) if debug else None
        rc = lib().kzg355_debug_cell_batch_intermediates_sets(out, *args) if debug else lib().kzg355_verify_cell_kzg_proof_batch_many_sets(*args)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_cell_kzg_proof_batch_many_sets")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_cell") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_cell_kzg_proof_batch_many_sets(groups, s):
        """verify_cell_kzg_proof_batch_many for groups of any sizes (an empty group is True): list of (commitments, cell_indices, cells, proofs),
        one independent verify_cell_kzg_proof_batch per group, all of them in one set of launches.  Returns a list of bool / Error."""
        return Kzg._cell_many_sets(groups, s, False)[0]

    @staticmethod
    def debug_cell_batch_intermediates_sets(groups, s):
        """(verdicts as verify_cell_kzg_proof_batch_many_sets, [r (32) | [I(tau)]_1 | LL | RL (48 each) per group; zero bytes for an empty group])."""
        res, raw = Kzg._cell_many_sets(groups, s, True)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def debug_cell_setup_monomial(s):
        """The 64 monomial points [tau^t]_1 the handle derived for the cell check, compressed."""
        out = C.create_string_buffer(64 * 48)
        _check(lib().kzg355_debug_cell_setup_monomial(out, s.handle), "debug_cell_setup_monomial")
        return [out.raw[48 * i:48 * i + 48] for i in range(64)]

    # ---- EIP-7594 cells and cell proofs of a blob (compute_cells_and_kzg_proofs; FK20 on the device) ----
    @staticmethod
    def _compute_cells(blobs, s, cells, proofs):
        bl = [_b(x, Blob) for x in blobs]
        n = len(bl)
        c_out, p_out, st = _cell_buffers(cells, proofs, CELLS_PER_EXT_BLOB * n, n)
        rc = lib().kzg355_compute_cells_and_kzg_proofs_many(c_out, p_out, st, b"".join(bl), n, s.handle)
        return _cell_results(rc, st, [CELLS_PER_EXT_BLOB] * n, c_out, p_out, "compute_cells_and_kzg_proofs", "compute_cells")

    @staticmethod
    def _one(res):
        if isinstance(res[0], Error):
            raise res[0]
        return res[0]

    @staticmethod
    def compute_cells(blob, s):
        """The 128 cells of the blob's 2x extension (cells 0..63 are the blob itself); BadArgs on a field element >= r."""
        return Kzg._one(Kzg._compute_cells([blob], s, True, False))[0]

    @staticmethod
    def compute_cells_and_kzg_proofs(blob, s):
        """([Cell] * 128, [KzgProof] * 128) in cell order."""
        return Kzg._one(Kzg._compute_cells([blob], s, True, True))

    @staticmethod
    def compute_kzg_cell_proofs(blob, s):
        """The 128 cell proofs alone (the cells are not computed)."""
        return Kzg._one(Kzg._compute_cells([blob], s, False, True))[1]

    @staticmethod
    def compute_cells_and_kzg_proofs_many(blobs, s):
        """One independent compute_cells_and_kzg_proofs per blob in one call: a list of (cells, proofs) tuples or Error."""
        return Kzg._compute_cells(blobs, s, True, True)

    # ---- EIP-7594 recovery: all cells and proofs of a blob from at least half of its cells (recover_cells_and_kzg_proofs) ----
    @staticmethod
    def _recover(cell_indices, rows, s, cells, proofs):
        ix = [int(i) for i in cell_indices]
        rw = [[_b(x, Cell) for x in row] for row in rows]
        n, m = len(ix), len(rw)
        if any(len(row) != n for row in rw):
            raise BadArgs("length mismatch")
        _, idx = _size_t_arrays(None, ix, "cell index out of range")
        c_out, p_out, st = _cell_buffers(cells, proofs, CELLS_PER_EXT_BLOB * m, m)
        rc = lib().kzg355_recover_cells_and_kzg_proofs_many(c_out, p_out, st, idx, b"".join(b"".join(row) for row in rw), n, m, s.handle)
        return _cell_results(rc, st, [CELLS_PER_EXT_BLOB] * m, c_out, p_out, "recover_cells_and_kzg_proofs", "recover_cells")

    @staticmethod
    def recover_cells_and_kzg_proofs(cell_indices, cells, s):
        """([Cell] * 128, [KzgProof] * 128) of the blob from 64..128 of its cells at the strictly ascending cell_indices; BadArgs on anything else."""
        if len(cell_indices) != len(cells):
            raise BadArgs("length mismatch")
        return Kzg._one(Kzg._recover(cell_indices, [cells], s, True, True))

    @staticmethod
    def recover_cells(cell_indices, cells, s):
        """The 128 cells alone (no proof is computed and no proof setup built)."""
        if len(cell_indices) != len(cells):
            raise BadArgs("length mismatch")
        return Kzg._one(Kzg._recover(cell_indices, [cells], s, True, False))[0]

    @staticmethod
    def recover_cells_and_kzg_proofs_many(cell_indices, rows, s):
        """rows: one list of cells per blob, every blob known at the same cell_indices; one independent recover_cells_and_kzg_proofs per blob in
        one call.  Returns a list of (cells, proofs) tuples or Error."""
        return Kzg._recover(cell_indices, rows, s, True, True)

    @staticmethod
    def _recover_sets(units, s, cells, proofs):
        us = [([int(i) for i in ix], [_b(x, Cell) for x in row]) for ix, row in units]
        m = len(us)
        if any(len(ix) != len(row) for ix, row in us):
            raise BadArgs("length mismatch")
        counts, idx = _size_t_arrays([len(ix) for ix, _ in us], [i for ix, _ in us for i in ix], "cell index out of range")
        c_out, p_out, st = _cell_buffers(cells, proofs, CELLS_PER_EXT_BLOB * m, m)
        rc = lib().kzg355_recover_cells_and_kzg_proofs_many_sets(c_out, p_out, st, counts, idx, b"".join(b"".join(row) for _, row in us), m, s.handle)
        return _cell_results(rc, st, [CELLS_PER_EXT_BLOB] * m, c_out, p_out, "recover_cells_and_kzg_proofs_many_sets", "recover_cells")

    @staticmethod
    def recover_cells_and_kzg_proofs_many_sets(units, s):
        """units: a sequence of (cell_indices, cells), every blob with its own index set (blocks of a node that catches up hold different
        columns); one independent recover_cells_and_kzg_proofs per unit in one call.  Returns a list of (cells, proofs) tuples or Error; a
        unit whose two lengths differ raises BadArgs."""
        return Kzg._recover_sets(units, s, True, True)

    @staticmethod
    def recover_cells_many_sets(units, s):
        """The cells alone, per unit a list of 128 cells or Error (no proof is computed and no proof setup built)."""
        return [r if isinstance(r, Error) else r[0] for r in Kzg._recover_sets(units, s, True, False)]

    # ---- the compute and recover calls with the blobs' commitments: slot 63 of the FK20 convolution whose other slots give the proofs ----
    @staticmethod
    def _commitment_buffer(commitments, cells, proofs, units):
        if not (commitments or cells or proofs):
            raise BadArgs("no output is asked for")
        return C.create_string_buffer(48 * max(units, 1)) if commitments else None

    @staticmethod
    def _compute_commitments_cells(blobs, s, commitments, cells, proofs):
        bl = [_b(x, Blob) for x in blobs]
        n = len(bl)
        k_out = Kzg._commitment_buffer(commitments, cells, proofs, n)
        c_out, p_out, st = _cell_buffers(cells, proofs, CELLS_PER_EXT_BLOB * n, n)
        rc = lib().kzg355_compute_commitments_cells_and_kzg_proofs_many(k_out, c_out, p_out, st, b"".join(bl), n, s.handle)
        return _commitment_cell_results(rc, st, n, k_out, c_out, p_out, "compute_commitment_cells_and_kzg_proofs", "compute_cells")

    @staticmethod
    def compute_commitment_cells_and_kzg_proofs(blob, s):
        """(KzgCommitment, [Cell] * 128, [KzgProof] * 128): compute_cells_and_kzg_proofs and blob_to_kzg_commitment in one call (the chain
        computes the commitment on its way to the proofs; no wide MSM table is built)."""
        return Kzg._one(Kzg._compute_commitments_cells([blob], s, True, True, True))

    @staticmethod
    def compute_commitment_cells_and_kzg_proofs_many(blobs, s):
        """One independent compute_commitment_cells_and_kzg_proofs per blob in one call: a list of (commitment, cells, proofs) tuples or Error."""
        return Kzg._compute_commitments_cells(blobs, s, True, True, True)

    @staticmethod
    def _recover_commitments(cell_indices, rows, s, commitments, cells, proofs):
        ix = [int(i) for i in cell_indices]
        rw = [[_b(x, Cell) for x in row] for row in rows]
        n, m = len(ix), len(rw)
        if any(len(row) != n for row in rw):
            raise BadArgs("length mismatch")
        _, idx = _size_t_arrays(None, ix, "cell index out of range")
        k_out = Kzg._commitment_buffer(commitments, cells, proofs, m)
        c_out, p_out, st = _cell_buffers(cells, proofs, CELLS_PER_EXT_BLOB * m, m)
        rc = lib().kzg355_recover_commitments_cells_and_kzg_proofs_many(k_out, c_out, p_out, st, idx, b"".join(b"".join(row) for row in rw), n, m, s.handle)
        return _commitment_cell_results(rc, st, m, k_out, c_out, p_out, "recover_commitment_cells_and_kzg_proofs", "recover_cells")

    @staticmethod
    def recover_commitment_cells_and_kzg_proofs(cell_indices, cells, s):
        """(KzgCommitment, [Cell] * 128, [KzgProof] * 128) of the blob from 64..128 of its cells: recover_cells_and_kzg_proofs with the
        commitment of the recovered blob, to compare with the block's blob_kzg_commitments (more than 64 cells that lie on no polynomial of
        degree < 4096 are no error; the commitment is then that of the coefficients the algorithm keeps, and differs)."""
        if len(cell_indices) != len(cells):
            raise BadArgs("length mismatch")
        return Kzg._one(Kzg._recover_commitments(cell_indices, [cells], s, True, True, True))

    @staticmethod
    def recover_commitment_cells_and_kzg_proofs_many(cell_indices, rows, s):
        """recover_cells_and_kzg_proofs_many with the commitments: a list of (commitment, cells, proofs) tuples or Error."""
        return Kzg._recover_commitments(cell_indices, rows, s, True, True, True)

    @staticmethod
    def _recover_commitments_sets(units, s, commitments, cells, proofs):
        us = [([int(i) for i in ix], [_b(x, Cell) for x in row]) for ix, row in units]
        m = len(us)
        if any(len(ix) != len(row) for ix, row in us):
            raise BadArgs("length mismatch")
        counts, idx = _size_t_arrays([len(ix) for ix, _ in us], [i for ix, _ in us for i in ix], "cell index out of range")
        k_out = Kzg._commitment_buffer(commitments, cells, proofs, m)
        c_out, p_out, st = _cell_buffers(cells, proofs, CELLS_PER_EXT_BLOB * m, m)
        rc = lib().kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(k_out, c_out, p_out, st, counts, idx,
                                                                             b"".join(b"".join(row) for _, row in us), m, s.handle)
        return _commitment_cell_results(rc, st, m, k_out, c_out, p_out, "recover_commitment_cells_and_kzg_proofs_many_sets", "recover_cells")

    @staticmethod
    def recover_commitment_cells_and_kzg_proofs_many_sets(units, s):
        """recover_cells_and_kzg_proofs_many_sets with the commitments: per unit (commitment, cells, proofs) or Error."""
        return Kzg._recover_commitments_sets(units, s, True, True, True)

    # ---- proofs of chosen EIP-7594 cells of a blob (compute_cell_kzg_proofs_at): every (blob, cell) pair through its own quotient and one MSM ----
    @staticmethod
    def _cells_at(blobs, index_lists, s, cells, proofs):
        bl = [_b(x, Blob) for x in blobs]
        lists = [[int(i) for i in ix] for ix in index_lists]
        n = len(bl)
        if len(lists) != n:
            raise BadArgs("length mismatch")
        slots = [len(ix) for ix in lists]
        counts, idx = _size_t_arrays(slots, [i for ix in lists for i in ix], "cell index out of range")
        c_out, p_out, st = _cell_buffers(cells, proofs, sum(slots), n)
        rc = lib().kzg355_compute_cell_kzg_proofs_at_many(c_out, p_out, st, b"".join(bl), n, counts, idx, s.handle)
        return _cell_results(rc, st, slots, c_out, p_out, "compute_cell_kzg_proofs_at_many", "compute_cell_kzg_proofs_at")

    @staticmethod
    def compute_cell_kzg_proofs_at(blob, cell_indices, s):
        """([Cell], [KzgProof]) of the blob at cell_indices (each < 128, any order, repeats allowed): entry j is what compute_cells_and_kzg_proofs
        returns at index cell_indices[j], at the price of one MSM per index instead of the FK20 chain.  BadArgs on a field element >= r, an
        index >= 128 or more than 128 indices."""
        return Kzg._one(Kzg._cells_at([blob], [cell_indices], s, True, True))

    @staticmethod
    def compute_kzg_cell_proofs_at(blob, cell_indices, s):
        """The proofs alone (the cells are not copied out)."""
        return Kzg._one(Kzg._cells_at([blob], [cell_indices], s, False, True))[1]

    @staticmethod
    def compute_cell_kzg_proofs_at_many(blobs, index_lists, s):
        """One independent compute_cell_kzg_proofs_at per blob, each with its own index list (which may be empty), in one call.  Returns a list
        of (cells, proofs) tuples or Error; blobs and index_lists of different lengths raise BadArgs."""
        return Kzg._cells_at(blobs, index_lists, s, True, True)

    # ---- openings of blobs at chosen points (compute_kzg_proofs_at): every (blob, point) pair through its own quotient and one MSM ----
    @staticmethod
    def compute_kzg_proofs_at_many(blobs, point_lists, s, proofs=True, ys=True):
        """One independent compute_kzg_proofs_at per blob, each with its own list of points (32-byte big-endian field elements; the list may be
        empty), in one call: the blob is handed over once however many openings it gets.  Returns (proofs, ys, statuses): per blob the list of
        its KzgProof and of its Bytes32 y = p(z) in the order of its points -- None for a part that was not asked for (proofs=False runs no
        MSM) and for a blob whose status is not 0 -- and the blobs' status codes.  blobs and point_lists of different lengths raise BadArgs,
        a failure of the whole call raises."""
        bl = [_b(x, Blob) for x in blobs]
        lists = [[_b(z, Bytes32) for z in zs] for zs in point_lists]
        n = len(bl)
        if len(lists) != n:
            raise BadArgs("length mismatch")
        if not proofs and not ys:
            raise BadArgs("proofs and ys are both declined")
        slots = [len(zs) for zs in lists]
        counts, total = (C.c_size_t * max(n, 1))(*slots), sum(slots)
        p_out = C.create_string_buffer(48 * max(total, 1)) if proofs else None
        y_out = C.create_string_buffer(32 * max(total, 1)) if ys else None
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_kzg_proofs_at_many(p_out, y_out, st, b"".join(bl), n, counts, b"".join(z for zs in lists for z in zs), s.handle)
        if _whole_call_failed(rc, st, n):
            _check(rc, "compute_kzg_proofs_at_many")
        praw, yraw = (None if b is None else b.raw for b in (p_out, y_out))
        res_p, res_y, off = [], [], 0
        for i, k in enumerate(slots):
            good = st[i] == 0
            res_p.append([KzgProof(praw[48 * j:48 * (j + 1)]) for j in range(off, off + k)] if good and praw is not None else None)
            res_y.append([Bytes32(yraw[32 * j:32 * (j + 1)]) for j in range(off, off + k)] if good and yraw is not None else None)
            off += k
        return res_p, res_y, [st[i] for i in range(n)]

    @staticmethod
    def compute_kzg_proofs_at(blob, zs, s, proofs=True):
        """([KzgProof], [Bytes32]) of the blob opened at the points zs (any order, repeats allowed, inside the domain or not; at most 4096):
        entry j is what compute_kzg_proof returns for (blob, zs[j]).  proofs=False returns (None, ys) and runs no MSM.  BadArgs on a field
        element >= r, a point >= r or more than 4096 points."""
        res_p, res_y, st = Kzg.compute_kzg_proofs_at_many([blob], [zs], s, proofs=proofs)
        if st[0] != 0:
            raise _ERRORS.get(st[0], InternalError)("compute_kzg_proofs_at")
        return res_p[0], res_y[0]

    # ---- chosen cells of recovered blobs (recover_cells_and_kzg_proofs_at): the recovery of recover_cells_and_kzg_proofs, then every wanted
    # (blob, cell) pair through its own quotient and one MSM ----
    @staticmethod
    def _recover_at(units, s, cells, proofs):
        us = [([int(i) for i in ix], [_b(x, Cell) for x in row], [int(i) for i in want]) for ix, row, want in units]
        m = len(us)
        if any(len(ix) != len(row) for ix, row, _ in us):
            raise BadArgs("length mismatch")
        slots = [len(want) for _, _, want in us]
        kcounts, kidx = _size_t_arrays([len(ix) for ix, _, _ in us], [i for ix, _, _ in us for i in ix], "cell index out of range")
        wcounts, widx = _size_t_arrays(slots, [i for _, _, want in us for i in want], "cell index out of range")
        c_out, p_out, st = _cell_buffers(cells, proofs, sum(slots), m)
        rc = lib().kzg355_recover_cells_and_kzg_proofs_at_many_sets(c_out, p_out, st, kcounts, kidx, b"".join(b"".join(row) for _, row, _ in us),
                                                                    wcounts, widx, m, s.handle)
        return _cell_results(rc, st, slots, c_out, p_out, "recover_cells_and_kzg_proofs_at_many_sets", "recover_cells_and_kzg_proofs_at")

    @staticmethod
    def recover_cells_and_kzg_proofs_at(cell_indices, cells, want_indices, s):
        """([Cell], [KzgProof]) at want_indices (each < 128, any order, repeats allowed) of the blob known at cell_indices (64..128 strictly
        ascending indices, cells in the same order): entry j is what recover_cells_and_kzg_proofs returns at index want_indices[j] for the
        same input, at the price of one MSM per wanted index instead of the FK20 chain.  BadArgs on what that call refuses, on a wanted
        index >= 128 and on more than 128 of them."""
        return Kzg._one(Kzg._recover_at([(cell_indices, cells, want_indices)], s, True, True))

    @staticmethod
    def recover_cells_and_kzg_proofs_at_many_sets(units, s):
        """units: a sequence of (cell_indices, cells, want_indices), every blob with its own two lists (want_indices may be empty: the blob
        is still recovered and checked); one independent recover_cells_and_kzg_proofs_at per unit in one call.  Returns a list of
        (cells, proofs) tuples or Error; a unit whose first two lengths differ raises BadArgs."""
        return Kzg._recover_at(units, s, True, True)

    @staticmethod
    def recover_missing_cells_and_kzg_proofs(cell_indices, cells, s):
        """(missing_indices, [Cell], [KzgProof]): the cells and proofs of the blob at the indices below 128 that are not among cell_indices,
        ascending -- what a node that lacks a few columns needs; the proofs of the known cells arrived with them."""
        known = {int(i) for i in cell_indices}
        missing = [i for i in range(CELLS_PER_EXT_BLOB) if i not in known]
        c, p = Kzg.recover_cells_and_kzg_proofs_at(cell_indices, cells, missing, s)
        return missing, c, p

    @staticmethod
    def debug_cell_compute_h(blobs, s):
        """FK20 intermediates per blob: H_0 .. H_63 compressed (H_63 is the point at infinity), or Error."""
        bl = [_b(x, Blob) for x in blobs]
        n = len(bl)
        out = C.create_string_buffer(64 * 48 * max(n, 1))
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_debug_cell_compute_h(out, st, b"".join(bl), n, s.handle)
        if _whole_call_failed(rc, st, n):
            _check(rc, "debug_cell_compute_h")
        raw = out.raw
        return [[raw[48 * (64 * i + e):48 * (64 * i + e + 1)] for e in range(64)] if st[i] == 0 else _ERRORS.get(st[i], InternalError)("h")
                for i in range(n)]

    @staticmethod
    def debug_cell_setup_monomial_all(s):
        """The 4096 monomial points [tau^t]_1 the handle derived for compute_cells_and_kzg_proofs, compressed."""
        out = C.create_string_buffer(4096 * 48)
        _check(lib().kzg355_debug_cell_setup_monomial_all(out, s.handle), "debug_cell_setup_monomial_all")
        return [out.raw[48 * i:48 * i + 48] for i in range(4096)]

    # ---- the three cell calls on device-resident data.  A device argument is an object with data_ptr() (a torch uint8 / int64 tensor on the
    # handle's device) or a plain integer address; sizes and dtypes are checked where the object offers them, before any FFI call ----
    @staticmethod
    def _dev(x, what, numel, dtype="uint8", optional=False):
        if x is None:
            if optional:
                return None
            raise BadArgs(f"{what}: missing")
        if isinstance(x, int):
            return x
        if not hasattr(x, "data_ptr"):
            raise BadArgs(f"{what}: neither an address nor an object with data_ptr()")
        if hasattr(x, "dtype") and str(x.dtype).rsplit(".", 1)[-1] != dtype:
            raise BadArgs(f"{what}: dtype {x.dtype}, expected {dtype}")
        if hasattr(x, "numel") and x.numel() != numel:
            raise BadArgs(f"{what}: {x.numel()} elements, expected {numel}")
        if hasattr(x, "is_contiguous") and not x.is_contiguous():
            raise BadArgs(f"{what}: not contiguous")
        return x.data_ptr()

    @staticmethod
    def _cell_many_device(commitments, cell_indices, cells, proofs, n_per_group, groups, s, prep_form, debug):
        npg, G = int(n_per_group), int(groups)
        if npg < 0 or G < 0 or prep_form not in (0, 1, 2):
            raise BadArgs("n_per_group, groups or prep_form out of range")
        N = npg * G
        ptrs = (Kzg._dev(commitments, "commitments", 48 * N, optional=N == 0), Kzg._dev(cell_indices, "cell_indices", N, "int64", optional=N == 0),
                Kzg._dev(cells, "cells", BYTES_PER_CELL * N, optional=N == 0), Kzg._dev(proofs, "proofs", 48 * N, optional=N == 0))
        if G == 0:
            return [], b""
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        if debug:
            out = C.create_string_buffer(176 * G)
            rc = lib().kzg355_debug_cell_batch_intermediates_device(out, ok, st, *ptrs, npg, G, prep_form, s.handle)
        else:
            if prep_form != 0:
                raise BadArgs("prep_form is pinned through debug_cell_batch_intermediates_device only")
            rc = lib().kzg355_verify_cell_kzg_proof_batch_many_device(ok, st, *ptrs, npg, G, s.handle)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_cell_kzg_proof_batch_many_device")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_cell") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_cell_kzg_proof_batch_many_device(commitments, cell_indices, cells, proofs, n_per_group, groups, s):
        """verify_cell_kzg_proof_batch_many on device memory: commitments (groups * n_per_group * 48 bytes, uint8), cell_indices (int64), cells
        (* 2048) and proofs (* 48), group-major.  Returns a list of bool / Error, one per group, as the host form does."""
        return Kzg._cell_many_device(commitments, cell_indices, cells, proofs, n_per_group, groups, s, 0, False)[0]

    @staticmethod
    def debug_cell_batch_intermediates_device(commitments, cell_indices, cells, proofs, n_per_group, groups, s, prep_form=0):
        """(verdicts, [176 bytes per group]) as debug_cell_batch_intermediates; prep_form 0 by shape, 1 device preparation, 2 host preparation."""
        res, raw = Kzg._cell_many_device(commitments, cell_indices, cells, proofs, n_per_group, groups, s, prep_form, True)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def _cell_many_sets_device(commitments, cell_indices, cells, proofs, cell_counts, s, prep_form, debug):
        counts = [int(c) for c in cell_counts]
        if any(c < 0 or c >= 1 << 64 for c in counts) or prep_form not in (0, 1, 2):
            raise BadArgs("cell_counts or prep_form out of range")
        N, G = sum(counts), len(counts)
        ptrs = (Kzg._dev(commitments, "commitments", 48 * N, optional=N == 0), Kzg._dev(cell_indices, "cell_indices", N, "int64", optional=N == 0),
                Kzg._dev(cells, "cells", BYTES_PER_CELL * N, optional=N == 0), Kzg._dev(proofs, "proofs", 48 * N, optional=N == 0))
        if G == 0:
            return [], b""
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        cnt = (C.c_size_t * G)(*counts)
        if debug:
            out = C.create_string_buffer(176 * G)
            rc = lib().kzg355_debug_cell_batch_intermediates_sets_device(out, ok, st, cnt, *ptrs, G, prep_form, s.handle)
        else:
            rc = lib().kzg355_verify_cell_kzg_proof_batch_many_sets_device(ok, st, cnt, *ptrs, G, s.handle)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_cell_kzg_proof_batch_many_sets_device")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_cell") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_cell_kzg_proof_batch_many_sets_device(commitments, cell_indices, cells, proofs, cell_counts, s):
        """verify_cell_kzg_proof_batch_many_sets on device memory: commitments (sum(cell_counts) * 48 bytes, uint8), cell_indices (int64), cells
        (* 2048) and proofs (* 48), group after group with no padding; cell_counts is a host list.  Returns a list of bool / Error per group."""
        return Kzg._cell_many_sets_device(commitments, cell_indices, cells, proofs, cell_counts, s, 0, False)[0]

    @staticmethod
    def debug_cell_batch_intermediates_sets_device(commitments, cell_indices, cells, proofs, cell_counts, s, prep_form=0):
        """(verdicts, [176 bytes per group; zero bytes for an empty group]) as debug_cell_batch_intermediates_sets; prep_form 0 by shape, 1 device
        preparation, 2 host preparation."""
        res, raw = Kzg._cell_many_sets_device(commitments, cell_indices, cells, proofs, cell_counts, s, prep_form, True)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def _cell_outputs(cells_out, proofs_out, slots):
        if cells_out is None and proofs_out is None:
            raise BadArgs("cells_out and proofs_out are both missing")
        return Kzg._dev(cells_out, "cells_out", BYTES_PER_CELL * slots, optional=True), Kzg._dev(proofs_out, "proofs_out", 48 * slots, optional=True)

    @staticmethod
    def compute_cells_and_kzg_proofs_many_device(blobs, n, s, cells_out=None, proofs_out=None):
        """compute_cells_and_kzg_proofs of n resident blobs (n * 131072 bytes) into the caller's device tensors cells_out (n * 128 * 2048 bytes)
        and proofs_out (n * 128 * 48); either may be None, not both.  Returns one entry per blob: None, or the Error of that blob (its output
        slots are then unspecified)."""
        n = int(n)
        if n < 0:
            raise BadArgs("n out of range")
        c_out, p_out = Kzg._cell_outputs(cells_out, proofs_out, CELLS_PER_EXT_BLOB * n)
        d_blobs = Kzg._dev(blobs, "blobs", 4096 * 32 * n, optional=n == 0)
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_cells_and_kzg_proofs_many_device(c_out, p_out, st, d_blobs, n, s.handle)
        return _device_results(rc, st, n, "compute_cells_and_kzg_proofs_many_device", "compute_cells")

    @staticmethod
    def recover_cells_and_kzg_proofs_many_device(cell_indices, cells, m, s, cells_out=None, proofs_out=None):
        """recover_cells_and_kzg_proofs of m resident blobs known at the same cell_indices (a host sequence of 64..128 strictly ascending
        indices): cells holds m * len(cell_indices) * 2048 bytes, blob after blob.  Outputs and return value as
        compute_cells_and_kzg_proofs_many_device."""
        cell_indices = list(cell_indices)
        n, m = len(cell_indices), int(m)
        if m < 0:
            raise BadArgs("m or a cell index out of range")
        _, idx = _size_t_arrays(None, cell_indices, "m or a cell index out of range")
        c_out, p_out = Kzg._cell_outputs(cells_out, proofs_out, CELLS_PER_EXT_BLOB * m)
        d_cells = Kzg._dev(cells, "cells", BYTES_PER_CELL * n * m, optional=m == 0)
        st = (C.c_int * max(m, 1))()
        rc = lib().kzg355_recover_cells_and_kzg_proofs_many_device(c_out, p_out, st, idx, d_cells, n, m, s.handle)
        return _device_results(rc, st, m, "recover_cells_and_kzg_proofs_many_device", "recover_cells")

    @staticmethod
    def recover_cells_and_kzg_proofs_many_sets_device(cell_counts, cell_indices, cells, s, cells_out=None, proofs_out=None):
        """recover_cells_and_kzg_proofs_many_sets of resident blobs: blob i is known at cell_counts[i] cells, its indices following those of
        blob i - 1 in cell_indices (both host sequences) and its cells those of blob i - 1 in cells (sum of the counts * 2048 bytes on the
        device).  Outputs and return value as compute_cells_and_kzg_proofs_many_device."""
        cell_counts, cell_indices = list(cell_counts), list(cell_indices)
        counts, idx = _size_t_arrays(cell_counts, cell_indices, "a count or a cell index out of range, or the counts do not add up to the indices")
        m = len(cell_counts)
        c_out, p_out = Kzg._cell_outputs(cells_out, proofs_out, CELLS_PER_EXT_BLOB * m)
        d_cells = Kzg._dev(cells, "cells", BYTES_PER_CELL * len(cell_indices), optional=m == 0)
        st = (C.c_int * max(m, 1))()
        rc = lib().kzg355_recover_cells_and_kzg_proofs_many_sets_device(c_out, p_out, st, counts, idx, d_cells, m, s.handle)
        return _device_results(rc, st, m, "recover_cells_and_kzg_proofs_many_sets_device", "recover_cells")

    @staticmethod
    def _commitment_cell_outputs(commitments_out, cells_out, proofs_out, units):
        if commitments_out is None and cells_out is None and proofs_out is None:
            raise BadArgs("commitments_out, cells_out and proofs_out are all missing")
        return (Kzg._dev(commitments_out, "commitments_out", 48 * units, optional=True),
                Kzg._dev(cells_out, "cells_out", BYTES_PER_CELL * CELLS_PER_EXT_BLOB * units, optional=True),
                Kzg._dev(proofs_out, "proofs_out", 48 * CELLS_PER_EXT_BLOB * units, optional=True))

    @staticmethod
    def compute_commitment_cells_and_kzg_proofs_many_device(blobs, n, s, commitments_out=None, cells_out=None, proofs_out=None):
        """compute_cells_and_kzg_proofs_many_device with the blobs' commitments written into the device tensor commitments_out (n * 48 bytes) as
        well; any of the three outputs may be None, not all.  Returns one entry per blob: None, or the Error of that blob."""
        n = int(n)
        if n < 0:
            raise BadArgs("n out of range")
        k_out, c_out, p_out = Kzg._commitment_cell_outputs(commitments_out, cells_out, proofs_out, n)
        d_blobs = Kzg._dev(blobs, "blobs", 4096 * 32 * n, optional=n == 0)
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_commitments_cells_and_kzg_proofs_many_device(k_out, c_out, p_out, st, d_blobs, n, s.handle)
        return _device_results(rc, st, n, "compute_commitment_cells_and_kzg_proofs_many_device", "compute_cells")

    @staticmethod
    def recover_commitment_cells_and_kzg_proofs_many_device(cell_indices, cells, m, s, commitments_out=None, cells_out=None, proofs_out=None):
        """recover_cells_and_kzg_proofs_many_device with the commitments of the recovered blobs in commitments_out (m * 48 bytes) as well."""
        cell_indices = list(cell_indices)
        n, m = len(cell_indices), int(m)
        if m < 0:
            raise BadArgs("m or a cell index out of range")
        _, idx = _size_t_arrays(None, cell_indices, "m or a cell index out of range")
        k_out, c_out, p_out = Kzg._commitment_cell_outputs(commitments_out, cells_out, proofs_out, m)
        d_cells = Kzg._dev(cells, "cells", BYTES_PER_CELL * n * m, optional=m == 0)
        st = (C.c_int * max(m, 1))()
        rc = lib().kzg355_recover_commitments_cells_and_kzg_proofs_many_device(k_out, c_out, p_out, st, idx, d_cells, n, m, s.handle)
        return _device_results(rc, st, m, "recover_commitment_cells_and_kzg_proofs_many_device", "recover_cells")

    @staticmethod
    def recover_commitment_cells_and_kzg_proofs_many_sets_device(cell_counts, cell_indices, cells, s, commitments_out=None, cells_out=None,
                                                                 proofs_out=None):
        """recover_cells_and_kzg_proofs_many_sets_device with the commitments of the recovered blobs in commitments_out (48 bytes per blob) as
        well."""
        cell_counts, cell_indices = list(cell_counts), list(cell_indices)
        counts, idx = _size_t_arrays(cell_counts, cell_indices, "a count or a cell index out of range, or the counts do not add up to the indices")
        m = len(cell_counts)
        k_out, c_out, p_out = Kzg._commitment_cell_outputs(commitments_out, cells_out, proofs_out, m)
        d_cells = Kzg._dev(cells, "cells", BYTES_PER_CELL * len(cell_indices), optional=m == 0)
        st = (C.c_int * max(m, 1))()
        rc = lib().kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(k_out, c_out, p_out, st, counts, idx, d_cells, m, s.handle)
        return _device_results(rc, st, m, "recover_commitment_cells_and_kzg_proofs_many_sets_device", "recover_cells")

    @staticmethod
    def compute_cell_kzg_proofs_at_many_device(blobs, n, cell_counts, cell_indices, s, cells_out=None, proofs_out=None):
        """compute_cell_kzg_proofs_at_many of n resident blobs (n * 131072 bytes): blob i asks for cell_counts[i] cells, its indices following
        those of blob i - 1 in cell_indices (both host sequences).  Slot j of the device tensors cells_out (sum of the counts * 2048 bytes) and
        proofs_out (* 48) receives the cell and proof of entry j of cell_indices; either may be None, not both.  Returns one entry per blob:
        None, or the Error of that blob (its output slots are then unspecified)."""
        cell_counts, cell_indices = list(cell_counts), list(cell_indices)
        n, message = int(n), "n, a count or a cell index out of range, or the counts do not add up to the indices"
        if n < 0 or len(cell_counts) != n:
            raise BadArgs(message)
        counts, idx = _size_t_arrays(cell_counts, cell_indices, message)
        c_out, p_out = Kzg._cell_outputs(cells_out, proofs_out, len(cell_indices))
        d_blobs = Kzg._dev(blobs, "blobs", 4096 * 32 * n, optional=n == 0)
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_cell_kzg_proofs_at_many_device(c_out, p_out, st, d_blobs, n, counts, idx, s.handle)
        return _device_results(rc, st, n, "compute_cell_kzg_proofs_at_many_device", "compute_cell_kzg_proofs_at")

    @staticmethod
    def compute_kzg_proofs_at_many_device(blobs, n, point_counts, zs, s, proofs_out=None, ys_out=None):
        """compute_kzg_proofs_at_many of n resident blobs (n * 131072 bytes): blob i is opened at point_counts[i] points, which follow those of
        blob i - 1 in zs (host: a sequence of 32-byte points, or their bytes joined).  Slot j of the device tensors proofs_out (sum of the
        counts * 48 bytes) and ys_out (* 32) receives the proof and y of point j of zs; either may be None, not both.  Returns one entry per
        blob: None, or the Error of that blob (its output slots are then unspecified)."""
        point_counts = [int(c) for c in point_counts]
        zz = bytes(zs) if isinstance(zs, (bytes, bytearray)) else b"".join(_b(z, Bytes32) for z in zs)
        n, message = int(n), "n or a count out of range, or the counts do not add up to the points"
        if n < 0 or len(point_counts) != n or any(c < 0 or c >= 1 << 64 for c in point_counts) or 32 * sum(point_counts) != len(zz):
            raise BadArgs(message)
        if proofs_out is None and ys_out is None:
            raise BadArgs("proofs_out and ys_out are both missing")
        total = sum(point_counts)
        p_out = Kzg._dev(proofs_out, "proofs_out", 48 * total, optional=True)
        y_out = Kzg._dev(ys_out, "ys_out", 32 * total, optional=True)
        d_blobs = Kzg._dev(blobs, "blobs", 4096 * 32 * n, optional=n == 0)
        st = (C.c_int * max(n, 1))()
        rc = lib().kzg355_compute_kzg_proofs_at_many_device(p_out, y_out, st, d_blobs, n, (C.c_size_t * max(n, 1))(*point_counts), zz, s.handle)
        return _device_results(rc, st, n, "compute_kzg_proofs_at_many_device", "compute_kzg_proofs_at")

    @staticmethod
    def recover_cells_and_kzg_proofs_at_many_sets_device(cell_counts, cell_indices, cells, want_counts, want_indices, s, cells_out=None, proofs_out=None):
        """recover_cells_and_kzg_proofs_at_many_sets of resident blobs: blob i is known at cell_counts[i] cells, its indices following those of
        blob i - 1 in cell_indices and its cells those of blob i - 1 in cells (sum of the cell counts * 2048 bytes on the device), and asks for
        want_counts[i] cells, its wanted indices following those of blob i - 1 in want_indices (the four lists are host sequences).  Slot j of
        the device tensors cells_out (sum of the want counts * 2048 bytes) and proofs_out (* 48) receives the cell and proof of entry j of
        want_indices; either may be None, not both.  Returns one entry per blob: None, or the Error of that blob (its output slots are then
        unspecified)."""
        cell_counts, cell_indices, want_counts, want_indices = list(cell_counts), list(cell_indices), list(want_counts), list(want_indices)
        m, message = len(cell_counts), "a count or a cell index out of range, or the counts do not add up to the indices"
        if len(want_counts) != m:
            raise BadArgs(message)
        kcounts, kidx = _size_t_arrays(cell_counts, cell_indices, message)
        wcounts, widx = _size_t_arrays(want_counts, want_indices, message)
        c_out, p_out = Kzg._cell_outputs(cells_out, proofs_out, len(want_indices))
        d_cells = Kzg._dev(cells, "cells", BYTES_PER_CELL * len(cell_indices), optional=m == 0)
        st = (C.c_int * max(m, 1))()
        rc = lib().kzg355_recover_cells_and_kzg_proofs_at_many_sets_device(c_out, p_out, st, kcounts, kidx, d_cells, wcounts, widx, m, s.handle)
        return _device_results(rc, st, m, "recover_cells_and_kzg_proofs_at_many_sets_device", "recover_cells_and_kzg_proofs_at")

    # ---- blobs against their EIP-7594 cell proofs (what a Fulu blob transaction or blobs bundle carries): verify_cell_kzg_proof_batch over all
    # 128 cells of every blob, the cells computed on the device ----
    @staticmethod
    def verify_blob_cell_proofs_batch(blobs, commitments, cell_proofs, s):
        """One blob transaction: its blobs, their commitments and 128 cell proofs per blob (blob after blob, cell order); True / False, BadArgs
        on bad input or when the three lengths do not fit."""
        bl = [_b(x, Blob) for x in blobs]
        cs = [_b(x, KzgCommitment) for x in commitments]
        ps = [_b(x, KzgProof) for x in cell_proofs]
        ok = C.c_bool()
        _check(lib().kzg355_verify_blob_cell_proofs_batch(C.byref(ok), b"".join(bl), len(bl), b"".join(cs), len(cs), b"".join(ps), len(ps), s.handle),
               "verify_blob_cell_proofs_batch")
        return bool(ok.value)

    @staticmethod
    def _blob_cells_many(groups, s, debug, interp_form=0):
        if not groups:
            return [], b""
        if interp_form not in (0, 1, 2):
            raise BadArgs("interp_form out of range")
        n = len(groups[0][0])
        flat = [[], [], []]
        for blobs, commitments, cell_proofs in groups:
            arrs = ([_b(x, Blob) for x in blobs], [_b(x, KzgCommitment) for x in commitments], [_b(x, KzgProof) for x in cell_proofs])
            if len(arrs[0]) != n:
                raise BadArgs("all groups must have the same number of blobs")
            if len(arrs[1]) != n or len(arrs[2]) != CELLS_PER_EXT_BLOB * n:
                raise BadArgs("length mismatch")
            for f, a in zip(flat, arrs):
                f += a
        G = len(groups)
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        args = (ok, st, b"".join(flat[0]), b"".join(flat[1]), b"".join(flat[2]), n, G)
        out = C.create_string_buffer(176 * G) if debug else None
        rc = (lib().kzg355_debug_blob_cell_batch_intermediates(out, *args, interp_form, s.handle) if debug
              else lib().kzg355_verify_blob_cell_proofs_batch_many(*args, s.handle))
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_blob_cell_proofs_batch_many")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_blob_cells") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_blob_cell_proofs_batch_many(groups, s):
        """groups: list of (blobs, commitments, cell_proofs), every group the same number of blobs; one independent
        verify_blob_cell_proofs_batch per group in one call.  Returns a list of bool / Error."""
        return Kzg._blob_cells_many(groups, s, False)[0]

    @staticmethod
    def debug_blob_cell_batch_intermediates(groups, s, interp_form=0):
        """(verdicts as verify_blob_cell_proofs_batch_many, [r (32) | [I(tau)]_1 | LL | RL (48 each) per group]); interp_form 0 what the call
        does, 1 the interpolation from the blobs' coefficients, 2 the column kernel over the computed cells."""
        res, raw = Kzg._blob_cells_many(groups, s, True, interp_form)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def _blob_cells_many_device(blobs, commitments, cell_proofs, n_per_group, groups, s, interp_form, prep_form, debug):
        n, G = int(n_per_group), int(groups)
        if n < 0 or G < 0 or interp_form not in (0, 1, 2) or prep_form not in (0, 1, 2):
            raise BadArgs("n_per_group, groups, interp_form or prep_form out of range")
        nb = n * G
        ptrs = (Kzg._dev(blobs, "blobs", BYTES_PER_BLOB * nb, optional=nb == 0), Kzg._dev(commitments, "commitments", 48 * nb, optional=nb == 0),
                Kzg._dev(cell_proofs, "cell_proofs", 48 * CELLS_PER_EXT_BLOB * nb, optional=nb == 0))
        if G == 0:
            return [], b""
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        if debug:
            out = C.create_string_buffer(176 * G)
            rc = lib().kzg355_debug_blob_cell_batch_intermediates_device(out, ok, st, *ptrs, n, G, interp_form, prep_form, s.handle)
        else:
            rc = lib().kzg355_verify_blob_cell_proofs_batch_many_device(ok, st, *ptrs, n, G, s.handle)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_blob_cell_proofs_batch_many_device")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_blob_cells") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_blob_cell_proofs_batch_many_device(blobs, commitments, cell_proofs, n_per_group, groups, s):
        """verify_blob_cell_proofs_batch_many on device memory: blobs (groups * n_per_group * 131072 bytes, uint8), commitments (* 48) and
        cell_proofs (* 128 * 48), group-major.  Returns a list of bool / Error, one per group, as the host form does."""
        return Kzg._blob_cells_many_device(blobs, commitments, cell_proofs, n_per_group, groups, s, 0, 0, False)[0]

    @staticmethod
    def debug_blob_cell_batch_intermediates_device(blobs, commitments, cell_proofs, n_per_group, groups, s, interp_form=0, prep_form=0):
        """(verdicts, [176 bytes per group]) as debug_blob_cell_batch_intermediates; prep_form 0 by shape, 1 transcripts hashed on the device,
        2 on the host."""
        res, raw = Kzg._blob_cells_many_device(blobs, commitments, cell_proofs, n_per_group, groups, s, interp_form, prep_form, True)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def _blob_cells_many_sets(groups, s, debug, interp_form=0):
        if interp_form not in (0, 1, 2):
            raise BadArgs("interp_form out of range")
        flat = [[], [], []]
        counts = []
        for blobs, commitments, cell_proofs in groups:
            arrs = ([_b(x, Blob) for x in blobs], [_b(x, KzgCommitment) for x in commitments], [_b(x, KzgProof) for x in cell_proofs])
            n = len(arrs[0])
            if len(arrs[1]) != n or len(arrs[2]) != CELLS_PER_EXT_BLOB * n:        # a group that does not fit: BadArgs, before any FFI call
                raise BadArgs("length mismatch")
            counts.append(n)
            for f, a in zip(flat, arrs):
                f += a
        G = len(counts)
        ok = (C.c_bool * max(G, 1))()
        st = (C.c_int * max(G, 1))()
        cnt = (C.c_size_t * max(G, 1))(*counts)
        args = (ok, st, cnt, b"".join(flat[0]), b"".join(flat[1]), b"".join(flat[2]), G)
        out = C.create_string_buffer(176 * max(G, 1)) if debug else None
        rc = (lib().kzg355_debug_blob_cell_batch_intermediates_sets(out, *args, interp_form, s.handle) if debug
              else lib().kzg355_verify_blob_cell_proofs_batch_many_sets(*args, s.handle))
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_blob_cell_proofs_batch_many_sets")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_blob_cells") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_blob_cell_proofs_batch_many_sets(groups, s):
        """verify_blob_cell_proofs_batch_many for groups of any blob counts (an empty group is True): list of (blobs, commitments, cell_proofs),
        one independent verify_blob_cell_proofs_batch per group, all of them in one set of launches.  Returns a list of bool / Error."""
        return Kzg._blob_cells_many_sets(groups, s, False)[0]

    @staticmethod
    def debug_blob_cell_batch_intermediates_sets(groups, s, interp_form=0):
        """(verdicts as verify_blob_cell_proofs_batch_many_sets, [r (32) | [I(tau)]_1 | LL | RL (48 each) per group; zero bytes for an empty
        group]); interp_form as in debug_blob_cell_batch_intermediates, 0 chosen per set of launches."""
        res, raw = Kzg._blob_cells_many_sets(groups, s, True, interp_form)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]

    @staticmethod
    def _blob_cells_many_sets_device(blobs, commitments, cell_proofs, blob_counts, s, interp_form, prep_form, debug):
        counts = [int(c) for c in blob_counts]
        if any(c < 0 for c in counts) or interp_form not in (0, 1, 2) or prep_form not in (0, 1, 2):
            raise BadArgs("blob_counts, interp_form or prep_form out of range")
        nb, G = sum(counts), len(counts)
        ptrs = (Kzg._dev(blobs, "blobs", BYTES_PER_BLOB * nb, optional=nb == 0), Kzg._dev(commitments, "commitments", 48 * nb, optional=nb == 0),
                Kzg._dev(cell_proofs, "cell_proofs", 48 * CELLS_PER_EXT_BLOB * nb, optional=nb == 0))
        if G == 0:
            return [], b""
        ok = (C.c_bool * G)()
        st = (C.c_int * G)()
        cnt = (C.c_size_t * G)(*counts)
        if debug:
            out = C.create_string_buffer(176 * G)
            rc = lib().kzg355_debug_blob_cell_batch_intermediates_sets_device(out, ok, st, cnt, *ptrs, G, interp_form, prep_form, s.handle)
        else:
            rc = lib().kzg355_verify_blob_cell_proofs_batch_many_sets_device(ok, st, cnt, *ptrs, G, s.handle)
        if _whole_call_failed(rc, st, G):
            _check(rc, "verify_blob_cell_proofs_batch_many_sets_device")
        res = [bool(ok[i]) if st[i] == 0 else _ERRORS.get(st[i], InternalError)("verify_blob_cells") for i in range(G)]
        return res, (out.raw if debug else b"")

    @staticmethod
    def verify_blob_cell_proofs_batch_many_sets_device(blobs, commitments, cell_proofs, blob_counts, s):
        """verify_blob_cell_proofs_batch_many_sets on device memory: blobs (sum(blob_counts) * 131072 bytes, uint8), commitments (* 48) and
        cell_proofs (* 128 * 48), group after group with no padding; blob_counts is a host list.  Returns a list of bool / Error per group."""
        return Kzg._blob_cells_many_sets_device(blobs, commitments, cell_proofs, blob_counts, s, 0, 0, False)[0]

    @staticmethod
    def debug_blob_cell_batch_intermediates_sets_device(blobs, commitments, cell_proofs, blob_counts, s, interp_form=0, prep_form=0):
        """(verdicts, [176 bytes per group]) as debug_blob_cell_batch_intermediates_sets; prep_form 0 by shape, 1 transcripts hashed on the
        device, 2 on the host."""
        res, raw = Kzg._blob_cells_many_sets_device(blobs, commitments, cell_proofs, blob_counts, s, interp_form, prep_form, True)
        return res, [raw[176 * i:176 * i + 176] for i in range(len(res))]
