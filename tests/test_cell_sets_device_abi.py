"""-m "not gpu": verify_cell_kzg_proof_batch_many_sets_device (groups of different sizes on device-resident data) at the boundary.
include/kzg355.h declares the call and its debug form with their argument names, the built library exports them, the ctypes loader binds them,
the Rust shim, the C++ mirror and INTEGRATION.md name them, a NULL handle refuses the whole call and marks every status, the Python wrapper
refuses tensors that do not fit the counts before any FFI call, and the ragged entry of k_cell_prep.hip uses no scratch, no dynamic stack and
the LDS of its uniform twin."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY, DEBUG = "kzg355_verify_cell_kzg_proof_batch_many_sets_device", "kzg355_debug_cell_batch_intermediates_sets_device"
BADARGS = 1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    names = lambda m: [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]      # noqa: E731
    args = ["ok", "status", "cell_counts", "d_commitments", "d_cell_indices", "d_cells", "d_proofs", "groups"]
    for fn, want in ((VERIFY, args + ["s"]), (DEBUG, ["out"] + args + ["prep_form", "s"])):
        m = re.search(r"int\s+" + fn + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and names(m) == want, fn


def test_header_states_the_contract_where_a_reader_looks_for_it():
    hdr = read("include", "kzg355.h")
    flow = lambda text: re.sub(r"\s*\n \* ?", " ", text)                                # noqa: E731  (the comment as running text)
    comment = flow(hdr[:hdr.index("int " + VERIFY + "(")].rsplit("/*", 1)[1])
    for phrase in ("16-byte", "8-byte aligned", "HOST pointers", "first device", "before any device is touched", "largest group", "16384 cells",
                   "uniform shapes only", "kzg355_settings_cell_calls_per_device", "never cut"):
        assert phrase in comment, phrase
    # the host form's comment points here and no longer says that this is missing
    host = flow(hdr[:hdr.index("int kzg355_verify_cell_kzg_proof_batch_many_sets(")].rsplit("/*", 1)[1])
    assert VERIFY in host and "built on one n per call" not in host
    assert "Not offered: cutting a group of this call over several devices" in host


def test_library_exports_them_and_the_loader_binds_them():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    for n, argc in ((VERIFY, 9), (DEBUG, 11)):
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc


def test_mirrors_name_them():
    ffi = read("rust", "src", "ffi.rs")
    for n in (VERIFY, DEBUG):
        assert re.search(r"pub fn " + n + r"\s*\(", ffi), n
    rust = read("rust", "src", "kzg.rs")
    assert "pub unsafe fn verify_cell_kzg_proof_batch_many_sets_device(" in rust and "ffi::" + VERIFY + "(" in rust
    hpp = read("include", "kzg355.hpp")
    assert VERIFY + "(" in hpp and "verify_cell_kzg_proof_batch_many_sets_device(const" in hpp.replace(VERIFY, "")
    doc = read("INTEGRATION.md")
    assert VERIFY in doc and DEBUG in doc and "Kzg.verify_cell_kzg_proof_batch_many_sets_device" in doc


def test_a_null_handle_refuses_the_call_and_marks_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    G = 3
    counts = (C.c_size_t * G)(2, 0, 1)
    ptr = C.cast(C.create_string_buffer(16), C.c_void_p)          # never read: the call is refused before it looks at an array
    out = C.create_string_buffer(176 * G)
    for fn, lead, forms in ((getattr(lib, VERIFY), (), ()), (getattr(lib, DEBUG), (out,), (0,))):
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert fn(*lead, ok, st, counts, ptr, ptr, ptr, ptr, G, *forms, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
        assert fn(*lead, ok, None, counts, ptr, ptr, ptr, ptr, G, *forms, None) == BADARGS
        assert fn(*lead, None, st, counts, ptr, ptr, ptr, ptr, G, *forms, None) == BADARGS
        assert fn(*lead, ok, st, counts, ptr, ptr, ptr, ptr, 0, *forms, None) == BADARGS      # a NULL handle is refused whatever the rest says
    ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
    assert getattr(lib, DEBUG)(None, ok, st, counts, ptr, ptr, ptr, ptr, G, 0, None) == BADARGS and list(st) == [BADARGS] * G


def test_what_the_counts_alone_refuse_is_refused_before_the_handle_is_read():
    """64 zero bytes stand in for a handle (NULL is refused one step earlier): a sum of the counts above 2^18 or one that overflows, a
    prep_form out of range, NULL counts, a NULL or misaligned array while the sum is above zero -- and groups == 0 touches nothing."""
    from kzg_rust_amd import _lib
    lib = _lib.load()
    G = 3
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    buf = C.create_string_buffer(64)
    base = C.addressof(buf)
    base += -base % 16
    verify, debug = getattr(lib, VERIFY), getattr(lib, DEBUG)
    out = C.create_string_buffer(176 * G)

    def both(counts, ptrs, groups=G, form=0):
        res = []
        for fn, lead, forms in ((verify, (), ()), (debug, (out,), (form,))):
            ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
            cnt = (C.c_size_t * G)(*counts) if counts is not None else None
            res.append((fn(*lead, ok, st, cnt, *ptrs, groups, *forms, fake), list(st), list(ok)))
        return res
    refused = (BADARGS, [BADARGS] * G, [False] * G)
    good = (base, base, base, base)
    for counts in ((1 << 18, 1, 0), (1 << 63, 1 << 63, 0), ((1 << 64) - 1, 2, 0), (0, 0, (1 << 18) + 1)):
        assert both(counts, good) == [refused] * 2, counts
    assert both(None, good) == [refused] * 2
    for bad in ((None, base, base, base), (base, None, base, base), (base + 8, base, base, base), (base, base, base + 8, base),
                (base, base, base, base + 8), (base, base + 4, base, base)):
        assert both((1, 0, 1), bad) == [refused] * 2, bad
    assert both((1, 0, 1), good, form=3)[1] == refused and both((1, 0, 1), good, form=-1)[1] == refused
    # groups == 0: nothing is touched
    assert both((1, 0, 1), good, groups=0) == [(0, [7] * G, [True] * G)] * 2


class FakeTensor:
    def __init__(self, numel, dtype="torch.uint8"):
        self._numel, self.dtype = numel, dtype

    def numel(self):
        return self._numel

    def data_ptr(self):
        return 0

    def is_contiguous(self):
        return True


def test_python_wrapper_checks_sizes_and_dtypes_against_the_counts_without_a_handle():
    import kzg_rust_amd as kz
    counts = [2, 0, 3]
    fit = dict(commitments=48 * 5, cell_indices=5, cells=2048 * 5, proofs=48 * 5)

    def tensors(**change):
        sizes = dict(fit, **{k: v for k, v in change.items() if isinstance(v, int)})
        dt = {k: v for k, v in change.items() if isinstance(v, str)}
        return [FakeTensor(sizes[k], dt.get(k, "torch.int64" if k == "cell_indices" else "torch.uint8")) for k in fit]
    for call in (kz.Kzg.verify_cell_kzg_proof_batch_many_sets_device, kz.Kzg.debug_cell_batch_intermediates_sets_device):
        for bad in (dict(commitments=48 * 6), dict(cell_indices=4), dict(cells=2048 * 5 + 1), dict(proofs=48 * 4),
                    dict(cell_indices="torch.int32"), dict(cells="torch.int64")):
            with pytest.raises(kz.BadArgs):
                call(*tensors(**bad), counts, None)
        with pytest.raises(kz.BadArgs):
            call(*tensors(), [2, -1, 4], None)
        with pytest.raises(kz.BadArgs):
            call(None, None, None, None, counts, None)            # missing arrays while the counts sum above zero
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_cell_batch_intermediates_sets_device(None, None, None, None, [0], None, prep_form=3)
    assert kz.Kzg.verify_cell_kzg_proof_batch_many_sets_device(None, None, None, None, [], None) == []


def test_the_ragged_preparation_uses_no_scratch_and_its_twins_lds(tmp_path):
    res = kernel_resources(tmp_path, "k_cell_prep")
    ragged = [k for k in res if re.fullmatch(r"_ZN3kzg\d+k_cell_prep_setsE.*", k)]
    uniform = [k for k in res if re.fullmatch(r"_ZN3kzg\d+k_cell_prepE.*", k)]
    assert len(ragged) == 1 and len(uniform) == 1, sorted(res)
    r, u = res[ragged[0]], res[uniform[0]]
    print("k_cell_prep", u, "| k_cell_prep_sets", r)
    assert r["scratch"] == 0 and not r["dynamic_stack"], r
    assert u["scratch"] == 0 and not u["dynamic_stack"], u
    assert r["lds"] == u["lds"], (u, r)
