"""-m "not gpu": verify_blob_cell_proofs_batch_many_sets (blob transactions of different blob counts in one call) at the boundary.
include/kzg355.h declares the four functions with their argument names and states the contract in the comment above them, the built library
exports them, the ctypes loader binds them, the Rust shim and the C++ mirror name them, the Python wrappers refuse a group whose three lists do
not fit before any FFI call, a NULL handle refuses the whole call and marks every status, a count of 2049 refuses it before the handle is looked
at, and the ragged kernel entries of k_blob_cells.hip and k_cell_prep.hip use no scratch, no dynamic stack and the LDS of their uniform twins."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY, VERIFY_DEV = "kzg355_verify_blob_cell_proofs_batch_many_sets", "kzg355_verify_blob_cell_proofs_batch_many_sets_device"
DEBUG, DEBUG_DEV = "kzg355_debug_blob_cell_batch_intermediates_sets", "kzg355_debug_blob_cell_batch_intermediates_sets_device"
BADARGS = 1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_four_functions():
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    names = lambda m: [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]      # noqa: E731
    host = ["ok", "status", "blob_counts", "blobs", "commitments", "cell_proofs", "groups"]
    dev = ["ok", "status", "blob_counts", "d_blobs", "d_commitments", "d_cell_proofs", "groups"]
    want = {VERIFY: host + ["s"], VERIFY_DEV: dev + ["s"], DEBUG: ["out"] + host + ["interp_form", "s"],
            DEBUG_DEV: ["out"] + dev + ["interp_form", "prep_form", "s"]}
    for fn, args in want.items():
        m = re.search(r"int\s+" + fn + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and names(m) == args, fn


def test_header_states_the_contract_where_a_reader_looks_for_it():
    hdr = read("include", "kzg355.h")
    comment = hdr[:hdr.index("int " + VERIFY + "(")].rsplit("/*", 1)[1]
    for phrase in ("blob_counts[0] + ... + blob_counts[g-1]", "no padding", "first appearance", "128 * count", "2^24", "2048", "131072",
                   "before any device\n * is touched", "groups == 0", "one set of\n * launches", "uneven in", "never cut", "not limited",
                   "kzg355_settings_cell_calls_per_device"):
        assert phrase in comment, phrase
    dev = hdr[:hdr.index("int " + VERIFY_DEV + "(")].rsplit("/*", 1)[1]
    for phrase in ("16-byte aligned", "HOST pointers", "first device", "deduplication", "uniform shapes only"):
        assert phrase in dev, phrase
    # the cell call's comment no longer says that this is missing
    cell = hdr[:hdr.index("int kzg355_verify_cell_kzg_proof_batch_many_sets(")].rsplit("/*", 1)[1]
    assert "are offered" in cell and "it needs this call's chain" not in cell


def test_library_exports_them_and_the_loader_binds_them():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    for n, argc in ((VERIFY, 8), (VERIFY_DEV, 8), (DEBUG, 10), (DEBUG_DEV, 11)):
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc


def test_mirrors_name_them():
    ffi = read("rust", "src", "ffi.rs")
    for n in (VERIFY, VERIFY_DEV, DEBUG, DEBUG_DEV):
        assert re.search(r"pub fn " + n + r"\s*\(", ffi), n
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn verify_blob_cell_proofs_batch_many_sets(" in rust and "ffi::" + VERIFY + "(" in rust
    hpp = read("include", "kzg355.hpp")
    assert VERIFY + "(" in hpp and "verify_blob_cell_proofs_batch_many_sets(const" in hpp.replace(VERIFY, "")
    assert "Kzg::verify_blob_cell_proofs_batch_many_sets" in read("INTEGRATION.md")


def test_python_wrappers_refuse_unfitting_lengths_without_a_handle():
    import kzg_rust_amd as kz
    blob, c, p = bytes(131072), bytes(48), bytes(48)
    good = ([blob] * 2, [c] * 2, [p] * 256)
    for call in (kz.Kzg.verify_blob_cell_proofs_batch_many_sets, kz.Kzg.debug_blob_cell_batch_intermediates_sets):
        for bad in (([blob], [c] * 2, [p] * 128), ([blob], [c], [p] * 127), ([blob] * 2, [c] * 2, [p] * 128), ([], [c], [])):
            with pytest.raises(kz.BadArgs):
                call([good, bad], None)
        with pytest.raises(kz.InvalidBytesLength):
            call([good, ([bytes(131071)], [c], [p] * 128)], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_blob_cell_batch_intermediates_sets([good], None, 3)
    for bad in (dict(interp_form=3), dict(prep_form=3)):
        with pytest.raises(kz.BadArgs):
            kz.Kzg.debug_blob_cell_batch_intermediates_sets_device(None, None, None, [0], None, **bad)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_blob_cell_proofs_batch_many_sets_device(None, None, None, [1, -1], None)
    # the uniform wrapper keeps requiring equal sizes
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_blob_cell_proofs_batch_many([good, ([blob], [c], [p] * 128)], None)


def _calls(lib, G):
    out = C.create_string_buffer(176 * G)
    return ((getattr(lib, VERIFY), (), ()), (getattr(lib, VERIFY_DEV), (), ()), (getattr(lib, DEBUG), (out,), (0,)), (getattr(lib, DEBUG_DEV), (out,), (0, 0)))


def test_a_null_handle_refuses_the_call_and_marks_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    G = 3
    counts = (C.c_size_t * G)(2, 0, 1)
    few = C.create_string_buffer(16)                              # never read: the call is refused before it looks at an array
    ptr = C.cast(few, C.c_void_p)
    for fn, lead, forms in _calls(lib, G):
        a = (ptr, ptr, ptr) if "_device" in fn.__name__ else (few, few, few)
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert fn(*lead, ok, st, counts, *a, G, *forms, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
        assert fn(*lead, ok, None, counts, *a, G, *forms, None) == BADARGS
        assert fn(*lead, None, st, counts, *a, G, *forms, None) == BADARGS
        assert fn(*lead, ok, st, counts, *a, 0, *forms, None) == BADARGS       # a NULL handle is refused whatever the rest says


def test_a_count_of_2049_is_refused_from_the_counts_alone():
    """Everything that refuses the call is decided before the handle is looked at, so a handle that is no handle is never read: 64 zero bytes
    stand in for it (NULL is refused one step earlier).  So are groups above 2^24, forms out of range and -- with counts of at most 2048 that
    sum above zero -- a NULL array."""
    from kzg_rust_amd import _lib
    lib = _lib.load()
    G = 3
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    few = C.create_string_buffer(16)
    ptr = C.cast(few, C.c_void_p)
    for fn, lead, forms in _calls(lib, G):
        a = (ptr, ptr, ptr) if "_device" in fn.__name__ else (few, few, few)
        for counts in ((1, 2049, 1), (2049, 0, 0), (0, 0, 2 ** 64 - 1)):
            ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
            assert fn(*lead, ok, st, (C.c_size_t * G)(*counts), *a, G, *forms, fake) == BADARGS, (fn.__name__, counts)
            assert list(st) == [BADARGS] * G and list(ok) == [False] * G
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert fn(*lead, ok, st, None, *a, G, *forms, fake) == BADARGS and list(st) == [BADARGS] * G
        null = (None, a[1], a[2])
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert fn(*lead, ok, st, (C.c_size_t * G)(1, 0, 2048), *null, G, *forms, fake) == BADARGS and list(st) == [BADARGS] * G
        assert fn(*lead, ok, st, (C.c_size_t * G)(1, 0, 1), *a, 0, *forms, fake) == 0 and list(st) == [BADARGS] * G      # groups == 0: nothing touched
    out = C.create_string_buffer(176 * G)
    for forms in ((3, 0), (0, 3), (-1, 0)):
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert getattr(lib, DEBUG_DEV)(out, ok, st, (C.c_size_t * G)(1, 0, 1), ptr, ptr, ptr, G, *forms, fake) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G


def _entries(res, short):
    hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
    assert len(hits) == 1, (short, sorted(res))
    return res[hits[0]]


def test_ragged_kernel_entries_use_no_scratch_and_their_twins_lds(tmp_path):
    pairs = {"k_blob_cells": ("k_blob_meta", "k_blob_weights", "k_blob_coef"), "k_cell_prep": ("k_cell_rhash_lanes", "k_cell_rhash_wave")}
    for unit, kernels in pairs.items():
        res = kernel_resources(tmp_path, unit)
        for short in kernels:
            uniform, ragged = _entries(res, short), _entries(res, short + "_sets")
            print(short, uniform, "| _sets", ragged)
            assert ragged["scratch"] == 0 and not ragged["dynamic_stack"], (short, ragged)
            assert ragged["lds"] == uniform["lds"], (short, uniform, ragged)
    assert len([k for k in kernel_resources(tmp_path, "k_blob_cells") if "_sets" in k]) == 3      # and no `_sets` entry but these
