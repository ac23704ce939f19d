"""-m "not gpu": verify_cell_kzg_proof_batch_many_sets (groups of different sizes in one call) at the boundary.  include/kzg355.h declares the call
and its debug form with their argument names, the built library exports them, the ctypes loader binds them, the Rust shim and the C++ mirror name
them, the Python wrapper refuses a group whose four lists differ in length before any FFI call, and a NULL handle refuses the whole call and marks
every status."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY, DEBUG = "kzg355_verify_cell_kzg_proof_batch_many_sets", "kzg355_debug_cell_batch_intermediates_sets"
BADARGS = 1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    verify = re.search(r"int\s+" + VERIFY + r"\s*\(([^)]*)\)\s*;", hdr)
    debug = re.search(r"int\s+" + DEBUG + r"\s*\(([^)]*)\)\s*;", hdr)
    assert verify and debug
    names = lambda m: [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]      # noqa: E731
    args = ["ok", "status", "cell_counts", "commitments", "cell_indices", "cells", "proofs", "groups", "s"]
    assert names(verify) == args
    assert names(debug) == ["out"] + args


def test_header_states_the_contract_where_a_reader_looks_for_it():
    hdr = read("include", "kzg355.h")
    comment = hdr[:hdr.index("int " + VERIFY)].rsplit("/*", 1)[1]
    for phrase in ("cell_counts[0] + ... + cell_counts[g-1]", "first appearance", "2^24", "2^18", "before any device is touched", "groups == 0",
                   "one set of launches", "uneven in", "force_sharded", "device-resident form", "kzg355_verify_blob_cell_proofs_batch_many"):
        assert phrase in comment, phrase


def test_library_exports_them_and_the_loader_binds_them():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    for n, argc in ((VERIFY, 9), (DEBUG, 10)):
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc


def test_mirrors_name_them():
    ffi = read("rust", "src", "ffi.rs")
    for n in (VERIFY, DEBUG):
        assert re.search(r"pub fn " + n + r"\s*\(", ffi)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn verify_cell_kzg_proof_batch_many_sets(" in rust and "ffi::" + VERIFY + "(" in rust
    hpp = read("include", "kzg355.hpp")
    assert VERIFY + "(" in hpp and "verify_cell_kzg_proof_batch_many_sets(const" in hpp.replace(VERIFY, "")
    assert "Kzg::verify_cell_kzg_proof_batch_many_sets" in read("INTEGRATION.md")


def test_python_wrapper_refuses_unequal_list_lengths_without_a_handle():
    import kzg_rust_amd as kz
    c, cell, p = bytes(48), bytes(2048), bytes(48)
    good = ([c] * 2, [0, 1], [cell] * 2, [p] * 2)
    for call in (kz.Kzg.verify_cell_kzg_proof_batch_many_sets, kz.Kzg.debug_cell_batch_intermediates_sets):
        for bad in (([c] * 3, [0, 1, 2], [cell] * 3, [p] * 2), ([c], [0, 1], [cell], [p]), ([], [], [cell], [])):
            with pytest.raises(kz.BadArgs):
                call([good, bad], None)
        with pytest.raises(kz.InvalidBytesLength):
            call([good, ([c], [0], [bytes(2047)], [p])], None)
    # the uniform wrapper keeps requiring equal sizes
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_cell_kzg_proof_batch_many([good, ([c], [0], [cell], [p])], None)


def test_a_null_handle_refuses_the_call_and_marks_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    G = 3
    counts, idx = (C.c_size_t * G)(2, 0, 1), (C.c_size_t * 3)(0, 1, 2)
    few = bytes(16)                                               # never read: the call is refused before it looks at an array
    out = C.create_string_buffer(176 * G)
    for fn, lead in ((getattr(lib, VERIFY), ()), (getattr(lib, DEBUG), (out,))):
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert fn(*lead, ok, st, counts, few, idx, few, few, G, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
        assert fn(*lead, ok, None, counts, few, idx, few, few, G, None) == BADARGS
        assert fn(*lead, None, st, counts, few, idx, few, few, G, None) == BADARGS
        assert fn(*lead, ok, st, counts, few, idx, few, few, 0, None) == BADARGS      # a NULL handle is refused whatever the rest says
