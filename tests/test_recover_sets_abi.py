"""-m "not gpu": recover_cells_and_kzg_proofs_many_sets (every blob with its own index set) at the boundary.  include/kzg355.h declares the host
and the device form with their argument names, the built library exports them, the ctypes loader binds them, the Rust shim and the C++ mirror
name them, the Python wrapper refuses a malformed unit before any FFI call, and a NULL handle refuses the whole call and marks every status."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kzg355_recover_cells_and_kzg_proofs_many_sets", "kzg355_recover_cells_and_kzg_proofs_many_sets_device"]
BADARGS = 1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    host = re.search(r"int\s+kzg355_recover_cells_and_kzg_proofs_many_sets\s*\(([^)]*)\)\s*;", hdr)
    dev = re.search(r"int\s+kzg355_recover_cells_and_kzg_proofs_many_sets_device\s*\(([^)]*)\)\s*;", hdr)
    assert host and dev
    names = lambda m: [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names(host) == ["cells_out", "proofs_out", "status", "cell_counts", "cell_indices", "cells", "m", "s"]
    assert names(dev) == ["d_cells_out", "d_proofs_out", "status", "cell_counts", "cell_indices", "d_cells", "m", "s"]


def test_library_exports_them_and_the_loader_binds_them():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    for n in NAMES:
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, n).argtypes) == 8


def test_mirrors_name_them():
    ffi = read("rust", "src", "ffi.rs")
    for n in NAMES:
        assert re.search(r"pub fn " + n + r"\s*\(", ffi)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn recover_cells_and_kzg_proofs_many_sets(" in rust and "pub unsafe fn recover_cells_and_kzg_proofs_many_sets_device(" in rust
    for n in NAMES:
        assert "ffi::" + n + "(" in rust
    hpp = read("include", "kzg355.hpp")
    for n in NAMES:
        assert n + "(" in hpp
    assert "recover_cells_and_kzg_proofs_many_sets(" in hpp.replace("kzg355_recover", "") and "recover_cells_and_kzg_proofs_many_sets_device(" in hpp


def test_python_wrapper_refuses_a_malformed_unit_without_a_handle():
    import kzg_rust_amd as kz
    cell = bytes(2048)
    good = (list(range(64)), [cell] * 64)
    for call in (kz.Kzg.recover_cells_and_kzg_proofs_many_sets, kz.Kzg.recover_cells_many_sets):
        with pytest.raises(kz.BadArgs):
            call([good, (list(range(64)), [cell] * 63)], None)
        with pytest.raises(kz.InvalidBytesLength):
            call([good, (list(range(64)), [cell] * 63 + [bytes(2047)])], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_many_sets_device([64, 64], list(range(64)), 0, None, cells_out=0)      # the counts ask for 128 indices


def test_a_null_handle_refuses_the_call_and_marks_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    m = 3
    counts, idx = (C.c_size_t * m)(64, 64, 64), (C.c_size_t * (64 * m))(*(list(range(64)) * m))
    out = C.create_string_buffer(16)                              # never written: the call is refused before it looks at the cells
    for name, data in ((NAMES[0], bytes(16)), (NAMES[1], 4096)):
        st = (C.c_int * m)(7, 7, 7)
        assert getattr(lib, name)(out, None, st, counts, idx, data, m, None) == BADARGS
        assert list(st) == [BADARGS] * m
        assert getattr(lib, name)(out, None, None, counts, idx, data, m, None) == BADARGS
