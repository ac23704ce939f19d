"""-m "not gpu": recover_cells_and_kzg_proofs at the boundary.  include/kzg355.h declares both entry points, the built library exports them,
the Rust shim, the C++ mirror and the ctypes loader name them, and the Python wrapper refuses a length mismatch before any FFI call."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kzg355_recover_cells_and_kzg_proofs", "kzg355_recover_cells_and_kzg_proofs_many"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    one = re.search(r"int\s+kzg355_recover_cells_and_kzg_proofs\s*\(([^)]*)\)\s*;", hdr)
    many = re.search(r"int\s+kzg355_recover_cells_and_kzg_proofs_many\s*\(([^)]*)\)\s*;", hdr)
    assert one and many
    names = lambda m: [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names(one) == ["cells_out", "proofs_out", "cell_indices", "cells", "n", "s"]
    assert names(many) == ["cells_out", "proofs_out", "status", "cell_indices", "cells", "n", "m", "s"]


def test_library_exports_them_and_the_loader_binds_them():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    for n in NAMES:
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, n).argtypes) == (6 if n == NAMES[0] else 8)


def test_mirrors_name_them():
    ffi = read("rust", "src", "ffi.rs")
    for n in NAMES:
        assert re.search(r"pub fn " + n + r"\s*\(", ffi)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn recover_cells_and_kzg_proofs(" in rust and "pub fn recover_cells_and_kzg_proofs_many(" in rust
    hpp = read("include", "kzg355.hpp")
    assert "recover_cells_and_kzg_proofs(const std::vector<size_t> &cell_indices" in hpp and NAMES[0] + "(" in hpp


def test_python_wrapper_refuses_a_length_mismatch_without_a_handle():
    import kzg_rust_amd as kz
    cell = bytes(2048)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs(list(range(64)), [cell] * 63, None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells(list(range(64)), [cell] * 65, None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_many(list(range(64)), [[cell] * 64, [cell] * 63], None)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.recover_cells(list(range(64)), [bytes(2047)] * 64, None)
