"""-m "not gpu": compute_cell_kzg_proofs_at (the proofs of chosen cells) at the boundary.  include/kzg355.h declares the three calls with their
argument names, the built library exports them, the ctypes loader binds them with the header's signatures, the Rust shim and the C++ mirror
name them, the Python wrapper refuses malformed lists before any FFI call, every refusal of the whole call that needs no device marks every
status, n == 0 touches nothing, and the gfx950 build of k_cell_quotient.hip gives the two new kernels no scratch."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE, MANY, DEVICE = NAMES = ["kzg355_compute_cell_kzg_proofs_at", "kzg355_compute_cell_kzg_proofs_at_many",
                                "kzg355_compute_cell_kzg_proofs_at_many_device"]
BADARGS = 1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_args(name):
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_three_calls():
    names = lambda n: [a.split()[-1].lstrip("*") for a in header_args(n)]      # noqa: E731
    assert names(SINGLE) == ["cells_out", "proofs_out", "blob", "cell_indices", "k", "s"]
    assert names(MANY) == ["cells_out", "proofs_out", "status", "blobs", "n", "cell_counts", "cell_indices", "s"]
    assert names(DEVICE) == ["d_cells_out", "d_proofs_out", "status", "d_blobs", "n", "cell_counts", "cell_indices", "s"]


def test_library_exports_them_and_the_loader_binds_the_headers_signatures():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    # a header argument as the loader spells it: byte buffers of the host forms as char pointers, device buffers and the handle as addresses
    kinds = {"uint8_t *": (C.c_char_p, C.c_void_p), "const uint8_t *": (C.c_char_p, C.c_void_p), "int *": (C.POINTER(C.c_int),),
             "const size_t *": (C.POINTER(C.c_size_t),), "size_t": (C.c_size_t,), "const kzg355_settings *": (C.c_void_p,)}
    for n in NAMES:
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, n)
        args = header_args(n)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args)
        for a, t in zip(args, fn.argtypes):
            decl = a.rsplit(" ", 1)[0] + (" *" if a.rsplit(" ", 1)[1].startswith("*") else "")
            assert t in kinds[decl], (n, a, t)
            if decl.endswith("uint8_t *"):
                assert t is (C.c_void_p if n == DEVICE else C.c_char_p), (n, a, t)


def test_mirrors_name_them():
    ffi = read("rust", "src", "ffi.rs")
    for n in NAMES:
        assert re.search(r"pub fn " + n + r"\s*\(", ffi)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn compute_cell_kzg_proofs_at(" in rust and "pub fn compute_cell_kzg_proofs_at_many(" in rust
    assert "ffi::" + MANY + "(" in rust
    hpp = read("include", "kzg355.hpp")
    for n in (SINGLE, MANY):
        assert n + "(" in hpp
    assert " compute_cell_kzg_proofs_at(" in hpp and " compute_cell_kzg_proofs_at_many(" in hpp


def test_python_wrapper_refuses_malformed_lists_without_a_handle():
    import kzg_rust_amd as kz
    blob = bytes(131072)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cell_kzg_proofs_at_many([blob, blob], [[0]], None)                 # two blobs, one list
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cell_kzg_proofs_at(blob, [-1], None)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.compute_cell_kzg_proofs_at(blob[:-1], [0], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cell_kzg_proofs_at_many_device(0, 2, [1, 1], [0], None, cells_out=0)      # the counts ask for two indices
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cell_kzg_proofs_at_many_device(0, 1, [1], [0], None)                      # no output


def test_refusals_of_the_whole_call_mark_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    n = 3
    counts, idx = (C.c_size_t * n)(2, 0, 1), (C.c_size_t * 3)(0, 127, 5)
    out = C.create_string_buffer(16)                              # never written: the calls are refused before they look at a blob
    # stands in for a handle where the refusal comes before the handle is looked at (no device here to load one on)
    handle = C.addressof(C.create_string_buffer(1 << 16))
    host_blobs, dev_blobs = bytes(16), 4096
    for name, blobs in ((MANY, host_blobs), (DEVICE, dev_blobs)):
        fn = getattr(lib, name)
        o = out if name == MANY else C.addressof(out)
        refused = [("NULL handle", (o, None, blobs, n, counts, idx, None)),
                   ("both outputs NULL", (None, None, blobs, n, counts, idx, handle)),
                   ("NULL blobs", (o, None, None, n, counts, idx, handle)),
                   ("NULL cell_counts", (o, None, blobs, n, None, idx, handle)),
                   ("NULL cell_indices", (None, o, blobs, n, counts, None, handle))]
        for what, (c, p, b, m, cn, ix, h) in refused:
            st = (C.c_int * n)(7, 7, 7)
            assert fn(c, p, st, b, m, cn, ix, h) == BADARGS, (name, what)
            assert list(st) == [BADARGS] * n, (name, what)
            assert fn(c, p, None, b, m, cn, ix, h) == BADARGS, (name, what)
        # n == 0: OK, and nothing is touched
        st = (C.c_int * n)(7, 7, 7)
        assert fn(o, None, st, None, 0, None, None, handle) == 0 and list(st) == [7, 7, 7] and out.raw == bytes(16), name
        assert fn(None, None, st, None, 0, None, None, handle) == BADARGS and list(st) == [7, 7, 7], name     # (no unit to mark)
    one = (C.c_size_t * 1)(0)
    assert lib.kzg355_compute_cell_kzg_proofs_at(out, None, host_blobs, one, 1, None) == BADARGS
    assert lib.kzg355_compute_cell_kzg_proofs_at(None, None, host_blobs, one, 1, handle) == BADARGS
    assert lib.kzg355_compute_cell_kzg_proofs_at(out, None, None, one, 1, handle) == BADARGS
    assert lib.kzg355_compute_cell_kzg_proofs_at(out, None, host_blobs, None, 1, handle) == BADARGS
    assert out.raw == bytes(16)


def test_new_kernels_use_no_scratch(tmp_path):
    res = kernel_resources(tmp_path, "k_cell_quotient")
    found = {}
    for short in ("k_cq_quotient", "k_cq_gather"):
        hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
        assert len(hits) == 1, (short, sorted(res))
        found[short] = res[hits[0]]
        print(short, found[short])
    for short, r in found.items():
        assert r["scratch"] == 0 and not r["dynamic_stack"], (short, r)
    assert found["k_cq_quotient"]["lds"] == 4096 * 9 * 4, found["k_cq_quotient"]      # Fr: nine 29-bit limbs
    assert found["k_cq_gather"]["lds"] == 0
