"""-m "not gpu": verify_blob_cell_proofs_batch at the boundary.  include/kzg355.h declares the five entry points, the built library exports them,
the ctypes loader and the Rust shim bind them with the same argument lists, a C11 consumer and the C++ mirror compile, every refusal that needs
no device marks every status, and the two kernels behind the call use no scratch (read from the code object the build left behind, as
tests/test_cell_kernel_resources.py reads k_cells.hip's)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARGS = 1
ARGS = {
    "kzg355_verify_blob_cell_proofs_batch": ["ok", "blobs", "n_blobs", "commitments", "n_commitments", "cell_proofs", "n_cell_proofs", "s"],
    "kzg355_verify_blob_cell_proofs_batch_many": ["ok", "status", "blobs", "commitments", "cell_proofs", "n_per_group", "groups", "s"],
    "kzg355_verify_blob_cell_proofs_batch_many_device": ["ok", "status", "d_blobs", "d_commitments", "d_cell_proofs", "n_per_group", "groups", "s"],
    "kzg355_debug_blob_cell_batch_intermediates":
        ["out", "ok", "status", "blobs", "commitments", "cell_proofs", "n_per_group", "groups", "interp_form", "s"],
    "kzg355_debug_blob_cell_batch_intermediates_device":
        ["out", "ok", "status", "d_blobs", "d_commitments", "d_cell_proofs", "n_per_group", "groups", "interp_form", "prep_form", "s"],
}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    from kzg_rust_amd import _lib
    return _lib.load()


def test_the_five_symbols_are_exported_and_bound_alike(lib):
    from kzg_rust_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", read("rust", "src", "ffi.rs"))
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, want in ARGS.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
        r = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", ffi)
        assert r and [a.split(":")[0].strip() for a in r.group(1).split(",")] == want, name
        assert name in exported and name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == len(want), name
    rust = read("rust", "src", "kzg.rs")
    for fn in ("verify_blob_cell_proofs_batch", "verify_blob_cell_proofs_batch_many"):
        assert "pub fn " + fn + "(" in rust and "ffi::kzg355_" + fn + "(" in rust
    assert "2048 blobs" in read("include", "kzg355.h"), "the header documents the cap on n_per_group"


def test_a_c11_consumer_and_the_cpp_mirror_compile(tmp_path):
    c = tmp_path / "consumer.c"
    c.write_text('#include "kzg355.h"\n'
                 "int probe(const kzg355_settings *s, const uint8_t *p, bool *ok, int *st, uint8_t *out) {\n"
                 "    int rc = kzg355_verify_blob_cell_proofs_batch(ok, p, 1, p, 1, p, 128, s);\n"
                 "    rc += kzg355_verify_blob_cell_proofs_batch_many(ok, st, p, p, p, 1, 1, s);\n"
                 "    rc += kzg355_verify_blob_cell_proofs_batch_many_device(ok, st, p, p, p, 1, 1, s);\n"
                 "    rc += kzg355_debug_blob_cell_batch_intermediates(out, ok, st, p, p, p, 1, 1, 0, s);\n"
                 "    rc += kzg355_debug_blob_cell_batch_intermediates_device(out, ok, st, p, p, p, 1, 1, 0, 0, s);\n"
                 "    return rc;\n}\n")
    out = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    cpp = tmp_path / "mirror.cpp"
    cpp.write_text('#include "kzg355.hpp"\n'
                   "int probe(const kzg355::KzgSettings &s) { return kzg355::Kzg::verify_blob_cell_proofs_batch({}, {}, {}, s).is_ok(); }\n")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(cpp)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_refusals_that_need_no_device_mark_every_status(lib):
    """Without a device no handle exists, so every case below is refused on its NULL handle at the latest; what is pinned is that such a call
    writes the code into the status (and false into the verdict) of EVERY group.  The checks themselves -- lengths, alignment, the forms --
    are met with a real handle in tests/test_gpu_blob_cells.py."""
    G = 3
    buf = C.create_string_buffer(64)
    host = C.cast(buf, C.c_char_p)
    for blobs, cms, proofs, n in ((host, host, host, 1), (None, host, host, 1), (host, None, host, 1), (host, host, None, 1),      # NULL arrays
                                  (host, host, host, 2049), (host, host, host, 1 << 40)):                                           # lengths
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert lib.kzg355_verify_blob_cell_proofs_batch_many(ok, st, blobs, cms, proofs, n, G, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
        ok, st, dbg = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7), C.create_string_buffer(176 * G)
        assert lib.kzg355_debug_blob_cell_batch_intermediates(dbg, ok, st, blobs, cms, proofs, n, G, 0, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
    for d_blobs, d_c, d_p, interp, prep in ((16, 16, 16, 0, 0), (17, 16, 16, 0, 0), (16, 24, 16, 0, 0), (16, 16, 8, 0, 0),          # misaligned
                                            (16, 16, 16, 3, 0), (16, 16, 16, -1, 0), (16, 16, 16, 0, 3), (0, 16, 16, 0, 0)):
        ok, st = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7)
        assert lib.kzg355_verify_blob_cell_proofs_batch_many_device(ok, st, d_blobs, d_c, d_p, 1, G, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
        ok, st, dbg = (C.c_bool * G)(True, True, True), (C.c_int * G)(7, 7, 7), C.create_string_buffer(176 * G)
        assert lib.kzg355_debug_blob_cell_batch_intermediates_device(dbg, ok, st, d_blobs, d_c, d_p, 1, G, interp, prep, None) == BADARGS
        assert list(st) == [BADARGS] * G and list(ok) == [False] * G
    # no output buffer, no verdict array
    st = (C.c_int * G)(7, 7, 7)
    assert lib.kzg355_debug_blob_cell_batch_intermediates(None, (C.c_bool * G)(), st, host, host, host, 1, G, 0, None) == BADARGS and list(st) == [BADARGS] * G
    st = (C.c_int * G)(7, 7, 7)
    assert lib.kzg355_verify_blob_cell_proofs_batch_many(None, st, host, host, host, 1, G, None) == BADARGS and list(st) == [BADARGS] * G
    # the one-group call: a NULL handle, and lengths that do not fit
    ok = C.c_bool(True)
    assert lib.kzg355_verify_blob_cell_proofs_batch(C.byref(ok), host, 1, host, 1, host, 128, None) == BADARGS
    assert lib.kzg355_verify_blob_cell_proofs_batch(None, host, 1, host, 1, host, 128, None) == BADARGS


def test_python_wrapper_refuses_before_any_ffi_call():
    import kzg_rust_amd as kz
    blob, c, p = bytes(131072), bytes(48), bytes(48)
    # (the settings argument is None: a wrapper that got as far as the FFI call would fail on its handle, not with BadArgs)
    for groups in ([([blob], [c, c], [p] * 128)], [([blob], [c], [p] * 127)], [([blob], [c], [p] * 128), ([blob] * 2, [c] * 2, [p] * 256)]):
        with pytest.raises(kz.BadArgs):
            kz.Kzg.verify_blob_cell_proofs_batch_many(groups, None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_blob_cell_batch_intermediates([([blob], [c], [p] * 128)], None, interp_form=3)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_blob_cell_batch_intermediates_device(16, 16, 16, 1, 1, None, prep_form=3)
    assert kz.Kzg.verify_blob_cell_proofs_batch_many([], None) == []


def test_the_new_kernels_use_no_scratch(tmp_path):
    res = kernel_resources(tmp_path, "k_blob_cells")
    found = {}
    for short in ("k_blob_weights", "k_blob_coef", "k_blob_meta"):
        hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
        assert len(hits) == 1, (short, sorted(res))
        found[short] = res[hits[0]]
        print(short, found[short])
    for short, r in found.items():
        assert r["scratch"] == 0 and not r["dynamic_stack"], (short, r)
    assert found["k_blob_coef"]["lds"] == 0 and found["k_blob_weights"]["lds"] == 128 * 36      # the 128 powers of r: Fr is nine words
