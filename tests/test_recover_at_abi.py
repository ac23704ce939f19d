"""-m "not gpu": recover_cells_and_kzg_proofs_at (the chosen cells of recovered blobs and their proofs) at the boundary.  include/kzg355.h
declares the three calls with their argument names, the built library exports them, the ctypes loader binds them with the header's
signatures, the Rust shim and the C++ mirror name them, the Python wrappers refuse malformed lists before any FFI call, every refusal of the
whole call that needs no device marks every status, m == 0 touches nothing, and the gfx950 build of k_cell_recover_at.hip gives the new
kernel no scratch."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE, SETS, DEVICE = NAMES = ["kzg355_recover_cells_and_kzg_proofs_at", "kzg355_recover_cells_and_kzg_proofs_at_many_sets",
                                "kzg355_recover_cells_and_kzg_proofs_at_many_sets_device"]
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
    assert names(SINGLE) == ["cells_out", "proofs_out", "cell_indices", "cells", "n", "want_indices", "k", "s"]
    assert names(SETS) == ["cells_out", "proofs_out", "status", "cell_counts", "cell_indices", "cells", "want_counts", "want_indices", "m", "s"]
    assert names(DEVICE) == ["d_cells_out", "d_proofs_out", "status", "cell_counts", "cell_indices", "d_cells", "want_counts", "want_indices", "m", "s"]
    # what is not offered is said where a caller looks for it
    hdr = " ".join(read("include", "kzg355.h").replace("\n * ", " ").split())
    assert "Not offered: a form with one index set shared by all blobs" in hdr and "a switch to the FK20 chain" in hdr


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
    assert "pub fn recover_cells_and_kzg_proofs_at(" in rust and "pub fn recover_cells_and_kzg_proofs_at_many_sets(" in rust
    assert "pub unsafe fn recover_cells_and_kzg_proofs_at_many_sets_device(" in rust
    assert "ffi::" + SETS + "(" in rust and "ffi::" + DEVICE + "(" in rust
    hpp = read("include", "kzg355.hpp")
    for n in (SINGLE, SETS):
        assert n + "(" in hpp
    assert " recover_cells_and_kzg_proofs_at(" in hpp and " recover_cells_and_kzg_proofs_at_many_sets(" in hpp


def test_python_wrappers_refuse_malformed_lists_without_a_handle():
    import kzg_rust_amd as kz
    cell = bytes(2048)
    ix = list(range(64))
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_at(ix, [cell] * 63, [0], None)                      # 64 indices, 63 cells
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_at_many_sets([(ix, [cell] * 64, [0]), (ix, [cell] * 65, [])], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_at(ix, [cell] * 64, [-1], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_at([-1] + ix[1:], [cell] * 64, [0], None)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.recover_cells_and_kzg_proofs_at(ix, [cell] * 63 + [cell[:-1]], [0], None)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.recover_missing_cells_and_kzg_proofs(ix, [cell] * 63 + [cell[:-1]], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_missing_cells_and_kzg_proofs(ix, [cell] * 65, None)
    dev = kz.Kzg.recover_cells_and_kzg_proofs_at_many_sets_device
    with pytest.raises(kz.BadArgs):
        dev([64, 64], ix, 0, [1, 1], [0, 1], None, cells_out=0)                                  # the cell counts ask for 128 indices
    with pytest.raises(kz.BadArgs):
        dev([64], ix, 0, [2], [0], None, cells_out=0)                                            # the want counts ask for two indices
    with pytest.raises(kz.BadArgs):
        dev([64], ix, 0, [1, 0], [0], None, cells_out=0)                                         # one blob, two want counts
    with pytest.raises(kz.BadArgs):
        dev([64], ix, 0, [1], [0], None)                                                         # no output


def test_refusals_of_the_whole_call_mark_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    m = 3
    sz = lambda *v: (C.c_size_t * len(v))(*v)                                   # noqa: E731
    kc, ki = sz(64, 64, 64), sz(*(list(range(64)) * 3))
    wc, wi = sz(2, 0, 1), sz(0, 127, 5)
    backing = C.create_string_buffer(48)
    # never written: the calls are refused before they look at a cell (16-byte aligned, so that the device form refuses for the reason named)
    out = (C.c_char * 16).from_address((C.addressof(backing) + 15) & ~15)
    # stands in for a handle where the refusal comes before the handle is looked at (no device here to load one on)
    handle = C.addressof(C.create_string_buffer(1 << 16))
    host_cells, dev_cells = bytes(16), 4096
    big = (1 << 64) - 64
    for name, cells in ((SETS, host_cells), (DEVICE, dev_cells)):
        fn = getattr(lib, name)
        o = out if name == SETS else C.addressof(out)
        refused = [("NULL handle", (o, None, kc, ki, cells, wc, wi, None)),
                   ("both outputs NULL", (None, None, kc, ki, cells, wc, wi, handle)),
                   ("NULL cell_counts", (o, None, None, ki, cells, wc, wi, handle)),
                   ("NULL cell_indices", (o, None, kc, None, cells, wc, wi, handle)),
                   ("NULL cells", (o, None, kc, ki, None, wc, wi, handle)),
                   ("NULL want_counts", (None, o, kc, ki, cells, None, wi, handle)),
                   ("NULL want_indices", (None, o, kc, ki, cells, wc, None, handle)),
                   ("cell counts pass 2^64", (o, None, sz(64, big, 64), ki, cells, wc, wi, handle)),
                   ("want counts pass 2^64", (o, None, kc, ki, cells, sz(2, big, 64), wi, handle)),
                   ("cell counts times 2048 pass 2^64", (o, None, sz(64, 1 << 53, 64), ki, cells, wc, wi, handle)),
                   ("want counts times 2048 pass 2^64", (o, None, kc, ki, cells, sz(2, 1 << 53, 1), wi, handle))]
        if name == DEVICE:
            refused += [("d_cells_out misaligned", (o + 8, None, kc, ki, cells, wc, wi, handle)),
                        ("d_proofs_out misaligned", (None, o + 8, kc, ki, cells, wc, wi, handle)),
                        ("d_cells misaligned", (o, None, kc, ki, cells + 8, wc, wi, handle))]
        for what, (c, p, a, b, d, e, f, h) in refused:
            st = (C.c_int * m)(7, 7, 7)
            assert fn(c, p, st, a, b, d, e, f, m, h) == BADARGS, (name, what)
            assert list(st) == [BADARGS] * m, (name, what)
            assert fn(c, p, None, a, b, d, e, f, m, h) == BADARGS, (name, what)
        # m above 2^32 (no status array: it would have to hold m words)
        assert fn(o, None, None, kc, ki, cells, wc, wi, (1 << 32) + 1, handle) == BADARGS, name
        # m == 0: OK, and nothing is touched
        st = (C.c_int * m)(7, 7, 7)
        assert fn(o, None, st, None, None, None, None, None, 0, handle) == 0 and list(st) == [7, 7, 7] and out.raw == bytes(16), name
        assert fn(None, None, st, None, None, None, None, None, 0, handle) == BADARGS and list(st) == [7, 7, 7], name     # (no unit to mark)
    single = lib.kzg355_recover_cells_and_kzg_proofs_at
    one = sz(0)
    assert single(out, None, ki, host_cells, 64, one, 1, None) == BADARGS
    assert single(None, None, ki, host_cells, 64, one, 1, handle) == BADARGS
    assert single(out, None, None, host_cells, 64, one, 1, handle) == BADARGS
    assert single(out, None, ki, None, 64, one, 1, handle) == BADARGS
    assert single(out, None, ki, host_cells, 64, None, 1, handle) == BADARGS
    assert out.raw == bytes(16)


def test_new_kernel_uses_no_scratch(tmp_path):
    res = kernel_resources(tmp_path, "k_cell_recover_at")
    hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+k_rc_cells_atE.*", k)]
    assert len(hits) == 1, sorted(res)
    r = res[hits[0]]
    print("k_rc_cells_at", r)
    assert r["scratch"] == 0 and not r["dynamic_stack"], r
    assert r["lds"] == 64 * 9 * 4, r                                # one cell of Fr: nine 29-bit limbs each
