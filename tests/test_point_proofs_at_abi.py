"""-m "not gpu": compute_kzg_proofs_at (openings of blobs at chosen points) at the boundary.  include/kzg355.h declares the three calls with
their argument names, the built library exports them, the ctypes loader binds them with the header's signatures, the Rust shim and the C++
mirror name them with the same layouts, the Python wrapper refuses malformed lists before any FFI call, every refusal of the whole call that
needs no device marks every status, n == 0 touches nothing, and the gfx950 build of k_point_quotient.hip gives k_pq_quotient no scratch
(DESIGN.md section 19)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE, MANY, DEVICE = NAMES = ["kzg355_compute_kzg_proofs_at", "kzg355_compute_kzg_proofs_at_many", "kzg355_compute_kzg_proofs_at_many_device"]
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
    assert names(SINGLE) == ["proofs_out", "ys_out", "blob", "zs", "k", "s"]
    assert names(MANY) == ["proofs_out", "ys_out", "status", "blobs", "n", "point_counts", "zs", "s"]
    assert names(DEVICE) == ["d_proofs_out", "d_ys_out", "status", "d_blobs", "n", "point_counts", "zs", "s"]


def test_library_exports_them_and_the_loader_binds_the_headers_signatures():
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from kzg_rust_amd import _lib
    lib = _lib.load()
    kinds = {"uint8_t *": (C.c_char_p, C.c_void_p), "const uint8_t *": (C.c_char_p, C.c_void_p), "int *": (C.POINTER(C.c_int),),
             "const size_t *": (C.POINTER(C.c_size_t),), "size_t": (C.c_size_t,), "const kzg355_settings *": (C.c_void_p,)}
    for n in NAMES:
        assert n in exported and n in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, n)
        args = header_args(n)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args)
        for a, t in zip(args, fn.argtypes):
            decl, arg = a.rsplit(" ", 1)[0] + (" *" if a.rsplit(" ", 1)[1].startswith("*") else ""), a.rsplit(" ", 1)[1].lstrip("*")
            assert t in kinds[decl], (n, a, t)
            if decl.endswith("uint8_t *"):                         # device buffers as addresses; the points stay host bytes in every form
                assert t is (C.c_void_p if arg.startswith("d_") else C.c_char_p), (n, a, t)


def test_mirrors_name_them_with_the_same_layouts():
    ffi = read("rust", "src", "ffi.rs")
    for n in NAMES:
        assert re.search(r"pub fn " + n + r"\s*\(", ffi)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn compute_kzg_proofs_at(" in rust and "pub fn compute_kzg_proofs_at_many(" in rust and "ffi::" + MANY + "(" in rust
    hpp = read("include", "kzg355.hpp")
    for n in (SINGLE, MANY):
        assert n + "(" in hpp
    assert " compute_kzg_proofs_at(" in hpp and " compute_kzg_proofs_at_many(" in hpp
    # slot j of the flat outputs is 48 bytes of proof and 32 bytes of y in all three mirrors, and unit i owns the next counts[i] slots
    py = read("kzg_rust_amd", "kzg.py")
    body = py[py.index("def compute_kzg_proofs_at_many("):py.index("def compute_kzg_proofs_at(")]
    assert "praw[48 * j:48 * (j + 1)]" in body and "yraw[32 * j:32 * (j + 1)]" in body and "off += k" in body
    body = hpp[hpp.index(" compute_kzg_proofs_at_many("):]
    body = body[:body.index("// ---- the EIP-4844 point-evaluation precompile")]
    assert "&pr[j * 48], 48" in body and "&ys[j * 32], 32" in body and "off += counts[i]" in body
    body = rust[rust.index("pub fn compute_kzg_proofs_at_many("):]
    body = body[:body.index("pub fn kzg_to_versioned_hash_many(")]
    assert "proofs[48 * j..48 * (j + 1)]" in body and "ys[32 * j..32 * (j + 1)]" in body and "off + counts[i]" in body


def test_python_wrapper_refuses_malformed_lists_without_a_handle():
    import kzg_rust_amd as kz
    blob, z = bytes(131072), bytes(32)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at_many([blob, blob], [[z]], None)                      # two blobs, one list
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at(blob, [z[:-1]], None)                                # a point of 31 bytes
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.compute_kzg_proofs_at(blob[:-1], [z], None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at_many([blob], [[z]], None, proofs=False, ys=False)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at_many_device(0, 2, [1, 1], [z], None, ys_out=0)       # the counts ask for two points
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at_many_device(0, 1, [1], [z], None)                    # no output


def test_refusals_of_the_whole_call_mark_every_status():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    n = 3
    counts, zs = (C.c_size_t * n)(2, 0, 1), bytes(96)
    out = C.create_string_buffer(16)                              # never written: the calls are refused before they look at a blob
    # stands in for a handle where the refusal comes before the handle is looked at (no device here to load one on); all zeros, it reads as a
    # handle of another FIELD_ELEMENTS_PER_BLOB where it is looked at
    handle = C.addressof(C.create_string_buffer(1 << 16))
    host_blobs, dev_blobs = bytes(16), 4096
    top = (2 ** 64 - 1) // 48
    for name, blobs in ((MANY, host_blobs), (DEVICE, dev_blobs)):
        fn = getattr(lib, name)
        o = out if name == MANY else C.addressof(out)
        refused = [("NULL handle", (o, None, blobs, n, counts, zs, None)),
                   ("both outputs NULL", (None, None, blobs, n, counts, zs, handle)),
                   ("NULL blobs", (o, None, None, n, counts, zs, handle)),
                   ("NULL point_counts", (o, None, blobs, n, None, zs, handle)),
                   ("NULL zs", (None, o, blobs, n, counts, None, handle)),
                   ("another FIELD_ELEMENTS_PER_BLOB", (o, None, blobs, n, counts, zs, handle)),
                   ("a sum that leaves size_t", (o, None, blobs, n, (C.c_size_t * n)(2 ** 64 - 1, 1, 0), zs, handle)),
                   ("a sum that leaves size_t times 48", (o, None, blobs, n, (C.c_size_t * n)(top, 1, 0), zs, handle))]
        if name == DEVICE:
            refused += [("misaligned d_proofs_out", (C.addressof(out) + 8, None, blobs, n, counts, zs, handle)),
                        ("misaligned d_ys_out", (None, C.addressof(out) + 8, blobs, n, counts, zs, handle)),
                        ("misaligned d_blobs", (o, None, blobs + 8, n, counts, zs, handle))]
        for what, (p, y, b, m, cn, z, h) in refused:
            st = (C.c_int * n)(7, 7, 7)
            assert fn(p, y, st, b, m, cn, z, h) == BADARGS, (name, what)
            assert list(st) == [BADARGS] * n, (name, what)
            assert fn(p, y, None, b, m, cn, z, h) == BADARGS, (name, what)
        # n > 2^32: refused from n alone (nothing of n entries is read: the status pointer is NULL)
        assert fn(o, None, None, blobs, 2 ** 32 + 1, counts, zs, handle) == BADARGS, name
        # n == 0: OK, and nothing is touched
        st = (C.c_int * n)(7, 7, 7)
        assert fn(o, None, st, None, 0, None, None, handle) == 0 and list(st) == [7, 7, 7] and out.raw == bytes(16), name
        assert fn(None, None, st, None, 0, None, None, handle) == BADARGS and list(st) == [7, 7, 7], name     # (no unit to mark)
    z1 = bytes(32)
    assert lib.kzg355_compute_kzg_proofs_at(out, None, host_blobs, z1, 1, None) == BADARGS
    assert lib.kzg355_compute_kzg_proofs_at(None, None, host_blobs, z1, 1, handle) == BADARGS
    assert lib.kzg355_compute_kzg_proofs_at(out, None, None, z1, 1, handle) == BADARGS
    assert lib.kzg355_compute_kzg_proofs_at(out, None, host_blobs, None, 1, handle) == BADARGS
    assert lib.kzg355_compute_kzg_proofs_at(out, None, host_blobs, z1, 1, handle) == BADARGS      # (the stand-in is no mainnet handle)
    assert out.raw == bytes(16)


def test_the_new_kernel_uses_no_scratch(tmp_path):
    res = kernel_resources(tmp_path, "k_point_quotient")
    hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+k_pq_quotientE.*", k)]
    assert len(hits) == 1 and len(res) == 1, sorted(res)
    r = res[hits[0]]
    print("k_pq_quotient", r)
    assert r["scratch"] == 0 and not r["dynamic_stack"], r
    assert r["lds"] == 4096 * 9 * 4, r                            # Fr: nine 29-bit limbs; the scan's exchange lives inside a[]
    assert r["vgprs"] <= 128, r                                   # 512 threads: two waves per SIMD, far below their 256 registers each
