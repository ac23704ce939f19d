"""-m "not gpu": kzg355_verify_blob_kzg_proof_batch_many_sets, its device form, the two debug forms and the per-device counter at the boundary.
include/kzg355.h declares them, the built library exports them, the ctypes loader and the Rust shim bind them with the same argument lists, a
C11 -pedantic consumer compiles and links, the Python and C++ mirrors refuse what they can before any call into the library, and every
whole-call refusal the header lists is KZG355_BADARGS with every status marked and every verdict false.

Without a GPU no handle can be loaded.  The refusals are decided from the counts alone, before the handle is read or a device touched, so the C
consumer below hands them an opaque non-NULL handle that is never a loaded one: a refusal that came too late would read it, which is why those
calls run in a process of their own and not inside pytest."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARGS = 1
ARGS = {
    "kzg355_verify_blob_kzg_proof_batch_many_sets": ["ok", "status", "blob_counts", "blobs", "commitments", "proofs", "groups", "s"],
    "kzg355_verify_blob_kzg_proof_batch_many_sets_device": ["ok", "status", "blob_counts", "d_blobs", "d_commitments", "d_proofs", "groups", "s"],
    "kzg355_debug_batch_intermediates_sets": ["out", "ok", "status", "blob_counts", "blobs", "commitments", "proofs", "groups", "s"],
    "kzg355_debug_batch_intermediates_sets_device": ["out", "ok", "status", "blob_counts", "d_blobs", "d_commitments", "d_proofs", "groups", "s"],
    "kzg355_settings_blob_sets_blobs_per_device": ["s", "out", "cap"],
    "kzg355_settings_set_blob_sets_max_blobs": ["s", "max_blobs"],
}
BOUND_BY_THE_SHIM = ("kzg355_verify_blob_kzg_proof_batch_many_sets", "kzg355_verify_blob_kzg_proof_batch_many_sets_device")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    from kzg_rust_amd import _lib
    return _lib.load()


def test_header_export_map_loader_and_shim_agree(lib):
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
        assert name in exported and name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want) and fn.restype is C.c_int, name
        if name in BOUND_BY_THE_SHIM:
            r = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", ffi)
            assert r and [a.split(":")[0].strip() for a in r.group(1).split(",")] == want, name
    # the uniform call's conventions: ok, status, then the counts in front of the three arrays
    for name in BOUND_BY_THE_SHIM:
        fn = getattr(lib, name)
        assert fn.argtypes[0] == C.POINTER(C.c_bool) and fn.argtypes[1] == C.POINTER(C.c_int) and fn.argtypes[2] == C.POINTER(C.c_size_t)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn verify_blob_kzg_proof_batch_many_sets(" in rust and "ffi::kzg355_verify_blob_kzg_proof_batch_many_sets(" in rust
    # the set limit is a setter on the handle, documented in the header; kzg355_options and the environment are as they were
    assert "32768" in read("include", "kzg355.h") and not [n for n, _ in _lib.Options._fields_ if "blob_sets" in n]
    assert "BLOB_SETS" not in read("kzg_rust_amd", "csrc", "options.hip")


def test_null_handle_is_badargs_with_every_status_marked(lib):
    G = 3
    counts = (C.c_size_t * G)(1, 0, 2)
    buf = C.create_string_buffer(3 * 131072)
    out = C.create_string_buffer(128 * G)
    calls = [lambda ok, st: lib.kzg355_verify_blob_kzg_proof_batch_many_sets(ok, st, counts, buf, buf, buf, G, None),
             lambda ok, st: lib.kzg355_verify_blob_kzg_proof_batch_many_sets_device(ok, st, counts, 16, 16, 16, G, None),
             lambda ok, st: lib.kzg355_debug_batch_intermediates_sets(out, ok, st, counts, buf, buf, buf, G, None),
             lambda ok, st: lib.kzg355_debug_batch_intermediates_sets_device(out, ok, st, counts, 16, 16, 16, G, None)]
    for call in calls:
        ok, st = (C.c_bool * G)(*([True] * G)), (C.c_int * G)(*([7] * G))
        assert call(ok, st) == BADARGS and list(st) == [BADARGS] * G and list(ok) == [False] * G
        ok = (C.c_bool * G)(*([True] * G))
        assert call(ok, None) == BADARGS and list(ok) == [False] * G            # a NULL status array is legal
        st = (C.c_int * G)(*([7] * G))
        assert call(None, st) == BADARGS and list(st) == [BADARGS] * G          # a NULL ok is refused, the statuses still say so
    assert lib.kzg355_settings_blob_sets_blobs_per_device(None, None, 0) == BADARGS
    assert lib.kzg355_settings_set_blob_sets_max_blobs(None, 5) == BADARGS


CONSUMER = r'''
#include "kzg355.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long long opaque[8192];                       /* never a loaded handle: a refusal decided from the counts alone does not read it */
static _Alignas(16) uint8_t arr[64];
static int fails = 0;
static void expect(int cond, const char *what) { if (!cond) { fails++; printf("FAIL %s\n", what); } }
static int marked(const bool *ok, const int *st, size_t n) {
    size_t i;
    for (i = 0; i < n; i++) if (ok[i] || st[i] != KZG355_BADARGS) return 0;
    return 1;
}
typedef int (*plain_fn)(bool *, int *, const size_t *, const uint8_t *, const uint8_t *, const uint8_t *, size_t, const kzg355_settings *);
typedef int (*debug_fn)(uint8_t *, bool *, int *, const size_t *, const uint8_t *, const uint8_t *, const uint8_t *, size_t, const kzg355_settings *);
static plain_fn plain[2];
static debug_fn debug[2];
static uint8_t out[4 * 128];
/* form 0, 1: the plain calls on host / device arrays; 2, 3: the debug forms */
static int call(int form, bool *ok, int *st, const size_t *counts, const uint8_t *b, const uint8_t *c, const uint8_t *p, size_t groups,
                const kzg355_settings *s) {
    return form < 2 ? plain[form](ok, st, counts, b, c, p, groups, s) : debug[form - 2](out, ok, st, counts, b, c, p, groups, s);
}

int main(void) {
    const kzg355_settings *h = (const kzg355_settings *)(const void *)opaque;
    size_t counts[4] = {1, 0, 2, 1}, zeros[4] = {0, 0, 0, 0}, big[2], wrap[2];
    bool ok[4];
    int st[4], form, i;
    kzg355_settings *none = 0;
    static uint8_t g1[48 * 4096], g2[96 * 65];
    plain[0] = kzg355_verify_blob_kzg_proof_batch_many_sets; plain[1] = kzg355_verify_blob_kzg_proof_batch_many_sets_device;
    debug[0] = kzg355_debug_batch_intermediates_sets; debug[1] = kzg355_debug_batch_intermediates_sets_device;
    big[0] = (size_t)1 << 24; big[1] = 1;
    wrap[0] = SIZE_MAX; wrap[1] = 2;
#define RESET for (i = 0; i < 4; i++) { ok[i] = true; st[i] = 7; }
    for (form = 0; form < 4; form++) {
        RESET expect(call(form, ok, st, counts, arr, arr, arr, 4, 0) == KZG355_BADARGS && marked(ok, st, 4), "NULL handle");
        RESET expect(call(form, 0, st, counts, arr, arr, arr, 4, h) == KZG355_BADARGS && st[0] == KZG355_BADARGS && st[3] == KZG355_BADARGS, "NULL ok");
        RESET expect(call(form, ok, st, 0, arr, arr, arr, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "NULL blob_counts");
        RESET expect(call(form, ok, st, counts, 0, arr, arr, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "NULL blobs");
        RESET expect(call(form, ok, st, counts, arr, 0, arr, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "NULL commitments");
        RESET expect(call(form, ok, st, counts, arr, arr, 0, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "NULL proofs");
        RESET expect(call(form, ok, st, big, arr, arr, arr, 2, h) == KZG355_BADARGS && marked(ok, st, 2) && st[2] == 7, "sum above 2^24");
        RESET expect(call(form, ok, st, wrap, arr, arr, arr, 2, h) == KZG355_BADARGS && marked(ok, st, 2) && st[2] == 7, "sum that overflows");
        /* groups == 0: OK, nothing touched (not even a NULL counts array or NULL arrays) */
        RESET expect(call(form, ok, st, 0, 0, 0, 0, 0, h) == KZG355_OK && ok[0] && st[0] == 7, "groups == 0");
        /* nothing but empty groups: true / OK on the spot, NULL arrays are fine, no device is touched */
        RESET expect(call(form, ok, st, zeros, 0, 0, 0, 4, h) == KZG355_OK && ok[0] && ok[3] && st[0] == KZG355_OK && st[3] == KZG355_OK, "empty groups");
    }
    for (form = 1; form < 4; form += 2) {            /* the device forms: 16-byte loads of the blobs, 4-byte loads of the points */
        RESET expect(call(form, ok, st, counts, arr + 8, arr, arr, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "d_blobs off 16 bytes");
        RESET expect(call(form, ok, st, counts, arr, arr + 2, arr, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "d_commitments off 4 bytes");
        RESET expect(call(form, ok, st, counts, arr, arr, arr + 1, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "d_proofs off 4 bytes");
    }
    for (form = 0; form < 2; form++) {               /* a debug form without its output */
        RESET expect(debug[form](0, ok, st, counts, arr, arr, arr, 4, h) == KZG355_BADARGS && marked(ok, st, 4), "NULL out");
    }
    {                                                /* more groups than 2^24: refused before the counts are read, every entry marked */
        const size_t many = ((size_t)1 << 24) + 1;
        bool *mok = malloc(many);
        int *mst = malloc(many * sizeof(int));
        memset(mok, 1, many);
        for (form = 0; form < 2; form++) {
            mst[0] = mst[many - 1] = 7; mok[0] = mok[many - 1] = true;
            expect(plain[form](mok, mst, counts, arr, arr, arr, many, h) == KZG355_BADARGS && !mok[0] && !mok[many - 1] && mst[0] == KZG355_BADARGS &&
                   mst[many - 1] == KZG355_BADARGS, "groups above 2^24");
        }
        free(mok); free(mst);
    }
    printf("load %d\n", kzg355_load_trusted_setup(g1, 4096, g2, 65, &none));
    printf("fails %d\n", fails);
    return fails != 0;
}
'''


def test_c11_consumer_and_every_whole_call_refusal(lib, tmp_path):
    """the header with the new declarations compiles as C11 -pedantic; the consumer links against libkzg355.so and gets every whole-call refusal of
    the header's list from all four forms, with nothing but the counts looked at"""
    import torch
    src = tmp_path / "consumer.c"
    src.write_text(CONSUMER)
    exe = tmp_path / "consumer"
    so_dir = os.path.join(ROOT, "kzg_rust_amd")
    cc = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                         "-L" + so_dir, "-lkzg355", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert "FAIL" not in out.stdout and out.returncode == 0 and "fails 0" in out.stdout, out.stdout + out.stderr
    if not torch.cuda.is_available():
        assert "load 6" in out.stdout                            # KZG355_NO_DEVICE: a missing device is an error, never a fallback


def test_python_mirror_refuses_before_any_ffi_call():
    import kzg_rust_amd as kz
    for fn in ("verify_blob_kzg_proof_batch_many_sets", "verify_blob_kzg_proof_batch_many_sets_device", "debug_batch_intermediates_sets",
               "debug_batch_intermediates_sets_device"):
        assert callable(getattr(kz.Kzg, fn)), fn
    assert callable(kz.KzgSettings.blob_sets_blobs_per_device) and callable(kz.KzgSettings.set_blob_sets_max_blobs)

    class Settings:                                               # what the wrappers look at before the call: a wrapper that got as far as the
        field_elements_per_blob = 4096                            # FFI call would fail on the missing handle, not with BadArgs
        handle = None

    class Fake:                                                  # what the wrapper looks at of a tensor
        def __init__(self, numel, dtype="torch.uint8"):
            self._n, self.dtype = numel, dtype
        def numel(self):
            return self._n
        def data_ptr(self):
            return 16

    blob, c48 = bytes(131072), bytes(48)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_blob_kzg_proof_batch_many_sets([([blob], [c48], [])], Settings)                  # kzg.rs:644-651 per group
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_batch_intermediates_sets([([blob, blob], [c48], [c48, c48])], Settings)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.verify_blob_kzg_proof_batch_many_sets([([blob[:-1]], [c48], [c48])], Settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_blob_kzg_proof_batch_many_sets_device(Fake(131072), Fake(48), Fake(48), [-1], Settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_blob_kzg_proof_batch_many_sets_device(Fake(131072), Fake(48), Fake(47), [1], Settings)   # a proofs tensor of the wrong size
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_batch_intermediates_sets_device(Fake(131072), Fake(96), Fake(96), [1, 1], Settings)


CPP_MIRROR = r'''
#include "kzg355.hpp"
#include <iostream>
using namespace kzg355;
int main() {
    KzgSettings none;                                  // no handle: whatever reaches the library is refused there
    Kzg::ProofGroup g;
    g.blobs.push_back(Blob::from_bytes(std::vector<uint8_t>(BYTES_PER_BLOB).data(), BYTES_PER_BLOB).value());
    g.commitments.push_back(KzgCommitment::from_bytes(std::vector<uint8_t>(48).data(), 48).value());
    auto a = Kzg::verify_blob_kzg_proof_batch_many_sets({g}, none);          // one blob, one commitment, no proof
    std::cout << (a.is_err() ? a.error().message : std::string("ok")) << "\n";
    g.proofs.push_back(KzgProof::from_bytes(std::vector<uint8_t>(48).data(), 48).value());
    auto b = Kzg::verify_blob_kzg_proof_batch_many_sets({g}, none);          // lengths fit: the library refuses the NULL handle
    // (a refusal of the whole call marks every group: the mirror hands the marks on, one Err per group)
    std::cout << (b.is_ok() && b.value().size() == 1 && b.value()[0].is_err() ? (int)b.value()[0].error().kind : -1) << "\n";
    auto c = Kzg::verify_blob_kzg_proof_batch_many_sets_device(nullptr, nullptr, nullptr, {1, 2}, none);
    std::cout << (c.is_ok() && c.value().size() == 2 && c.value()[1].is_err() ? (int)c.value()[1].error().kind : -1) << "\n";
    return 0;
}
'''


def test_cpp_mirror_checks_lengths_before_the_library(lib, tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text(CPP_MIRROR)
    exe = tmp_path / "mirror"
    so_dir = os.path.join(ROOT, "kzg_rust_amd")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L" + so_dir, "-lkzg355",
                         "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "length mismatch"
    assert lines[1] == "1" and lines[2] == "1"                    # Error::BadArgs
