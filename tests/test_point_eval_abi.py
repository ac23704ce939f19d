"""-m "not gpu": the point-evaluation precompile at the boundary, on a machine without a GPU.
kzg355_kzg_to_versioned_hash_many is pure host code and is checked against hashlib right here.  The header, the loader and the Rust shim declare
the five calls with the same argument lists.  Every whole-call refusal the header lists is KZG355_BADARGS with every status marked and every ok /
hash_match false, decided from the arguments alone: the C consumer below hands the calls an opaque non-NULL handle that is never a loaded one --
a refusal that came too late would read it, which is why those calls run in a process of their own.  k_pe_unpack and k_versioned_hash use no
scratch, no dynamic stack and no LDS (read from the built code object).  And the host build of the byte layout (csrc/point_eval.h through
tests/native/point_eval_probe.cpp, plain and under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program) gives the match flags
of hashlib and the records of the plain re-ordering of the fields."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import pytest

import point_eval_cases as pc
from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARGS = 1
ARGS = {
    "kzg355_kzg_to_versioned_hash_many": ["out", "commitments", "n"],
    "kzg355_kzg_to_versioned_hash_many_device": ["d_out", "d_commitments", "n", "s"],
    "kzg355_point_evaluation_many": ["ok", "status", "hash_match", "inputs", "n", "s"],
    "kzg355_point_evaluation_many_device": ["ok", "status", "hash_match", "d_inputs", "n", "s"],
    "kzg355_point_evaluation": ["out", "input", "input_len", "s"],
}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    from kzg_rust_amd import _lib
    return _lib.load()


def test_header_loader_and_shim_agree(lib):
    from kzg_rust_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", read("rust", "src", "ffi.rs"))
    assert re.search(r"#define\s+KZG355_BYTES_PER_POINT_EVALUATION_INPUT\s+192\b", hdr)
    for name, want in ARGS.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert [re.sub(r"\[\d+\]", "", a.split()[-1]).lstrip("*") for a in m.group(1).split(",")] == want, name
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want) and fn.restype is C.c_int, name
        r = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", ffi)
        assert r and [a.split(":")[0].strip() for a in r.group(1).split(",")] == want, name
    rust = read("rust", "src", "kzg.rs")
    for fn in ("kzg_to_versioned_hash", "point_evaluation_many", "point_evaluation"):
        assert "pub fn " + fn + "(" in rust, fn
    hpp = read("include", "kzg355.hpp")
    for fn in ("kzg_to_versioned_hash", "point_evaluation_many", "point_evaluation"):
        assert re.search(r"\b" + fn + r"\s*\(", hpp), fn
    import kzg_rust_amd as kz
    for fn in ("kzg_to_versioned_hash", "kzg_to_versioned_hash_many", "kzg_to_versioned_hash_many_device", "point_evaluation_many",
               "point_evaluation_many_device", "point_evaluation"):
        assert callable(getattr(kz.Kzg, fn)), fn


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_versioned_hash_on_the_host_against_hashlib(lib, n):
    """no handle, no device: 0x01 || sha256(C)[1:] per commitment, and nothing behind the n * 32 bytes.  Hashing does not validate: the encoding
    of infinity, 48 bytes that are no point and arbitrary bytes are hashed like any others."""
    special = [bytes([0xC0]) + bytes(47), bytes([0xFF]) * 48]
    cs = [special[i] if i < 2 else hashlib.sha256(b"commitment %d" % i).digest() + bytes([i] * 16) for i in range(n)]
    guard = 0xA5
    out = (C.c_ubyte * (32 * n + 64))(*([guard] * (32 * n + 64)))
    src = b"".join(cs)
    rc = lib.kzg355_kzg_to_versioned_hash_many(C.cast(out, C.c_char_p), src if n else None, n)
    assert rc == 0
    got = bytes(out)
    assert got[32 * n:] == bytes([guard]) * 64
    for i, c in enumerate(cs):
        assert got[32 * i:32 * i + 32] == b"\x01" + hashlib.sha256(c).digest()[1:], i
    if n:
        assert lib.kzg355_kzg_to_versioned_hash_many(None, src, n) == BADARGS
        assert lib.kzg355_kzg_to_versioned_hash_many(C.cast(out, C.c_char_p), None, n) == BADARGS
        import kzg_rust_amd as kz
        assert kz.Kzg.kzg_to_versioned_hash_many(cs) == [pc.vh(c) for c in cs]
        assert kz.Kzg.kzg_to_versioned_hash(kz.KzgCommitment(cs[0])) == pc.vh(cs[0])


def test_null_handle_refuses_every_form(lib):
    n = 3
    buf = C.create_string_buffer(192 * n)
    calls = [lambda ok, st, m: lib.kzg355_point_evaluation_many(ok, st, m, buf, n, None),
             lambda ok, st, m: lib.kzg355_point_evaluation_many_device(ok, st, m, 16, n, None)]
    for call in calls:
        ok, st, m = (C.c_bool * n)(*([True] * n)), (C.c_int * (n + 1))(*([7] * (n + 1))), (C.c_bool * (n + 1))(*([True] * (n + 1)))
        assert call(ok, st, m) == BADARGS
        assert list(ok) == [False] * n and list(st) == [BADARGS] * n + [7] and list(m) == [False] * n + [True]
        ok = (C.c_bool * n)(*([True] * n))
        assert call(ok, None, None) == BADARGS and list(ok) == [False] * n      # NULL status and NULL hash_match are legal
    out = C.create_string_buffer(b"\x5a" * 64, 64)
    assert lib.kzg355_point_evaluation(out, bytes(192), 192, None) == BADARGS and out.raw == b"\x5a" * 64
    assert lib.kzg355_kzg_to_versioned_hash_many_device(16, 16, 1, None) == BADARGS
    # n == 0: KZG355_OK with every pointer NULL
    assert lib.kzg355_point_evaluation_many(None, None, None, None, 0, None) == 0
    assert lib.kzg355_point_evaluation_many_device(None, None, None, None, 0, None) == 0
    assert lib.kzg355_kzg_to_versioned_hash_many(None, None, 0) == 0 and lib.kzg355_kzg_to_versioned_hash_many_device(None, None, 0, None) == 0


CONSUMER = r'''
#include "kzg355.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long long opaque[8192];                       /* never a loaded handle: a refusal decided from the arguments alone does not read it */
static _Alignas(16) uint8_t arr[4 * KZG355_BYTES_PER_POINT_EVALUATION_INPUT + 16];
static int fails = 0;
static void expect(int cond, const char *what) { if (!cond) { fails++; printf("FAIL %s\n", what); } }
/* ok, st and m have a guard entry behind the n the call is told about */
static bool ok[5], m[5];
static int st[5];
static int marked(size_t n) {
    size_t i;
    for (i = 0; i < n; i++) if (ok[i] || m[i] || st[i] != KZG355_BADARGS) return 0;
    return ok[n] && m[n] && st[n] == 7;
}
typedef int (*many_fn)(bool *, int *, bool *, const uint8_t *, size_t, const kzg355_settings *);

int main(void) {
    const kzg355_settings *h = (const kzg355_settings *)(const void *)opaque;
    many_fn many[2];
    int form, i;
    uint8_t out[64 + 8];
    kzg355_settings *none = 0;
    static uint8_t g1[48 * 4096], g2[96 * 65];
    many[0] = kzg355_point_evaluation_many; many[1] = kzg355_point_evaluation_many_device;
#define RESET for (i = 0; i < 5; i++) { ok[i] = true; m[i] = true; st[i] = 7; }
    for (form = 0; form < 2; form++) {
        RESET expect(many[form](ok, st, m, arr, 4, 0) == KZG355_BADARGS && marked(4), "NULL handle");
        RESET expect(many[form](0, st, m, arr, 4, h) == KZG355_BADARGS && st[0] == KZG355_BADARGS && st[3] == KZG355_BADARGS && st[4] == 7 && !m[0] && !m[3] &&
                     m[4], "NULL ok");
        RESET expect(many[form](ok, st, m, 0, 4, h) == KZG355_BADARGS && marked(4), "NULL inputs");
        RESET expect(many[form](ok, 0, 0, arr, 4, 0) == KZG355_BADARGS && !ok[0] && !ok[3] && ok[4] && st[0] == 7 && m[0], "NULL status and hash_match");
        RESET expect(many[form](0, 0, 0, 0, 0, 0) == KZG355_OK && ok[0] && m[0] && st[0] == 7, "n == 0");
        RESET expect(many[form](ok, st, m, arr, 0, h) == KZG355_OK && ok[0] && m[0] && st[0] == 7, "n == 0, nothing touched");
    }
    RESET expect(many[1](ok, st, m, arr + 8, 4, h) == KZG355_BADARGS && marked(4), "d_inputs off 16 bytes");
    RESET expect(many[1](ok, st, m, arr + 4, 2, h) == KZG355_BADARGS && marked(2), "d_inputs off 16 bytes by 4");
    {                                                /* n above 2^24: every entry marked */
        const size_t big = ((size_t)1 << 24) + 1;
        bool *bok = malloc(big + 1), *bm = malloc(big + 1);
        int *bst = malloc((big + 1) * sizeof(int));
        for (form = 0; form < 2; form++) {
            size_t k, bad = 0;
            memset(bok, 1, big + 1); memset(bm, 1, big + 1);
            for (k = 0; k <= big; k++) bst[k] = 7;
            expect(many[form](bok, bst, bm, arr, big, h) == KZG355_BADARGS, "n above 2^24");
            for (k = 0; k < big; k++) bad += bok[k] || bm[k] || bst[k] != KZG355_BADARGS;
            expect(bad == 0 && bok[big] && bm[big] && bst[big] == 7, "n above 2^24: marks");
        }
        free(bok); free(bm); free(bst);
    }
    /* the hash calls have no per-input arrays: BADARGS, nothing written */
    memset(out, 0x5a, sizeof out);
    expect(kzg355_kzg_to_versioned_hash_many_device(arr + 8, arr, 1, h) == KZG355_BADARGS, "d_out off 16 bytes");
    expect(kzg355_kzg_to_versioned_hash_many_device(arr, arr + 2, 1, h) == KZG355_BADARGS, "d_commitments off 4 bytes");
    expect(kzg355_kzg_to_versioned_hash_many_device(0, arr, 1, h) == KZG355_BADARGS, "NULL d_out");
    expect(kzg355_kzg_to_versioned_hash_many_device(arr, 0, 1, h) == KZG355_BADARGS, "NULL d_commitments");
    expect(kzg355_kzg_to_versioned_hash_many_device(arr, arr, ((size_t)1 << 24) + 1, h) == KZG355_BADARGS, "hash n above 2^24");
    expect(kzg355_kzg_to_versioned_hash_many_device(0, 0, 0, 0) == KZG355_OK, "hash n == 0");
    /* the single call: the length rule comes before anything is read */
    expect(kzg355_point_evaluation(out, arr, 191, h) == KZG355_BADARGS, "input_len 191");
    expect(kzg355_point_evaluation(out, arr, 193, h) == KZG355_BADARGS, "input_len 193");
    expect(kzg355_point_evaluation(out, arr, 0, h) == KZG355_BADARGS, "input_len 0");
    expect(kzg355_point_evaluation(out, 0, 192, h) == KZG355_BADARGS, "NULL input");
    expect(kzg355_point_evaluation(0, arr, 192, h) == KZG355_BADARGS, "NULL out");
    expect(kzg355_point_evaluation(out, arr, 192, 0) == KZG355_BADARGS, "NULL handle, single");
    for (i = 0; i < (int)sizeof out; i++) expect(out[i] == 0x5a, "out untouched");
    printf("load %d\n", kzg355_load_trusted_setup(g1, 4096, g2, 65, &none));
    printf("fails %d\n", fails);
    return fails != 0;
}
'''


def test_c11_consumer_and_every_whole_call_refusal(lib, tmp_path):
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

    class Settings:
        field_elements_per_blob = 4096
        handle = None

    with pytest.raises(kz.BadArgs):
        kz.Kzg.point_evaluation(bytes(191), Settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.point_evaluation(bytes(193), Settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.point_evaluation_many([bytes(192), bytes(191)], Settings)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Kzg.kzg_to_versioned_hash_many([bytes(47)])
    assert kz.Kzg.point_evaluation_many([], Settings) == ([], [])
    assert kz.Kzg.kzg_to_versioned_hash_many([]) == []


def test_the_kernels_use_no_scratch_and_no_lds(tmp_path):
    res = kernel_resources(tmp_path, "k_point_eval")
    found = {}
    for short in ("k_pe_unpack", "k_versioned_hash"):
        hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
        assert len(hits) == 1, (short, sorted(res))
        found[short] = res[hits[0]]
        print(short, found[short])
    assert len(res) == 2, sorted(res)
    for short, r in found.items():
        assert r["scratch"] == 0 and not r["dynamic_stack"] and r["lds"] == 0, (short, r)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_host_build_of_the_layout_against_hashlib(tmp_path, flags):
    """csrc/point_eval.h is the one place the byte layout is written; the kernel calls it with the device rounds, this program with sha256_block"""
    exe = tmp_path / "point_eval_probe"
    cc = subprocess.run(["g++", "-O1", "-std=c++17"] + flags + ["-o", str(exe), os.path.join(ROOT, "tests", "native", "point_eval_probe.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    cases = tmp_path / "cases.bin"
    cases.write_bytes(pc.pack(pc.CASES))
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.split()
    assert len(lines) == 3 * len(pc.CASES)
    for i, c in enumerate(pc.CASES):
        h, z, y, commitment, proof = pc.fields(c.data)
        good = b"\x01" + hashlib.sha256(commitment).digest()[1:]
        assert lines[3 * i] == ("1" if h == good else "0") and (h == good) == c.match, c.name
        assert bytes.fromhex(lines[3 * i + 1]) == commitment + z + y + proof, c.name
        assert bytes.fromhex(lines[3 * i + 2]) == good, c.name
