"""-m "not gpu": the six calls that return the blobs' commitments out of the FK20 chain, at the boundary.  include/kzg355.h declares them, the
built library exports them, the ctypes loader and the Rust shim bind them with the same argument lists, a C11 -pedantic consumer and the C++
mirror compile, and every refusal that needs no device is KZG355_BADARGS with every status marked.

Without a GPU no handle exists (the load itself is KZG355_NO_DEVICE, which the C consumer below checks), and the entry points test the handle
first, so a call can only be reached here with a NULL handle: that is BADARGS, never NO_DEVICE, exactly as for the calls they extend
(test_cell_device_abi.py says the same of those).  All three outputs NULL is refused at the same place, before any device work; that check is
told apart from the others with a real handle in test_gpu_cell_commitments.py.

k_cc_proofs in the built code object (the method of test_cell_kernel_resources.py): the commitment output costs no scratch and no LDS.  The
build before this output existed had 182 VGPRs, 21504 bytes of LDS (128 Jacobian points) and 2496 bytes of scratch; this build has the same
three figures."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cell_kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARGS, NO_DEVICE = 1, 6
ARGS = {
    "kzg355_compute_commitments_cells_and_kzg_proofs_many": ["commitments_out", "cells_out", "proofs_out", "status", "blobs", "n", "s"],
    "kzg355_compute_commitments_cells_and_kzg_proofs_many_device":
        ["d_commitments_out", "d_cells_out", "d_proofs_out", "status", "d_blobs", "n", "s"],
    "kzg355_recover_commitments_cells_and_kzg_proofs_many":
        ["commitments_out", "cells_out", "proofs_out", "status", "cell_indices", "cells", "n", "m", "s"],
    "kzg355_recover_commitments_cells_and_kzg_proofs_many_device":
        ["d_commitments_out", "d_cells_out", "d_proofs_out", "status", "cell_indices", "d_cells", "n", "m", "s"],
    "kzg355_recover_commitments_cells_and_kzg_proofs_many_sets":
        ["commitments_out", "cells_out", "proofs_out", "status", "cell_counts", "cell_indices", "cells", "m", "s"],
    "kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device":
        ["d_commitments_out", "d_cells_out", "d_proofs_out", "status", "cell_counts", "cell_indices", "d_cells", "m", "s"],
}
PARENT_K_CC_PROOFS = {"lds": 21504, "scratch": 2496}            # the build before the commitment output (its VGPR count: 182)


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
    assert "global: kzg355_*;" in read("kzg_rust_amd", "csrc", "exports.map")
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, want in ARGS.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
        old = re.search(r"int\s+" + name.replace("_commitments", "") + r"\s*\(([^)]*)\)\s*;", hdr)
        # the existing signature with the commitments in front
        assert [" ".join(a.split()) for a in m.group(1).split(",")][1:] == [" ".join(a.split()) for a in old.group(1).split(",")], name
        assert re.fullmatch(r"uint8_t \*(d_)?commitments_out", m.group(1).split(",")[0].strip())
        r = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", ffi)
        assert r and [a.split(":")[0].strip() for a in r.group(1).split(",")] == want, name
        assert name in exported and name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want) and fn.restype is C.c_int, name
        assert fn.argtypes[3] == C.POINTER(C.c_int), name                                   # status
    rust = read("rust", "src", "kzg.rs")
    for fn in ("compute_commitment_cells_and_kzg_proofs", "compute_commitment_cells_and_kzg_proofs_many", "recover_commitment_cells_and_kzg_proofs",
               "recover_commitment_cells_and_kzg_proofs_many", "recover_commitment_cells_and_kzg_proofs_many_sets"):
        assert "pub fn " + fn + "(" in rust, fn
    for fn in ("compute_commitment_cells_and_kzg_proofs_many_device", "recover_commitment_cells_and_kzg_proofs_many_device",
               "recover_commitment_cells_and_kzg_proofs_many_sets_device"):
        assert "pub unsafe fn " + fn + "(" in rust, fn
    for name in ARGS:
        assert "ffi::" + name + "(" in rust, name


def test_python_mirror_has_the_methods_and_refuses_before_any_ffi_call():
    import kzg_rust_amd as kz
    for fn in ("compute_commitment_cells_and_kzg_proofs", "compute_commitment_cells_and_kzg_proofs_many",
               "compute_commitment_cells_and_kzg_proofs_many_device", "recover_commitment_cells_and_kzg_proofs",
               "recover_commitment_cells_and_kzg_proofs_many", "recover_commitment_cells_and_kzg_proofs_many_sets",
               "recover_commitment_cells_and_kzg_proofs_many_device", "recover_commitment_cells_and_kzg_proofs_many_sets_device"):
        assert callable(getattr(kz.Kzg, fn)), fn

    class Fake:                                                  # what the wrapper looks at of a tensor
        def __init__(self, numel, dtype="torch.uint8"):
            self._n, self.dtype = numel, dtype
        def numel(self):
            return self._n
        def data_ptr(self):
            return 16

    # (the settings argument is None: a wrapper that got as far as the FFI call would fail on its handle, not with BadArgs)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_commitment_cells_and_kzg_proofs_many_device(Fake(131072), 1, None)                                 # no output at all
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_commitment_cells_and_kzg_proofs_many_device(Fake(131072), 1, None, commitments_out=Fake(47))
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_device(list(range(64)), Fake(2048 * 64), 1, None, commitments_out=Fake(48, "torch.int8"))
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_sets_device([64], list(range(64)), Fake(2048 * 64), None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_commitment_cells_and_kzg_proofs(list(range(64)), [bytes(2048)] * 63, None)                         # length mismatch
    with pytest.raises(kz.BadArgs):
        kz.Kzg._compute_commitments_cells([bytes(131072)], None, False, False, False)


def test_refusals_that_need_no_device_mark_every_status(lib):
    m = 4
    idx = (C.c_size_t * 64)(*range(64))
    counts = (C.c_size_t * m)(*([16] * m))
    sets_idx = (C.c_size_t * 64)(*(list(range(16)) * 4))
    host = C.create_string_buffer(64)
    calls = [lambda k, c, p, st: lib.kzg355_compute_commitments_cells_and_kzg_proofs_many(k, c, p, st, host, m, None),
             lambda k, c, p, st: lib.kzg355_recover_commitments_cells_and_kzg_proofs_many(k, c, p, st, idx, host, 64, m, None),
             lambda k, c, p, st: lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(k, c, p, st, counts, sets_idx, host, m, None)]
    for call in calls:
        for outs in ((None, None, None), (host, None, None), (None, host, None), (host, host, host)):
            st = (C.c_int * m)(*([7] * m))
            assert call(*outs, st) == BADARGS and list(st) == [BADARGS] * m
            assert call(*outs, None) == BADARGS                                             # a NULL status array is legal
    dcalls = [lambda k, c, p, st: lib.kzg355_compute_commitments_cells_and_kzg_proofs_many_device(k, c, p, st, 16, m, None),
              lambda k, c, p, st: lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_device(k, c, p, st, idx, 16, 64, m, None),
              lambda k, c, p, st: lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(k, c, p, st, counts, sets_idx, 16, m, None)]
    for call in dcalls:
        for outs in ((None, None, None), (16, None, None), (24, 16, 16), (16, 16, 16)):    # (24: a commitments pointer off a 16-byte boundary)
            st = (C.c_int * m)(*([7] * m))
            assert call(*outs, st) == BADARGS and list(st) == [BADARGS] * m


def test_c11_consumer_names_the_six_symbols(lib, tmp_path):
    """include/kzg355.h with the six declarations compiles as C11 -pedantic, a C program that calls all six links against libkzg355.so, gets
    BADARGS with every status marked from each for a NULL handle, and -- without a GPU -- NO_DEVICE from the load, never a fallback."""
    import torch
    src = tmp_path / "consumer.c"
    src.write_text('#include "kzg355.h"\n#include <stdio.h>\n'
                   'static int marked(const int *st) { return st[0] == KZG355_BADARGS && st[1] == KZG355_BADARGS; }\n'
                   'int main(void) {\n'
                   '    static unsigned char g1[48 * 4096], g2[96 * 65], k[96], buf[64];\n'
                   '    size_t idx[64], counts[2] = {64, 64};\n'
                   '    int st[2], bad = 0, i;\n'
                   '    kzg355_settings *s = 0;\n'
                   '    for (i = 0; i < 64; i++) idx[i] = (size_t)i;\n'
                   '    st[0] = st[1] = 7; bad += kzg355_compute_commitments_cells_and_kzg_proofs_many(k, 0, 0, st, buf, 2, s) != KZG355_BADARGS || !marked(st);\n'
                   '    st[0] = st[1] = 7; bad += kzg355_compute_commitments_cells_and_kzg_proofs_many_device(k, 0, 0, st, buf, 2, s) != KZG355_BADARGS || !marked(st);\n'
                   '    st[0] = st[1] = 7; bad += kzg355_recover_commitments_cells_and_kzg_proofs_many(k, 0, 0, st, idx, buf, 64, 2, s) != KZG355_BADARGS || !marked(st);\n'
                   '    st[0] = st[1] = 7; bad += kzg355_recover_commitments_cells_and_kzg_proofs_many_device(k, 0, 0, st, idx, buf, 64, 2, s) != KZG355_BADARGS || !marked(st);\n'
                   '    st[0] = st[1] = 7; bad += kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(k, 0, 0, st, counts, idx, buf, 2, s) != KZG355_BADARGS || !marked(st);\n'
                   '    st[0] = st[1] = 7; bad += kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(k, 0, 0, st, counts, idx, buf, 2, s) != KZG355_BADARGS || !marked(st);\n'
                   '    printf("%d|%d\\n", bad, kzg355_load_trusted_setup(g1, 4096, g2, 65, &s));\n'
                   '    return bad;\n'
                   '}\n')
    exe = tmp_path / "consumer"
    so_dir = os.path.join(ROOT, "kzg_rust_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + so_dir, "-lkzg355", "-Wl,-rpath," + so_dir], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    bad, rc = r.stdout.strip().split("|")
    assert int(bad) == 0 and int(rc) != 0                            # (all-zero bytes are no valid setup points)
    if not torch.cuda.is_available():
        assert int(rc) == NO_DEVICE, rc


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "kzg355.hpp"\n'
                   "int probe(const kzg355::KzgSettings &s, const kzg355::Blob &blob, const std::vector<kzg355::Cell> &cells) {\n"
                   "    using K = kzg355::Kzg;\n"
                   "    auto a = K::compute_commitment_cells_and_kzg_proofs(blob, s);\n"
                   "    auto b = K::compute_commitment_cells_and_kzg_proofs_many({blob, blob}, s);\n"
                   "    auto c = K::recover_commitment_cells_and_kzg_proofs({0, 1}, cells, s);\n"
                   "    auto d = K::recover_commitment_cells_and_kzg_proofs_many({0, 1}, cells, 1, s);\n"
                   "    auto e = K::recover_commitment_cells_and_kzg_proofs_many_sets({K::RecoverUnit{{0, 1}, cells}}, s);\n"
                   "    auto f = K::compute_commitment_cells_and_kzg_proofs_many_device(nullptr, nullptr, nullptr, nullptr, 0, s);\n"
                   "    auto g = K::recover_commitment_cells_and_kzg_proofs_many_device(nullptr, nullptr, nullptr, {}, nullptr, 0, s);\n"
                   "    auto h = K::recover_commitment_cells_and_kzg_proofs_many_sets_device(nullptr, nullptr, nullptr, {}, {}, nullptr, s);\n"
                   "    const kzg355::KzgCommitment &k = a.value().commitment;\n"
                   "    return a.is_ok() + b.is_ok() + c.is_ok() + d.is_ok() + e.is_ok() + f.is_ok() + g.is_ok() + h.is_ok() + (int)k.bytes.size()\n"
                   "           + (int)b.value()[0].value().cells.size() + (int)c.value().proofs.size();\n}\n")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_k_cc_proofs_resources(tmp_path):
    res = kernel_resources(tmp_path, "k_cell_compute")
    hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+k_cc_proofsE.*", k)]
    assert len(hits) == 1, sorted(res)
    r = res[hits[0]]
    print("k_cc_proofs", r)                                          # (the VGPR count is recorded in this file's docstring: 182)
    assert hits[0].endswith("EPhS6_S6_"), hits[0]                    # three byte outputs: proofs, H, commitments
    assert r["scratch"] <= PARENT_K_CC_PROOFS["scratch"] and not r["dynamic_stack"], r
    assert r["lds"] == PARENT_K_CC_PROOFS["lds"] == 128 * 3 * 56, r  # 128 Jacobian points: three Fp of 14 words
    assert 0 < r["vgprs"] <= 256, r
