"""-m "not gpu": the device-resident cell calls at the boundary.  include/kzg355.h declares the five entry points, the built library exports
them, the ctypes loader and the Rust shim bind them with the same argument lists, the C++ mirror compiles, and every refusal that needs no
device (a NULL handle, both outputs NULL, n outside 64..128, indices not ascending, misaligned pointers) is KZG355_BADARGS with every status
marked.  It also checks, without a GPU, that the generator of the GPU file's differential fuzz draws what it says it draws."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cell_device_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARGS = 1
ARGS = {
    "kzg355_verify_cell_kzg_proof_batch_many_device":
        ["ok", "status", "d_commitments", "d_cell_indices", "d_cells", "d_proofs", "n_per_group", "groups", "s"],
    "kzg355_compute_cells_and_kzg_proofs_many_device": ["d_cells_out", "d_proofs_out", "status", "d_blobs", "n", "s"],
    "kzg355_recover_cells_and_kzg_proofs_many_device": ["d_cells_out", "d_proofs_out", "status", "cell_indices", "d_cells", "n", "m", "s"],
    "kzg355_debug_cell_batch_intermediates_device":
        ["out", "ok", "status", "d_commitments", "d_cell_indices", "d_cells", "d_proofs", "n_per_group", "groups", "prep_form", "s"],
    "kzg355_settings_cell_device_prep_calls": ["s"],
}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    from kzg_rust_amd import _lib
    return _lib.load()


def test_header_loader_and_shim_agree_on_the_argument_lists(lib):
    from kzg_rust_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", read("rust", "src", "ffi.rs"))
    assert "global: kzg355_*;" in read("kzg_rust_amd", "csrc", "exports.map")
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, want in ARGS.items():
        m = re.search(r"(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert (m.group(1) == "long") == name.endswith("_calls")
        assert [a.split()[-1].lstrip("*") for a in m.group(2).split(",")] == want, name
        r = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", ffi)
        assert r and [a.split(":")[0].strip() for a in r.group(1).split(",")] == want, name
        assert name in exported and name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == len(want), name
    # device cell indices are size_t on every side, as in the host form
    assert re.search(r"const size_t \*d_cell_indices", hdr) and "d_cell_indices: *const usize" in ffi
    rust = read("rust", "src", "kzg.rs")
    for fn in ("verify_cell_kzg_proof_batch_many_device", "compute_cells_and_kzg_proofs_many_device", "recover_cells_and_kzg_proofs_many_device"):
        assert "pub unsafe fn " + fn + "(" in rust and "ffi::kzg355_" + fn + "(" in rust


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "kzg355.hpp"\n'
                   "int probe(const kzg355::KzgSettings &s) {\n"
                   "    auto a = kzg355::Kzg::verify_cell_kzg_proof_batch_many_device(nullptr, nullptr, nullptr, nullptr, 0, 0, s);\n"
                   "    auto b = kzg355::Kzg::compute_cells_and_kzg_proofs_many_device(nullptr, nullptr, nullptr, 0, s);\n"
                   "    auto c = kzg355::Kzg::recover_cells_and_kzg_proofs_many_device(nullptr, nullptr, {}, nullptr, 0, s);\n"
                   "    return a.is_ok() + b.is_ok() + c.is_ok();\n}\n")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_a_null_handle_is_badargs(lib):
    G = 3
    ok, st, dbg = (C.c_bool * G)(), (C.c_int * G)(), C.create_string_buffer(176 * G)
    assert lib.kzg355_verify_cell_kzg_proof_batch_many_device(ok, st, 16, 16, 16, 16, 1, G, None) == BADARGS
    assert lib.kzg355_debug_cell_batch_intermediates_device(dbg, ok, st, 16, 16, 16, 16, 1, G, 1, None) == BADARGS
    st = (C.c_int * G)(7, 7, 7)
    assert lib.kzg355_compute_cells_and_kzg_proofs_many_device(16, 16, st, 16, G, None) == BADARGS and list(st) == [BADARGS] * G
    st = (C.c_int * G)(7, 7, 7)
    idx = (C.c_size_t * 64)(*range(64))
    assert lib.kzg355_recover_cells_and_kzg_proofs_many_device(16, 16, st, idx, 16, 64, G, None) == BADARGS and list(st) == [BADARGS] * G
    assert lib.kzg355_settings_cell_device_prep_calls(None) == 0


def test_refusals_that_need_no_device_mark_every_status(lib):
    """tests/test_recover_abi.py's companion for the device form, and no more than that: what it pins is that a call refused before any device
    work writes the code into the status of EVERY unit.  It cannot tell the argument checks apart: without a device no handle exists (any
    non-null address would be dereferenced), a NULL handle is itself BADARGS, and the entry points test it first, so every case below leaves by
    that one branch.  The checks themselves (alignment, n outside 64..128, the order of the indices, both outputs NULL) are covered with a real
    handle, against the host form, by test_gpu_cell_device.py::test_recover_refusals_match_the_host_form and
    ::test_compute_statuses_and_refusals."""
    m = 4
    asc = list(range(64))
    for out_c, out_p, ix, d_cells in ((None, None, asc, 16),                       # both outputs NULL
                                      (16, None, list(range(63)), 16),             # n outside 64..128
                                      (16, None, list(range(129)), 16),
                                      (16, None, asc[::-1], 16),                   # not ascending
                                      (16, None, [0] + asc[:-1], 16),              # a duplicate
                                      (16, None, asc[:-1] + [128], 16),            # an index >= 128
                                      (24, None, asc, 16), (16, 8, asc, 16), (16, None, asc, 17)):   # misaligned
        st = (C.c_int * m)(*([7] * m))
        idx = (C.c_size_t * len(ix))(*ix)
        assert lib.kzg355_recover_cells_and_kzg_proofs_many_device(out_c, out_p, st, idx, d_cells, len(ix), m, None) == BADARGS
        assert list(st) == [BADARGS] * m
    for out_c, out_p, blobs in ((None, None, 16), (8, None, 16), (16, 4, 16), (16, None, 3)):
        st = (C.c_int * m)(*([7] * m))
        assert lib.kzg355_compute_cells_and_kzg_proofs_many_device(out_c, out_p, st, blobs, m, None) == BADARGS
        assert list(st) == [BADARGS] * m


def test_python_wrapper_refuses_before_any_ffi_call():
    import kzg_rust_amd as kz

    class Fake:                                                  # what the wrapper looks at of a tensor
        def __init__(self, numel, dtype="torch.uint8"):
            self._n, self.dtype = numel, dtype
        def numel(self):
            return self._n
        def data_ptr(self):
            return 16

    # (the settings argument is None: a wrapper that got as far as the FFI call would fail on its handle, not with BadArgs)
    V = kz.Kzg.verify_cell_kzg_proof_batch_many_device
    good = lambda: (Fake(48 * 6), Fake(6, "torch.int64"), Fake(2048 * 6), Fake(48 * 6))
    for k, bad in ((0, Fake(48 * 5)), (1, Fake(6, "torch.int32")), (1, Fake(5, "torch.int64")), (2, Fake(2048 * 6, "torch.float32")), (3, object())):
        args = list(good()); args[k] = bad
        with pytest.raises(kz.BadArgs):
            V(*args, 3, 2, None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells_and_kzg_proofs_many_device(Fake(131072), 1, None)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells_and_kzg_proofs_many_device(Fake(131072), 1, None, cells_out=Fake(128 * 2048 - 1))
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_many_device(list(range(64)), Fake(2048 * 63), 1, None, cells_out=Fake(128 * 2048))
    assert "import torch" not in read("kzg_rust_amd", "kzg.py")


def test_fuzz_generator_draws_what_it_says(oracle):
    fx = cases.fixture()
    shapes = cases.fuzz_groups(fx, cases.not_in_subgroup(oracle))
    assert [npg for npg, _ in shapes] == [1, 2, 6, 16, 64, 128] and sum(len(g) for _, g in shapes) >= 200
    kinds, dup = set(), 0
    for npg, groups in shapes:
        for grp, kind in groups:
            assert all(len(x) == npg for x in grp)
            assert cases.well_formed(oracle, grp) == (kind != "malformed"), (npg, kind)
            kinds.add(kind)
            dup += len(set(grp[0])) < npg
    assert kinds == {"valid", "tampered", "malformed"} and dup >= 50
