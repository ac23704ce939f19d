"""-m "not gpu": kzg355_settings_cell_calls_per_device at the boundary.  include/kzg355.h declares it, the built library exports it, the ctypes
loader and the Rust shim bind it with the same argument list, the Python, C++ and Rust mirrors have their accessor, and what it refuses without a
device (a NULL handle) is KZG355_BADARGS.  What it counts needs a GPU: tests/test_gpu_cell_multi_device.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kzg355_settings_cell_calls_per_device"
BADARGS = 1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_library_loader_and_shim_agree():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "kzg355.h"), flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, "not declared in include/kzg355.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ["const kzg355_settings *s", "long *out", "size_t cap"]
    ffi = re.sub(r"//[^\n]*", "", read("rust", "src", "ffi.rs"))
    r = re.search(r"pub fn " + NAME + r"\s*\(([^)]*)\)\s*->\s*c_int\s*;", ffi)
    assert r and [" ".join(a.split()) for a in r.group(1).split(",")] == ["s: *const kzg355_settings", "out: *mut c_long", "cap: usize"]
    so = os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NAME in _lib.EXPORTED_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_long), C.c_size_t] and fn.restype is C.c_int


def test_the_mirrors_have_their_accessor(tmp_path):
    from kzg_rust_amd import kzg
    assert callable(kzg.KzgSettings.cell_calls_per_device)
    rust = read("rust", "src", "kzg.rs")
    assert "pub fn cell_calls_per_device(&self)" in rust and "ffi::" + NAME + "(" in rust
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "kzg355.hpp"\n'
                   "long probe(const kzg355::KzgSettings &s) { std::vector<long> v = s.cell_calls_per_device(); return (long)v.size(); }\n")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_a_null_handle_is_badargs():
    from kzg_rust_amd import _lib
    lib = _lib.load()
    out = (C.c_long * 4)(7, 7, 7, 7)
    assert lib.kzg355_settings_cell_calls_per_device(None, out, 4) == BADARGS
    assert lib.kzg355_settings_cell_calls_per_device(None, None, 0) == BADARGS
    assert list(out) == [7, 7, 7, 7]
