"""-m "not gpu": what the gfx950 build of k_cells.hip says about the kernels behind a cell batch cut over several devices.
k_cell_merge and the k_cell_rpowers that takes a first exponent must use no scratch (private memory) at all; k_cell_finish shares its body with
k_cell_merge and is held to the same.  The figures are read from the code object inside the object file the build left behind (its AMDGPU
metadata: .private_segment_fixed_size, .vgpr_count, .group_segment_fixed_size), so nothing is compiled again; without that object file the
test builds it.  One wave adds the blocks in k_cell_merge, so its LDS is 64 + 3 points."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_rust_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernel_resources(tmp_path, name):
    obj = os.path.join(CSRC, name + ".o")
    if not os.path.exists(obj):
        subprocess.run(["make", "-C", CSRC, name + ".o"], check=True, capture_output=True)
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "device.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co], check=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for entry in re.split(r"\n\s*- \.", notes):                   # one YAML map per kernel
        m = re.search(r"\.?name:\s+(\S+)", entry)
        if not m or ".private_segment_fixed_size" not in "." + entry:
            continue
        get = lambda key: int(re.search(r"\.?" + key + r":\s+(\d+)", entry).group(1))      # noqa: E731
        out[m.group(1)] = {"vgprs": get("vgpr_count"), "lds": get("group_segment_fixed_size"), "scratch": get("private_segment_fixed_size"),
                           "dynamic_stack": bool(re.search(r"uses_dynamic_stack:\s+true", entry))}
    return out


def test_merge_rpowers_and_finish_use_no_scratch(tmp_path):
    res = kernel_resources(tmp_path, "k_cells")
    found = {}
    for short in ("k_cell_merge", "k_cell_rpowers", "k_cell_finish"):
        hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
        assert len(hits) == 1, (short, sorted(res))
        found[short] = res[hits[0]]
        print(short, found[short])
    for short, r in found.items():
        assert r["scratch"] == 0 and not r["dynamic_stack"], (short, r)
    assert found["k_cell_rpowers"]["lds"] == 0
    assert found["k_cell_merge"]["lds"] == (64 + 3) * 3 * 56, found["k_cell_merge"]      # G1Jac: three Fp of 14 words
