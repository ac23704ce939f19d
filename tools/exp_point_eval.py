#!/usr/bin/env python3
"""What the front of the point-evaluation precompile costs (the point-evaluation section), measured against another build of the
library on one card.

The driver starts one child process per build, the two builds alternating (--rounds times each), so that neither side owns the warmer or the
cooler part of the job.  A child loads its library with plain ctypes (an older build lacks the new entry points, so the package's loader cannot
bind it), makes a default handle, puts n = --n valid inputs (the true verify_kzg_proof vectors of tests/golden/vectors.json, tiled) into HBM
both as 192-byte precompile inputs and as the pre-packed 160-byte records C | z | y | proof, and times the synchronous C entry points:
  * records:     kzg355_verify_kzg_proof_many_device on the records (both builds) -- the yardstick that existed before, all n in one launch set;
  * point_eval:  kzg355_point_evaluation_many_device on the inputs (builds that have it): hash, compare, re-pack, then the same chain in sets.
Per variant: ms per call as median, min and max of --reps timed calls after --warmup; for point_eval also the `pe_unpack` family of one more
call with the library's event timing on.  Every verdict must be true.  The shader clock is sampled from the card's hwmon files over the child's
run (best effort).  One JSON line per (build, round), then a summary line per build over the rounds.
Run:  python tools/exp_point_eval.py --other /path/to/other/libkzg355.so [--rounds 2] [--reps 7] [--warmup 2] [--n 131072]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    import torch                        # before the library, so that both bind one HIP runtime
    sys.path.insert(0, ROOT)
    from bench import PowerSampler
    lib = C.CDLL(a.child)
    vp, sz, u8p, ip, bp = C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_bool)
    lib.kzg355_load_trusted_setup.argtypes = [u8p, sz, u8p, sz, C.POINTER(vp)]
    lib.kzg355_free_trusted_setup.argtypes = [vp]
    lib.kzg355_free_trusted_setup.restype = None
    lib.kzg355_verify_kzg_proof_many_device.argtypes = [bp, ip, vp, sz, vp]
    lib.kzg355_set_kernel_timing.argtypes = [vp, C.c_int]
    lib.kzg355_set_kernel_timing.restype = None
    lib.kzg355_reset_kernel_stats.argtypes = [vp]
    lib.kzg355_reset_kernel_stats.restype = None
    lib.kzg355_kernel_ms_stats.argtypes = [vp, u8p, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    lib.kzg355_settings_device.argtypes = [vp]
    new = hasattr(lib, "kzg355_point_evaluation_many_device")
    if new:
        lib.kzg355_point_evaluation_many_device.argtypes = [bp, ip, bp, vp, sz, vp]
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    h = vp()
    assert lib.kzg355_load_trusted_setup(g1, 4096, g2, 65, C.byref(h)) == 0
    vectors = json.load(open(os.path.join(g, "vectors.json")))["functions"]["verify_kzg_proof"]
    unhex = lambda s: bytes.fromhex(s[2:] if s.startswith("0x") else s)      # noqa: E731
    true = [tuple(unhex(v["input"][k]) for k in ("commitment", "z", "y", "proof")) for v in vectors if v["output"] is True]
    n = a.n
    inputs = b"".join(b"\x01" + hashlib.sha256(c).digest()[1:] + z + y + c + p for c, z, y, p in true)
    records = b"".join(c + z + y + p for c, z, y, p in true)
    reps = n // len(true) + 1
    dev = torch.device("cuda", lib.kzg355_settings_device(h))
    d_in = torch.frombuffer(bytearray((inputs * reps)[:192 * n]), dtype=torch.uint8).to(dev)
    d_rec = torch.frombuffer(bytearray((records * reps)[:160 * n]), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    ok, st, match = (C.c_bool * n)(), (C.c_int * n)(), (C.c_bool * n)()

    def run_records():
        assert lib.kzg355_verify_kzg_proof_many_device(ok, st, d_rec.data_ptr(), n, h) == 0

    def run_point_eval():
        assert lib.kzg355_point_evaluation_many_device(ok, st, match, d_in.data_ptr(), n, h) == 0

    variants = {"records": run_records}
    if new:
        variants["point_eval"] = run_point_eval
    sampler = PowerSampler(dev.index or 0)
    sampler.start()
    row = {"build": a.label, "round": a.round, "n": n}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t))
        assert all(ok) and (name == "records" or all(match)), name
        row[name] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}
        if name == "point_eval":
            lib.kzg355_set_kernel_timing(h, 1)
            lib.kzg355_reset_kernel_stats(h)
            fn()
            total, launches = C.c_double(), C.c_long()
            lib.kzg355_kernel_ms_stats(h, b"pe_unpack", C.byref(total), C.byref(launches))
            lib.kzg355_set_kernel_timing(h, 0)
            row[name]["pe_unpack_ms"] = round(total.value, 4)
            row[name]["pe_unpack_launches"] = launches.value
    clk = sampler.stop()
    row["sclk_mhz"] = clk and clk["sclk_mhz"]
    print(json.dumps(row), flush=True)
    lib.kzg355_free_trusted_setup(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the build to compare with (libkzg355.so of the parent commit)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--child")
    ap.add_argument("--label")
    ap.add_argument("--round", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    builds = ([("other", a.other)] if a.other else []) + [("this", os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so"))]
    rows = []
    for r in range(a.rounds):
        for label, lib in builds:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--label", label, "--round", str(r), "--reps", str(a.reps),
                                  "--warmup", str(a.warmup), "--n", str(a.n)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                print(out.stdout, out.stderr, sep="\n", flush=True)
                return 1                                            # nothing more is started after a failed child
            for ln in out.stdout.splitlines():
                print(ln, flush=True)
                rows.append(json.loads(ln))
    for label, _ in builds:
        mine = [r for r in rows if r["build"] == label]
        line = {"summary": label, "n": a.n}
        for v in ("records", "point_eval"):
            if mine and all(v in r for r in mine):
                line[v] = {"ms_median": round(statistics.median(r[v]["ms_median"] for r in mine), 3), "ms_min": min(r[v]["ms_min"] for r in mine),
                           "ms_max": max(r[v]["ms_max"] for r in mine)}
                if v == "point_eval":
                    line[v]["pe_unpack_ms"] = round(statistics.median(r[v]["pe_unpack_ms"] for r in mine), 4)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
