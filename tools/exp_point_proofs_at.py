#!/usr/bin/env python3
"""What openings at chosen points cost, measured against the one-blob-per-opening call of another build on one card.

The driver starts one child process per build, the two builds alternating (--rounds times each), so that neither side owns the warmer or the
cooler part of the job.  A child loads its library with plain ctypes (an older build lacks the new entry points, so the package's loader cannot
bind it), makes a default handle (wide MSM table, built before anything is timed) and times, at every shape of --shapes (blobs x points, the
points seeded random ones or, with the suffix d, the first points of the domain in blob order), with preallocated buffers around the
synchronous C entry point:
  * yardstick:  kzg355_compute_kzg_proof_many on the same (blob, z) pairs with the blobs duplicated (the --other build; this build too);
  * host:       kzg355_compute_kzg_proofs_at_many, proofs and ys (builds that have it);
  * ys_only:    the same call without proofs_out;
  * device:     kzg355_compute_kzg_proofs_at_many_device on resident blobs, outputs resident.
Per variant: ms per call as median, min and max of --reps timed calls after --warmup, openings per second from the median, and the kernel
families of one more call with the library's event timing on.  A yardstick whose warm-up call takes longer than --slow-ms is reported by
that one call alone (the all-in-domain shape walks its points serially in the old call).  The new call's bytes are checked against the
yardstick's.  One JSON line per (build, round, shape) with the shader clock sampled over the child, then a summary per (build, shape).
Run:  python tools/exp_point_proofs_at.py --other /path/to/other/libkzg355.so [--rounds 1] [--reps 5] [--warmup 1] [--shapes 1x1,1x64,1x4096d,1x4096,64x64]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOB = 131072
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FAMILIES = ["cc_field", "pq_quotient", "msm_wide", "msm_finalize", "quotient"]


def parse_shape(text):
    domain = text.endswith("d")
    n, k = (int(v) for v in text.rstrip("d").split("x"))
    return n, k, domain


def points(n, k, domain):
    if domain:
        root = pow(7, (R - 1) // 4096, R)
        rev = lambda i: int(format(i, "012b")[::-1], 2)      # noqa: E731
        one = [pow(root, rev(j), R).to_bytes(32, "big") for j in range(k)]
        return [one] * n
    rng = random.Random(19 * n + k)
    return [[rng.randrange(R).to_bytes(32, "big") for _ in range(k)] for _ in range(n)]


def child(a):
    import torch                        # before the library, so that both bind one HIP runtime
    sys.path.insert(0, ROOT)
    from bench import PowerSampler
    lib = C.CDLL(a.child)
    vp, sz, u8p, ip, szp = C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_size_t)
    lib.kzg355_load_trusted_setup.argtypes = [u8p, sz, u8p, sz, C.POINTER(vp)]
    lib.kzg355_free_trusted_setup.argtypes = [vp]
    lib.kzg355_free_trusted_setup.restype = None
    lib.kzg355_settings_build_msm_table.argtypes = [vp]
    lib.kzg355_settings_device.argtypes = [vp]
    lib.kzg355_compute_kzg_proof_many.argtypes = [u8p, u8p, ip, u8p, u8p, sz, vp]
    lib.kzg355_set_kernel_timing.argtypes = [vp, C.c_int]
    lib.kzg355_set_kernel_timing.restype = None
    lib.kzg355_reset_kernel_stats.argtypes = [vp]
    lib.kzg355_reset_kernel_stats.restype = None
    lib.kzg355_kernel_ms_stats.argtypes = [vp, u8p, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    new = hasattr(lib, "kzg355_compute_kzg_proofs_at_many")
    if new:
        lib.kzg355_compute_kzg_proofs_at_many.argtypes = [u8p, u8p, ip, u8p, sz, szp, u8p, vp]
        lib.kzg355_compute_kzg_proofs_at_many_device.argtypes = [vp, vp, ip, vp, sz, szp, u8p, vp]
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    h = vp()
    assert lib.kzg355_load_trusted_setup(g1, 4096, g2, 65, C.byref(h)) == 0
    assert lib.kzg355_settings_build_msm_table(h) == 0
    dev = torch.device("cuda", lib.kzg355_settings_device(h))
    all_blobs = open(a.blobs, "rb").read()
    sampler = PowerSampler(dev.index or 0)
    sampler.start()
    rows = []
    for shape in a.shapes.split(","):
        n, k, domain = parse_shape(shape)
        total = n * k
        lists = points(n, k, domain)
        zs = b"".join(z for one in lists for z in one)
        blobs = all_blobs[:BLOB * n]
        dup = b"".join(blobs[BLOB * i:BLOB * (i + 1)] * k for i in range(n))
        counts, st, st_old = (C.c_size_t * n)(*([k] * n)), (C.c_int * n)(), (C.c_int * total)()
        p_old, y_old, p_new, y_new = (C.create_string_buffer(w * total) for w in (48, 32, 48, 32))
        d_blobs = torch.frombuffer(bytearray(blobs), dtype=torch.uint8).to(dev)
        d_p, d_y = torch.zeros(48 * total, dtype=torch.uint8, device=dev), torch.zeros(32 * total, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def yardstick():
            assert lib.kzg355_compute_kzg_proof_many(p_old, y_old, st_old, dup, zs, total, h) == 0

        variants = {"yardstick": yardstick}
        if new:
            variants["host"] = lambda: lib.kzg355_compute_kzg_proofs_at_many(p_new, y_new, st, blobs, n, counts, zs, h) == 0 or sys.exit("host form failed")
            variants["ys_only"] = lambda: lib.kzg355_compute_kzg_proofs_at_many(None, y_new, st, blobs, n, counts, zs, h) == 0 or sys.exit("ys only failed")
            variants["device"] = lambda: lib.kzg355_compute_kzg_proofs_at_many_device(d_p.data_ptr(), d_y.data_ptr(), st, d_blobs.data_ptr(), n, counts, zs,
                                                                                      h) == 0 or sys.exit("device form failed")
        row = {"build": a.label, "round": a.round, "shape": shape, "openings": total}
        for name, fn in variants.items():
            t = time.perf_counter()
            fn()
            first = 1e3 * (time.perf_counter() - t)
            if name == "yardstick" and first > a.slow_ms:
                row[name] = {"ms_median": round(first, 3), "ms_min": round(first, 3), "ms_max": round(first, 3), "calls": 1,
                             "openings_per_s": round(1e3 * total / first, 1)}
                continue
            for _ in range(a.warmup - 1):
                fn()
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                fn()
                ts.append(1e3 * (time.perf_counter() - t))
            med = statistics.median(ts)
            row[name] = {"ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "calls": a.reps,
                         "openings_per_s": round(1e3 * total / med, 1)}
            lib.kzg355_set_kernel_timing(h, 1)
            lib.kzg355_reset_kernel_stats(h)
            fn()
            lib.kzg355_set_kernel_timing(h, 0)
            for fam in FAMILIES:
                ms, launches = C.c_double(), C.c_long()
                lib.kzg355_kernel_ms_stats(h, fam.encode(), C.byref(ms), C.byref(launches))
                if launches.value:
                    row[name][fam + "_ms"] = round(ms.value, 4)
        if new:
            assert p_new.raw == p_old.raw and y_new.raw == y_old.raw, shape
            assert bytes(d_p.cpu().numpy()) == p_old.raw and bytes(d_y.cpu().numpy()) == y_old.raw, shape
        rows.append(row)
    clk = sampler.stop()
    for row in rows:
        row["sclk_mhz"] = clk and clk["sclk_mhz"]
        print(json.dumps(row), flush=True)
    lib.kzg355_free_trusted_setup(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the build to compare with (libkzg355.so of the parent commit)")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slow-ms", type=float, default=10000.0, dest="slow_ms")
    ap.add_argument("--shapes", default="1x1,1x64,1x4096d,1x4096,64x64")
    ap.add_argument("--child")
    ap.add_argument("--label")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--blobs")
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth import random_blob
    nmax = max(parse_shape(s)[0] for s in a.shapes.split(","))
    builds = ([("other", a.other)] if a.other else []) + [("this", os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so"))]
    rows = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "blobs.bin")
        with open(path, "wb") as f:
            for i in range(nmax):
                f.write(random_blob(48440 + i))
        for r in range(a.rounds):
            for label, lib in builds:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--label", label, "--round", str(r), "--blobs", path,
                                      "--reps", str(a.reps), "--warmup", str(a.warmup), "--slow-ms", str(a.slow_ms), "--shapes", a.shapes],
                                     capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    print(out.stdout, out.stderr, sep="\n", flush=True)
                    return 1                                        # nothing more is started after a failed child
                for ln in out.stdout.splitlines():
                    print(ln, flush=True)
                    rows.append(json.loads(ln))
    for label, _ in builds:
        for shape in a.shapes.split(","):
            mine = [r for r in rows if r["build"] == label and r["shape"] == shape]
            line = {"summary": label, "shape": shape}
            for v in ("yardstick", "host", "ys_only", "device"):
                if mine and all(v in r for r in mine):
                    med = statistics.median(r[v]["ms_median"] for r in mine)
                    line[v] = {"ms_median": round(med, 3), "ms_min": min(r[v]["ms_min"] for r in mine), "ms_max": max(r[v]["ms_max"] for r in mine),
                               "openings_per_s": round(1e3 * mine[0]["openings"] / med, 1)}
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
