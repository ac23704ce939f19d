#!/usr/bin/env python3
"""Throughput of compute_cells_and_kzg_proofs (EIP-7594 cells and their FK20 proofs) on one device:
  * the first call of a fresh handle (it builds the proof setup: 4096 monomial points and the comb table) against the next call;
  * kzg355_compute_cells_and_kzg_proofs_many at n = 1, 6, 32, 128, 512 seeded blobs: ms per call (median, min, max of --reps timed calls after
    --warmup), blobs/s, and one more call with the library's per-kernel timing on (field stage, columns, fixed-base sums, G1 transforms);
  * blob_to_kzg_commitment_many at n = 512 on the same handle, the yardstick the issue compares against.
The C entry point is called with preallocated buffers, so the figures hold no Python object construction.  The first timed output of every
shape is checked against single calls.
Run:  python tools/exp_cell_compute.py [--reps 5] [--warmup 1]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kzg_rust_amd as kz              # noqa: E402
from synth import random_blob          # noqa: E402

FAMILIES = ["cc_field", "cc_columns", "cc_msm", "cc_proofs"]
CELLS_B, PROOFS_B = 128 * 2048, 128 * 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1,6,32,128,512")
    a = ap.parse_args()
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    lib = kz.kzg.lib()
    sizes = [int(x) for x in a.sizes.split(",")]
    nmax = max(sizes)
    blobs = b"".join(random_blob(50000 + i) for i in range(nmax))
    cells, proofs = C.create_string_buffer(CELLS_B * nmax), C.create_string_buffer(PROOFS_B * nmax)
    st = (C.c_int * nmax)()

    def run(n):
        rc = lib.kzg355_compute_cells_and_kzg_proofs_many(cells, proofs, st, blobs, n, s.handle)
        assert rc == 0 and not any(st[i] for i in range(n)), rc

    t = time.perf_counter(); run(1); first = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter(); run(1); second = 1e3 * (time.perf_counter() - t)
    print(json.dumps({"first_call_ms_incl_setup": round(first, 1), "second_call_ms": round(second, 2), "setup_ms": round(first - second, 1)}), flush=True)

    for n in sizes:
        for _ in range(a.warmup):
            run(n)
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            run(n)
            ts.append(1e3 * (time.perf_counter() - t))
        c1, p1 = C.create_string_buffer(CELLS_B), C.create_string_buffer(PROOFS_B)
        j = n - 1
        assert lib.kzg355_compute_cells_and_kzg_proofs(c1, p1, blobs[131072 * j:131072 * (j + 1)], s.handle) == 0
        assert c1.raw == cells.raw[CELLS_B * j:CELLS_B * (j + 1)] and p1.raw == proofs.raw[PROOFS_B * j:PROOFS_B * (j + 1)], n
        s.set_kernel_timing(True)
        run(n)
        split = {f: round(s.last_kernel_ms(f), 3) for f in FAMILIES}
        s.set_kernel_timing(False)
        med = statistics.median(ts)
        print(json.dumps({"n": n, "ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                          "blobs_per_s": round(n / (med / 1e3), 1), "kernel_ms": split, "reps": a.reps, "warmup": a.warmup}), flush=True)

    n = 512
    bl = [blobs[131072 * i:131072 * (i + 1)] for i in range(min(n, nmax))]
    kz.Kzg.blob_to_kzg_commitment_many(bl, s)
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        kz.Kzg.blob_to_kzg_commitment_many(bl, s)
        ts.append(1e3 * (time.perf_counter() - t))
    med = statistics.median(ts)
    print(json.dumps({"yardstick": "blob_to_kzg_commitment_many", "n": len(bl), "ms_median": round(med, 3),
                      "blobs_per_s": round(len(bl) / (med / 1e3), 1)}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
