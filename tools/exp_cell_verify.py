#!/usr/bin/env python3
"""Throughput of verify_cell_kzg_proof_batch (EIP-7594 cells) on one device: cells/s and ms per call for
  * the sidecar shape: verify_cell_kzg_proof_batch_many with 128 groups (one per column) of n_per_group in {6, 16, 32, 64} cells;
  * one large single batch of 128 x 32 cells;
  * n = 1.
Every timed call must return True.  The valid cells and proofs come from the committed fixture tests/golden/cells.json (oracle-derived, three
seeded blobs): a group of column c takes cell c of blob b mod 3 for b < n_per_group, so commitments repeat within a group (3 unique).  Per shape:
warm-up calls, then --reps timed calls (median, min, max of the wall time), then one more call with the library's per-kernel timing on, which
splits the call into host preparation (commitment dedup, column sort, transcript SHA-256: "cell_host") and the device kernel families.
Run:  python tools/exp_cell_verify.py [--reps 7] [--warmup 2]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cell_spec as cs                 # noqa: E402
import kzg_rust_amd as kz              # noqa: E402
from synth import random_blob          # noqa: E402

FAMILIES = ["cell_host", "cell_points", "cell_scalars", "cell_interp", "cell_lincomb", "cell_pairing"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    random.seed(a.seed)
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    fx = json.load(open(os.path.join(g, "cells.json")))
    cells = [cs.compute_cells(random_blob(x)) for x in fx["blob_seeds"]]
    C = [bytes.fromhex(c) for c in fx["commitments"]]
    P = [[bytes.fromhex(p) for p in ps] for ps in fx["proofs"]]
    nb = len(cells)

    def group(col, n):
        items = [(b % nb, col) for b in range(n)]
        return [C[b] for b, _ in items], [k for _, k in items], [cells[b][k] for b, k in items], [P[b][k] for b, k in items]

    def rand_group(n):
        items = [(random.randrange(nb), random.randrange(128)) for _ in range(n)]
        return [C[b] for b, _ in items], [k for _, k in items], [cells[b][k] for b, k in items], [P[b][k] for b, k in items]

    t0 = time.perf_counter()
    kz.Kzg.verify_cell_kzg_proof_batch(*group(0, 1), s)
    first_ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps({"first_cell_call_ms_incl_setup": round(first_ms, 2)}), flush=True)

    shapes = [(f"sidecar_many_128x{n}", "many", [group(c, n) for c in range(128)]) for n in (6, 16, 32, 64)]
    shapes.append(("single_batch_128x32", "single", [rand_group(128 * 32)]))
    shapes.append(("single_n1", "single", [group(5, 1)]))
    for name, form, groups in shapes:
        n_cells = sum(len(x[0]) for x in groups)

        def call():
            if form == "many":
                r = kz.Kzg.verify_cell_kzg_proof_batch_many(groups, s)
            else:
                r = [kz.Kzg.verify_cell_kzg_proof_batch(*groups[0], s)]
            assert r == [True] * len(groups), (name, r)
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            call()
            ts.append(1e3 * (time.perf_counter() - t))
        s.set_kernel_timing(True)
        call()
        split = {f: round(s.last_kernel_ms(f), 3) for f in FAMILIES}
        s.set_kernel_timing(False)
        med = statistics.median(ts)
        dev = round(sum(v for k, v in split.items() if k != "cell_host"), 3)
        print(json.dumps({"shape": name, "cells": n_cells, "ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                          "cells_per_s": round(n_cells / (med / 1e3)), "host_prep_ms": split["cell_host"], "device_kernels_ms": dev,
                          "split_ms": split, "reps": a.reps, "warmup": a.warmup}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
