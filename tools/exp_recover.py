#!/usr/bin/env python3
"""Cost of recover_cells_and_kzg_proofs (EIP-7594 recovery from half of a blob's cells) next to the calls that compute from the blob, in one
process, on the same seeded blobs and one random set of 64 cell indices.  For m = 1 and 128 blobs (--sizes):
  * cells only: kzg355_recover_cells_and_kzg_proofs_many with no proof output against kzg355_compute_cells_and_kzg_proofs_many with none;
  * cells and proofs: the same two entry points with both outputs.  The compute call is the yardstick.
The two calls of a pair alternate, --reps timed pairs after --warmup; ms per call as median (min-max).  One more call of each with the
library's per-kernel timing on gives the stages: rc_vanish, rc_interp, rc_columns, rc_cells of the recovery's own field stage, cc_field of the
compute call's, and the FK20 chain both share (cc_columns, cc_msm, cc_proofs).  The C entry points get preallocated buffers, so no figure
holds Python object construction.  Every recovered output is compared with the computed one.  The shader clock is sampled from the card's
hwmon files over the timed calls (best effort).
Run:  python tools/exp_recover.py [--reps 7] [--warmup 2]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kzg_rust_amd as kz              # noqa: E402
from bench import PowerSampler         # noqa: E402
from synth import random_blob          # noqa: E402

RC = ["rc_vanish", "rc_interp", "rc_columns", "rc_cells"]
CC = ["cc_field", "cc_columns", "cc_msm", "cc_proofs"]
CELL_B, CELLS_B, PROOFS_B, BLOB_B = 2048, 128 * 2048, 128 * 48, 131072


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,128")
    a = ap.parse_args()
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    lib = kz.kzg.lib()
    sizes = [int(x) for x in a.sizes.split(",")]
    mmax = max(sizes)
    blobs = b"".join(random_blob(60000 + i) for i in range(mmax))
    ix = sorted(random.Random(7594).sample(range(128), 64))
    n = len(ix)
    idx = (C.c_size_t * n)(*ix)
    c_cells, c_proofs = C.create_string_buffer(CELLS_B * mmax), C.create_string_buffer(PROOFS_B * mmax)
    r_cells, r_proofs = C.create_string_buffer(CELLS_B * mmax), C.create_string_buffer(PROOFS_B * mmax)
    st = (C.c_int * mmax)()

    def compute(m, proofs):
        rc = lib.kzg355_compute_cells_and_kzg_proofs_many(c_cells, c_proofs if proofs else None, st, blobs, m, s.handle)
        assert rc == 0 and not any(st[i] for i in range(m)), rc

    compute(mmax, True)                                           # also the proof setup of the handle
    full = c_cells.raw
    known = b"".join(full[CELLS_B * b + CELL_B * k:CELLS_B * b + CELL_B * (k + 1)] for b in range(mmax) for k in ix)

    def recover(m, proofs):
        rc = lib.kzg355_recover_cells_and_kzg_proofs_many(r_cells, r_proofs if proofs else None, st, idx, known, n, m, s.handle)
        assert rc == 0 and not any(st[i] for i in range(m)), rc

    sampler = PowerSampler(s.device)
    sampler.start()
    for m in sizes:
        for proofs in (False, True):
            for _ in range(a.warmup):
                compute(m, proofs); recover(m, proofs)
            tc, tr = [], []
            for _ in range(a.reps):
                t = time.perf_counter(); compute(m, proofs); tc.append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter(); recover(m, proofs); tr.append(1e3 * (time.perf_counter() - t))
            assert r_cells.raw[:CELLS_B * m] == c_cells.raw[:CELLS_B * m], m
            if proofs:
                assert r_proofs.raw[:PROOFS_B * m] == c_proofs.raw[:PROOFS_B * m], m
            s.set_kernel_timing(True)
            compute(m, proofs)
            k_c = {f: round(s.last_kernel_ms(f), 3) for f in (CC if proofs else CC[:1])}
            recover(m, proofs)
            k_r = {f: round(s.last_kernel_ms(f), 3) for f in (RC + CC[1:] if proofs else RC)}
            s.set_kernel_timing(False)
            print(json.dumps({"m": m, "proofs": proofs, "known_cells": n, "compute": stats(tc), "recover": stats(tr),
                              "recover_minus_compute_ms": round(statistics.median(tr) - statistics.median(tc), 3),
                              "compute_kernel_ms": k_c, "recover_kernel_ms": k_r, "recover_field_stage_ms": round(sum(k_r[f] for f in RC), 3),
                              "reps": a.reps, "warmup": a.warmup}), flush=True)
    clk = sampler.stop()
    print(json.dumps({"clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
