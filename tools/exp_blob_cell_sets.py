#!/usr/bin/env python3
"""verify_blob_cell_proofs_batch_many_sets (blob transactions of different blob counts in one call) on one device and one handle, against what a
caller composes without it, through the C entry points with preallocated buffers (host: bytes; device: torch tensors).

The mix: 64 transactions with blob counts cycling 1 .. 6 (224 blobs), the blobs the three seeded fixture blobs of tests/golden/cells.json with
their commitments and cell proofs, blob (t + i) mod 3 at place i of transaction t.
  (a) one `_sets` call
  (b) one uniform `_many` call per distinct count: 6 calls (the caller's regrouping of its arrays by count is NOT timed: the arrays are prepared)
  (c) one `_many` call per transaction: 64 calls
and 64 x 6 uniform groups through `_sets` and through `_many`.  Host arrays and device-resident arrays, warm, medians of --reps calls after --warmup
with min and max; then, with the library's kernel timing on, the per-family kernel times of (a) and of the two uniform calls.  Every timed call
must be true.  The shader clock is sampled over the run (best effort).
Run:  python tools/exp_blob_cell_sets.py [--reps 9] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["cell_host", "cc_field", "cell_prep", "cell_rhash", "cell_points", "cell_scalars", "cell_interp", "cell_lincomb", "cell_pairing"]


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert a.reps >= 7
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import kzg_rust_amd as kz
    from bench import PowerSampler
    from synth import random_blob

    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    fx = json.load(open(os.path.join(g, "cells.json")))
    blobs = [random_blob(x) for x in fx["blob_seeds"]]
    Cm = [bytes.fromhex(c) for c in fx["commitments"]]
    P = [b"".join(bytes.fromhex(p) for p in ps) for ps in fx["proofs"]]
    lib = kz.kzg.lib()
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    sampler = PowerSampler(s.device)
    sampler.start()

    class Arrays:
        """the transactions `txs` (lists of fixture blob numbers) one after the other, in host and in device memory"""

        def __init__(self, txs):
            which = [w for tx in txs for w in tx]
            self.counts, self.G = [len(tx) for tx in txs], len(txs)
            self.h = (b"".join(blobs[w] for w in which), b"".join(Cm[w] for w in which), b"".join(P[w] for w in which))
            self.t = [torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda() for x in self.h]
            self.d = tuple(x.data_ptr() for x in self.t)
            self.ok, self.st, self.cnt = (C.c_bool * self.G)(), (C.c_int * self.G)(), (C.c_size_t * self.G)(*self.counts)

        def sets(self, device):
            fn = lib.kzg355_verify_blob_cell_proofs_batch_many_sets_device if device else lib.kzg355_verify_blob_cell_proofs_batch_many_sets
            rc = fn(self.ok, self.st, self.cnt, *(self.d if device else self.h), self.G, s.handle)
            assert rc == 0 and all(self.ok), rc

        def many(self, device):
            assert len(set(self.counts)) == 1
            fn = lib.kzg355_verify_blob_cell_proofs_batch_many_device if device else lib.kzg355_verify_blob_cell_proofs_batch_many
            rc = fn(self.ok, self.st, *(self.d if device else self.h), self.counts[0], self.G, s.handle)
            assert rc == 0 and all(self.ok), rc

    mix = [[(t + i) % 3 for i in range(1 + t % 6)] for t in range(64)]
    whole = Arrays(mix)
    by_count = [Arrays([tx for tx in mix if len(tx) == n]) for n in range(1, 7)]
    each = [Arrays([tx]) for tx in mix]
    uniform = Arrays([[(t + i) % 3 for i in range(6)] for t in range(64)])
    print(json.dumps({"mix": {"transactions": 64, "blobs": sum(whole.counts), "per_count": [x.G for x in by_count]}}), flush=True)

    def families(fn):
        s.set_kernel_timing(True)
        lib.kzg355_reset_kernel_stats(s.handle)
        rows = []
        for _ in range(a.reps):
            fn()
            rows.append({f: s.last_kernel_ms(f) for f in FAMILIES})
        s.set_kernel_timing(False)
        return {f: round(statistics.median(x[f] for x in rows), 3) for f in FAMILIES if rows[0][f] >= 0}

    for device in (False, True):
        where = "device" if device else "host"
        row = {"arrays": where}
        row["a_one_sets_call"] = stats(timed(lambda: whole.sets(device), a.reps, a.warmup))
        row["b_six_many_calls"] = stats(timed(lambda: [x.many(device) for x in by_count], a.reps, a.warmup))
        row["c_64_calls"] = stats(timed(lambda: [x.many(device) for x in each], a.reps, a.warmup))
        row["uniform_64x6_sets"] = stats(timed(lambda: uniform.sets(device), a.reps, a.warmup))
        row["uniform_64x6_many"] = stats(timed(lambda: uniform.many(device), a.reps, a.warmup))
        row["a_one_sets_call"]["kernel_ms_median"] = families(lambda: whole.sets(device))
        row["uniform_64x6_sets"]["kernel_ms_median"] = families(lambda: uniform.sets(device))
        row["uniform_64x6_many"]["kernel_ms_median"] = families(lambda: uniform.many(device))
        print(json.dumps(row), flush=True)
    clk = sampler.stop()
    print(json.dumps({"clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}, "reps": a.reps, "warmup": a.warmup}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
