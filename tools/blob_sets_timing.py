#!/usr/bin/env python3
"""kzg355_verify_blob_kzg_proof_batch_many_sets_device (batches of different blob counts in one call) against the uniform
kzg355_verify_blob_kzg_proof_batch_many_device, on device-resident inputs: the 512 blobs of tests/golden/batch512.json with their commitments and
proofs, repeated on the device to 24,576 blobs (3.2 GB).
  (a) 4096 batches, all of 6 blobs: the ragged call, and the uniform call with n_per_group = 6
  (b) the same blobs with counts cycling 1 .. 6 (7021 batches): the ragged call
Warm wall-clock medians of --reps calls after --warmup, then, with the library's kernel timing on, the HIP-event milliseconds per kernel family of
one more call of each (the stage-1 families are the same launches in all three).  Every batch of every timed call must be true.
Run:  python tools/blob_sets_timing.py [--reps 7] [--warmup 2]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["validate_points", "challenge", "challenge_from_digest", "eval", "rpowers", "lincomb", "pairing", "err_fold"]
REPEAT, N_FIXTURE = 48, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import kzg_rust_amd as kz
    from synth import random_blob

    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    fx = json.load(open(os.path.join(g, "batch512.json")))
    lib = kz.kzg.lib()
    os.environ.setdefault("KZG355_MSM", "bucket")                  # a verify-only run: no wide MSM table
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])

    def dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0").repeat(REPEAT)
    d_blobs = dev(b"".join(random_blob(fx["first_index"] + i) for i in range(N_FIXTURE)))
    d_c = dev(b"".join(bytes.fromhex(x) for x in fx["commitments"]))
    d_p = dev(b"".join(bytes.fromhex(x) for x in fx["proofs"]))
    total = REPEAT * N_FIXTURE
    ptrs = [C.c_void_p(t.data_ptr()) for t in (d_blobs, d_c, d_p)]
    uniform = [6] * (total // 6)
    cycling = list(range(1, 7)) * (total // 21)
    cycling.append(total - sum(cycling))
    assert sum(uniform) == sum(cycling) == total and 1 <= cycling[-1] <= 6

    def caller(counts, ragged):
        G = len(counts)
        ok, st = (C.c_bool * G)(), (C.c_int * G)()
        cnt = (C.c_size_t * G)(*counts)

        def call():
            if ragged:
                rc = lib.kzg355_verify_blob_kzg_proof_batch_many_sets_device(ok, st, cnt, *ptrs, G, s.handle)
            else:
                rc = lib.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, *ptrs, counts[0], G, s.handle)
            assert rc == 0 and all(ok), rc
        return call

    runs = {"a_ragged_4096x6": caller(uniform, True), "a_uniform_4096x6": caller(uniform, False), "b_ragged_cycling_1_6": caller(cycling, True)}
    out = {"blobs": total, "groups": {"a": len(uniform), "b": len(cycling)}, "device": torch.cuda.get_device_name(0), "runs": {}}
    for name, call in runs.items():
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter(); call(); ts.append(1e3 * (time.perf_counter() - t))
        lib.kzg355_set_kernel_timing(s.handle, 1)
        lib.kzg355_reset_kernel_stats(s.handle)
        call()
        fam = {}
        for f in FAMILIES:
            ms, n = C.c_double(), C.c_long()
            if lib.kzg355_kernel_ms_stats(s.handle, f.encode(), C.byref(ms), C.byref(n)) == 0 and n.value:
                fam[f] = {"ms": round(ms.value, 3), "launches": n.value}
        lib.kzg355_set_kernel_timing(s.handle, 0)
        out["runs"][name] = {"wall_ms_median": round(statistics.median(ts), 3), "wall_ms_min": round(min(ts), 3), "wall_ms_max": round(max(ts), 3),
                             "blobs_per_s": round(total / (statistics.median(ts) * 1e-3)), "kernel_ms": fam}
    print(json.dumps(out, indent=1))
    s.free()


if __name__ == "__main__":
    main()
