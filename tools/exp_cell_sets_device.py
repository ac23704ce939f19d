#!/usr/bin/env python3
"""verify_cell_kzg_proof_batch_many_sets_device on three ragged shapes, on one device, through the C entry points with preallocated buffers:
  * 128 groups of 1 .. 64 cells, 1024 groups of 1 .. 6 cells, 8 groups of 1000 .. 16000 cells (sizes drawn once from --seed).
Per shape three routes for data that is resident in HBM are timed in turn: the call prepared on the device (prep_form 1), the call prepared on
the host from a copy back inside the library (prep_form 2), and what a caller had before the call existed -- the four arrays copied to host
memory (torch .cpu()) and the host `_sets` form on them.  Then each once more with the library's kernel timing on: cell_host (host
preparation) next to cell_prep and cell_rhash.  Every timed call must be true.  The line also says which route a prep_form 0 call takes.
Medians of --reps calls after --warmup, with min and max; the shader clock is sampled from the card's hwmon files over the run (best effort).
Run:  python tools/exp_cell_sets_device.py [--reps 7] [--warmup 2]"""
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

import torch                           # noqa: E402
import cell_spec as cs                 # noqa: E402
import kzg_rust_amd as kz              # noqa: E402
from bench import PowerSampler         # noqa: E402
from synth import random_blob          # noqa: E402

FAMILIES = ["cell_host", "cell_prep", "cell_rhash", "cell_points", "cell_scalars", "cell_interp", "cell_lincomb", "cell_pairing"]


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    assert a.reps >= 7
    rng = random.Random(a.seed)
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    lib = kz.kzg.lib()
    fx = json.load(open(os.path.join(g, "cells.json")))
    cells = [cs.compute_cells(random_blob(x)) for x in fx["blob_seeds"]]
    Cm = [bytes.fromhex(c) for c in fx["commitments"]]
    P = [[bytes.fromhex(p) for p in ps] for ps in fx["proofs"]]
    nb = len(cells)
    shapes = [("128_groups_of_1_to_64", [rng.randint(1, 64) for _ in range(128)]), ("1024_groups_of_1_to_6", [rng.randint(1, 6) for _ in range(1024)]),
              ("8_groups_of_1000_to_16000", [rng.randint(1000, 16000) for _ in range(8)])]
    u8p, szp = C.c_char_p, C.POINTER(C.c_size_t)                                                 # the loader's types for host arrays
    sampler = PowerSampler(s.device)
    sampler.start()
    kz.Kzg.verify_cell_kzg_proof_batch([Cm[0]], [5], [cells[0][5]], [P[0][5]], s)               # the handle's cell setup
    for name, counts in shapes:
        G, N = len(counts), sum(counts)
        items = [(rng.randrange(nb), rng.randrange(128)) for _ in range(N)]      # valid cells of a few blobs: every group is true
        d_c = torch.frombuffer(bytearray(b"".join(Cm[b] for b, _ in items)), dtype=torch.uint8).cuda()
        d_cl = torch.frombuffer(bytearray(b"".join(cells[b][k] for b, k in items)), dtype=torch.uint8).cuda()
        d_p = torch.frombuffer(bytearray(b"".join(P[b][k] for b, k in items)), dtype=torch.uint8).cuda()
        d_i = torch.tensor([k for _, k in items], dtype=torch.int64).cuda()
        ptrs = (d_c.data_ptr(), d_i.data_ptr(), d_cl.data_ptr(), d_p.data_ptr())
        ok, st, dbg, cnt = (C.c_bool * G)(), (C.c_int * G)(), C.create_string_buffer(176 * G), (C.c_size_t * G)(*counts)

        def device(form):
            def f():
                rc = lib.kzg355_debug_cell_batch_intermediates_sets_device(dbg, ok, st, cnt, *ptrs, G, form, s.handle)
                assert rc == 0 and all(ok), (name, form, rc)
            return f

        def copy_back_then_host_form():
            h_c, h_i, h_cl, h_p = d_c.cpu(), d_i.cpu(), d_cl.cpu(), d_p.cpu()
            rc = lib.kzg355_verify_cell_kzg_proof_batch_many_sets(ok, st, cnt, C.cast(h_c.data_ptr(), u8p), C.cast(h_i.data_ptr(), szp),
                                                                  C.cast(h_cl.data_ptr(), u8p), C.cast(h_p.data_ptr(), u8p), G, s.handle)
            assert rc == 0 and all(ok), (name, rc)
        before = s.cell_device_prep_calls
        rc = lib.kzg355_verify_cell_kzg_proof_batch_many_sets_device(ok, st, cnt, *ptrs, G, s.handle)
        assert rc == 0 and all(ok)
        row = {"shape": name, "groups": G, "cells": N, "largest_group": max(counts),
               "prep_form_0_takes": "device" if s.cell_device_prep_calls - before else "host"}
        for label, fn in (("device_prep", device(1)), ("host_prep", device(2)), ("copy_back_then_host_form", copy_back_then_host_form)):
            row[label] = stats(timed(fn, a.reps, a.warmup))
            s.set_kernel_timing(True)
            lib.kzg355_reset_kernel_stats(s.handle)
            fn()
            row[label]["kernel_ms"] = {f: round(s.last_kernel_ms(f), 3) for f in FAMILIES if s.last_kernel_ms(f) >= 0}
            s.set_kernel_timing(False)
        print(json.dumps(row), flush=True)
    clk = sampler.stop()
    print(json.dumps({"clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}, "reps": a.reps, "warmup": a.warmup}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
