#!/usr/bin/env python3
"""The device-resident forms of the three EIP-7594 cell calls against their host forms, on one device, through the C entry points with
preallocated buffers (host: bytes / ctypes buffers; device: torch tensors).
  * verify: the six shapes of tools/exp_cell_verify.py (128 groups of 6 / 16 / 32 / 64 cells, one batch of 4096 cells, n = 1).  Per shape the
    host form, the device form prepared on the device (prep_form 1) and the device form prepared on the host from a copy back (prep_form 2) are
    timed in turn, then once more each with the library's kernel timing on: cell_host (host preparation) next to cell_prep and cell_rhash.
    Every timed call must be true.  The line also says which preparation a prep_form 0 call of that shape takes.
  * compute and recover (64 known cells) at m = 1, 128, 512 blobs, cells + proofs and cells only, host form against device form; the device
    outputs must equal the host outputs.
Medians of --reps calls after --warmup, with min and max; the shader clock is sampled from the card's hwmon files over the run (best effort).
Run:  python tools/exp_cell_device.py [--reps 7] [--warmup 2] [--sizes 1,128,512]"""
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

VERIFY = ["cell_host", "cell_prep", "cell_rhash", "cell_points", "cell_scalars", "cell_interp", "cell_lincomb", "cell_pairing"]
CELL_B, CELLS_B, PROOFS_B = 2048, 128 * 2048, 128 * 48


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


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
    ap.add_argument("--sizes", default="1,128,512")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    assert a.reps >= 7
    random.seed(a.seed)
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

    def items_of(items):
        return [Cm[b] for b, _ in items], [k for _, k in items], [cells[b][k] for b, k in items], [P[b][k] for b, k in items]

    shapes = [(f"sidecar_many_128x{n}", [items_of([(b % nb, col) for b in range(n)]) for col in range(128)]) for n in (6, 16, 32, 64)]
    shapes.append(("single_batch_128x32", [items_of([(random.randrange(nb), random.randrange(128)) for _ in range(128 * 32)])]))
    shapes.append(("single_n1", [items_of([(5 % nb, 5)])]))
    sampler = PowerSampler(s.device)
    sampler.start()
    kz.Kzg.verify_cell_kzg_proof_batch(*shapes[-1][1][0], s)                                  # the handle's cell setup
    for name, groups in shapes:
        G, npg = len(groups), len(groups[0][0])
        h_c, h_cl, h_p = (b"".join(b"".join(x[k]) for x in groups) for k in (0, 2, 3))
        ix = [i for x in groups for i in x[1]]
        h_i = (C.c_size_t * len(ix))(*ix)
        d_c, d_cl, d_p = dev(h_c), dev(h_cl), dev(h_p)
        d_i = torch.tensor(ix, dtype=torch.int64).cuda()
        ok, st, dbg = (C.c_bool * G)(), (C.c_int * G)(), C.create_string_buffer(176 * G)

        def host():
            rc = lib.kzg355_verify_cell_kzg_proof_batch_many(ok, st, h_c, h_i, h_cl, h_p, npg, G, s.handle)
            assert rc == 0 and all(ok), (name, rc)

        def device(form):
            def f():
                rc = lib.kzg355_debug_cell_batch_intermediates_device(dbg, ok, st, d_c.data_ptr(), d_i.data_ptr(), d_cl.data_ptr(), d_p.data_ptr(), npg, G,
                                                                      form, s.handle)
                assert rc == 0 and all(ok), (name, form, rc)
            return f
        before = s.cell_device_prep_calls
        rc = lib.kzg355_verify_cell_kzg_proof_batch_many_device(ok, st, d_c.data_ptr(), d_i.data_ptr(), d_cl.data_ptr(), d_p.data_ptr(), npg, G, s.handle)
        assert rc == 0 and all(ok)
        auto = "device" if s.cell_device_prep_calls - before else "host"
        row = {"shape": name, "groups": G, "n_per_group": npg, "cells": G * npg, "transcript_bytes_per_group": 48 + 48 * len(set(groups[0][0])) + 2112 * npg,
               "prep_form_0_takes": auto}
        for label, fn in (("host_form", host), ("device_prep", device(1)), ("device_form_host_prep", device(2))):
            row[label] = stats(timed(fn, a.reps, a.warmup))
            s.set_kernel_timing(True)
            lib.kzg355_reset_kernel_stats(s.handle)
            fn()
            row[label]["kernel_ms"] = {f: round(s.last_kernel_ms(f), 3) for f in VERIFY if s.last_kernel_ms(f) >= 0}
            s.set_kernel_timing(False)
        print(json.dumps(row), flush=True)

    sizes = [int(x) for x in a.sizes.split(",")]
    mmax = max(sizes)
    blobs = b"".join(random_blob(60000 + i) for i in range(mmax))
    kix = sorted(random.Random(7594).sample(range(128), 64))
    idx = (C.c_size_t * 64)(*kix)
    h_cells, h_proofs = C.create_string_buffer(CELLS_B * mmax), C.create_string_buffer(PROOFS_B * mmax)
    st = (C.c_int * mmax)()
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(h_cells, h_proofs, st, blobs, mmax, s.handle) == 0       # also the handle's proof setup
    full = h_cells.raw
    known = b"".join(full[CELLS_B * b + CELL_B * k:CELLS_B * b + CELL_B * (k + 1)] for b in range(mmax) for k in kix)
    d_blobs, d_known = dev(blobs), dev(known)
    d_cells = torch.zeros(CELLS_B * mmax, dtype=torch.uint8, device="cuda")
    d_proofs = torch.zeros(PROOFS_B * mmax, dtype=torch.uint8, device="cuda")
    for m in sizes:
        for proofs in (False, True):
            hp, dp = (h_proofs, d_proofs.data_ptr()) if proofs else (None, None)

            def ok_(rc):
                assert rc == 0 and not any(st[i] for i in range(m)), rc
            calls = {
                "compute_host": lambda: ok_(lib.kzg355_compute_cells_and_kzg_proofs_many(h_cells, hp, st, blobs, m, s.handle)),
                "compute_device": lambda: ok_(lib.kzg355_compute_cells_and_kzg_proofs_many_device(d_cells.data_ptr(), dp, st, d_blobs.data_ptr(), m, s.handle)),
                "recover_host": lambda: ok_(lib.kzg355_recover_cells_and_kzg_proofs_many(h_cells, hp, st, idx, known, 64, m, s.handle)),
                "recover_device": lambda: ok_(lib.kzg355_recover_cells_and_kzg_proofs_many_device(d_cells.data_ptr(), dp, st, idx, d_known.data_ptr(), 64, m,
                                                                                                   s.handle)),
            }
            row = {"m": m, "proofs": proofs}
            for label, fn in calls.items():
                d_cells.zero_(); d_proofs.zero_()
                row[label] = stats(timed(fn, a.reps, a.warmup))
                if label.endswith("device"):
                    assert bytes(d_cells[:CELLS_B * m].cpu().numpy()) == full[:CELLS_B * m], (label, m)
                    assert not proofs or bytes(d_proofs[:PROOFS_B * m].cpu().numpy()) == h_proofs.raw[:PROOFS_B * m], (label, m)
            print(json.dumps(row), flush=True)
    clk = sampler.stop()
    print(json.dumps({"clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}, "reps": a.reps, "warmup": a.warmup}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
