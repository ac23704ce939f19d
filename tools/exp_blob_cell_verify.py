#!/usr/bin/env python3
"""verify_blob_cell_proofs_batch (blobs against their EIP-7594 cell proofs) on one device, against what a client composes without it, through
the C entry points with preallocated buffers (host: bytes / ctypes buffers; device: torch tensors).

Shapes (transactions x blobs per transaction): 1 x 1, 1 x 6, 64 x 1, 64 x 6, 1 x 128.  The blobs are the three seeded fixture blobs of
tests/golden/cells.json with their commitments and cell proofs, blob (t + i) mod 3 at place i of transaction t: three unique commitments at most.

  --part yardstick   compute_cells_and_kzg_proofs_many (cells only) followed by verify_cell_kzg_proof_batch_many on host buffers, INCLUDING the
                     caller's array building (every commitment 128 times, the indices 0..127 per blob); and the same on device buffers
                     (compute ..._many_device into a device tensor, the arrays built with torch, verify ..._many_device).  Uses nothing this
                     tool's call added: --package-root points it at another checkout's kzg_rust_amd (the parent commit) on the same box.
  --part new         kzg355_verify_blob_cell_proofs_batch_many and its _device form; then, with the library's kernel timing on, the cell_interp
                     family (k_blob_weights + k_blob_coef + k_cell_interp, or k_cell_columns + k_cell_interp) under interp_form 1 and 2 next to
                     the other families; and the first call on a fresh handle (the 384 MiB proof setup is not built: it would take seconds).
Every timed call must be true.  Medians of --reps calls after --warmup, with min and max; the shader clock is sampled over the run (best effort).
Run:  python tools/exp_blob_cell_verify.py [--part all] [--reps 7] [--warmup 2]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 6), (64, 1), (64, 6), (1, 128)]
FAMILIES = ["cell_host", "cc_field", "cell_prep", "cell_rhash", "cell_points", "cell_scalars", "cell_interp", "cell_lincomb", "cell_pairing"]
BLOB_B, CELLS_B = 131072, 128 * 2048


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
    ap.add_argument("--part", choices=["all", "yardstick", "new"], default="all")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose kzg_rust_amd is measured")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.reps >= 7
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    import kzg_rust_amd as kz
    from bench import PowerSampler
    from synth import random_blob

    def dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    setup = ([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    fx = json.load(open(os.path.join(g, "cells.json")))
    blobs = [random_blob(x) for x in fx["blob_seeds"]]
    Cm = [bytes.fromhex(c) for c in fx["commitments"]]
    P = [b"".join(bytes.fromhex(p) for p in ps) for ps in fx["proofs"]]
    lib = kz.kzg.lib()
    print(json.dumps({"package": os.path.dirname(os.path.abspath(kz.__file__)), "version": lib.kzg355_version().decode(), "part": a.part}), flush=True)

    if a.part in ("all", "new"):
        s0 = kz.Kzg.load_trusted_setup(*setup)
        one = C.c_bool()
        t0 = time.perf_counter()
        rc = lib.kzg355_verify_blob_cell_proofs_batch(C.byref(one), blobs[0], 1, Cm[0], 1, P[0], 128, s0.handle)
        first_ms = 1e3 * (time.perf_counter() - t0)
        assert rc == 0 and one.value
        print(json.dumps({"first_blob_cell_call_on_a_fresh_handle_ms": round(first_ms, 2)}), flush=True)
        s0.free()

    s = kz.Kzg.load_trusted_setup(*setup)
    sampler = PowerSampler(s.device)
    sampler.start()
    for G, n in SHAPES:
        nb, npg = G * n, 128 * n
        which = [(t + i) % 3 for t in range(G) for i in range(n)]
        h_b, h_c, h_p = b"".join(blobs[w] for w in which), b"".join(Cm[w] for w in which), b"".join(P[w] for w in which)
        d_b, d_c, d_p = dev(h_b), dev(h_c), dev(h_p)
        ok, st, stb = (C.c_bool * G)(), (C.c_int * G)(), (C.c_int * nb)()
        row = {"shape": f"{G}x{n}", "groups": G, "blobs_per_group": n, "blobs": nb, "cells": 128 * nb}

        if a.part in ("all", "yardstick"):
            h_cells = C.create_string_buffer(CELLS_B * nb)
            d_cells = torch.zeros(CELLS_B * nb, dtype=torch.uint8, device="cuda")

            def y_host():
                rc = lib.kzg355_compute_cells_and_kzg_proofs_many(h_cells, None, stb, h_b, nb, s.handle)
                assert rc == 0
                com = b"".join(h_c[48 * i:48 * i + 48] * 128 for i in range(nb))          # the caller's three repeated arrays
                idx = (C.c_size_t * (128 * nb))(*(list(range(128)) * nb))
                rc = lib.kzg355_verify_cell_kzg_proof_batch_many(ok, st, com, idx, h_cells, h_p, npg, G, s.handle)
                assert rc == 0 and all(ok), rc

            def y_device():
                rc = lib.kzg355_compute_cells_and_kzg_proofs_many_device(d_cells.data_ptr(), None, stb, d_b.data_ptr(), nb, s.handle)
                assert rc == 0
                com = d_c.view(nb, 48).repeat_interleave(128, dim=0).contiguous()
                idx = torch.arange(128, dtype=torch.int64, device="cuda").repeat(nb)
                rc = lib.kzg355_verify_cell_kzg_proof_batch_many_device(ok, st, com.data_ptr(), idx.data_ptr(), d_cells.data_ptr(), d_p.data_ptr(), npg, G,
                                                                        s.handle)
                assert rc == 0 and all(ok), rc
            row["yardstick_host"] = stats(timed(y_host, a.reps, a.warmup))
            row["yardstick_device"] = stats(timed(y_device, a.reps, a.warmup))
            row["yardstick_host"]["pcie_bytes_per_blob"] = BLOB_B + 2 * CELLS_B + 128 * (48 + 8 + 48)

        if a.part in ("all", "new"):
            dbg = C.create_string_buffer(176 * G)

            def n_host():
                rc = lib.kzg355_verify_blob_cell_proofs_batch_many(ok, st, h_b, h_c, h_p, n, G, s.handle)
                assert rc == 0 and all(ok), rc

            def n_device():
                rc = lib.kzg355_verify_blob_cell_proofs_batch_many_device(ok, st, d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, G, s.handle)
                assert rc == 0 and all(ok), rc

            def n_form(form):
                def f():
                    rc = lib.kzg355_debug_blob_cell_batch_intermediates(dbg, ok, st, h_b, h_c, h_p, n, G, form, s.handle)
                    assert rc == 0 and all(ok), (form, rc)
                return f
            row["new_host"] = stats(timed(n_host, a.reps, a.warmup))
            row["new_device"] = stats(timed(n_device, a.reps, a.warmup))
            for form in (1, 2):
                fn = n_form(form)
                row[f"interp_form_{form}"] = stats(timed(fn, a.reps, a.warmup))
                s.set_kernel_timing(True)
                lib.kzg355_reset_kernel_stats(s.handle)
                fams = []
                for _ in range(a.reps):
                    fn()
                    fams.append({f: s.last_kernel_ms(f) for f in FAMILIES})
                s.set_kernel_timing(False)
                row[f"interp_form_{form}"]["kernel_ms_median"] = {f: round(statistics.median(x[f] for x in fams), 3) for f in FAMILIES if fams[0][f] >= 0}
            # the host form's PCIe traffic per blob: the blob up, the extension half back for the host's hash when the host hashes, the proofs
            row["new_host"]["pcie_bytes_per_blob_up"] = BLOB_B + 48 + 128 * 48
        print(json.dumps(row), flush=True)
    clk = sampler.stop()
    print(json.dumps({"clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}, "reps": a.reps, "warmup": a.warmup}), flush=True)
    s.free()


if __name__ == "__main__":
    main()
