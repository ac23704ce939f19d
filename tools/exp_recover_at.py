#!/usr/bin/env python3
"""Cost of kzg355_recover_cells_and_kzg_proofs_at_many_sets (recovery, then one quotient and one MSM per wanted cell) next to the two ways to
the same cells and proofs before it, in one process on seeded blobs:
  (a) kzg355_recover_cells_and_kzg_proofs_many_sets with cells and proofs (the FK20 chain, always 128 proofs per blob);
  (b) what a client composed: the same call with cells only, cells 0..63 of every blob cut out as its blob (one memmove per blob), then
      kzg355_compute_cell_kzg_proofs_at_many on those blobs for the proofs.
Shapes (--shapes): blobs x known cells; every blob of a shape is known at the same seeded index set (a node lacks the same columns of every
blob of a block) and wants its 128 - known missing cells, ascending.  Per shape the three sides alternate: --warmup rounds, then --reps timed
rounds; ms per call as median (min-max).  Every cell and proof of the new call, and every proof of (b), is compared with (a)'s at the same
index.  Kernel ms by family come from the library's event timing, one extra call per shape.  The C entry points get preallocated buffers, so
no figure holds Python object construction; the MSM table build and the first call of every kind happen before any timed call.  Handles
(--handles): "default" (the table sized from the free memory) and "bucket" (msm_bits = 8).  The shader clock is sampled from the card's hwmon
files over the timed calls (best effort).
Run:  python tools/exp_recover_at.py [--reps 7] [--warmup 2] [--shapes 1x120,6x120,...] [--handles default,bucket]"""
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

try:
    import torch                        # noqa: F401 -- before the library, so that both bind one HIP runtime (the clock sampler uses it)
except Exception:                       # noqa: BLE001
    pass
from bench import PowerSampler         # noqa: E402
from kzg_rust_amd import _lib          # noqa: E402
from synth import random_blob          # noqa: E402

NEW = ["rc_vanish", "rc_interp", "rc_columns", "rc_cells_at", "cq_quotient", "digits", "msm_wide", "msm_bucket", "msm_finalize"]
FULL = ["rc_vanish", "rc_interp", "rc_columns", "rc_cells", "cc_columns", "cc_msm", "cc_proofs"]
CELL, ROW, PROOFS, BLOB = 2048, 128 * 2048, 128 * 48, 131072


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def spread(s):
    return s["ms_max"] - s["ms_min"]


def timed(f):
    t = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1x120,6x120,21x120,128x120,6x64,128x64")
    ap.add_argument("--handles", default="default,bucket")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    lib = _lib.load()
    sz, vp = C.c_size_t, C.c_void_p
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    nmax = max(n for n, _ in shapes)
    blobs = b"".join(random_blob(75940 + i) for i in range(nmax))
    full_c, full_p = C.create_string_buffer(ROW * nmax), C.create_string_buffer(PROOFS * nmax)      # (a)
    mid_c, mid_blobs, mid_p = C.create_string_buffer(ROW * nmax), C.create_string_buffer(BLOB * nmax), C.create_string_buffer(PROOFS * nmax)   # (b)
    new_c, new_p = C.create_string_buffer(ROW * nmax), C.create_string_buffer(PROOFS * nmax)
    st = (C.c_int * nmax)()
    print(json.dumps({"reps": a.reps, "warmup": a.warmup}), flush=True)
    for name in a.handles.split(","):
        opt = _lib.Options()
        lib.kzg355_options_default(C.byref(opt))
        if name == "bucket":
            opt.msm_bits = 8
        h = vp()
        assert lib.kzg355_load_trusted_setup_ex(g1, 4096, g2, 65, None, 0, C.byref(opt), C.byref(h)) == 0
        t_build = timed(lambda: lib.kzg355_settings_build_msm_table(h))
        kernel_ms = lambda fams: {f: round(v, 3) for f in fams for v in [lib.kzg355_last_kernel_ms(h, f.encode())] if v >= 0}     # noqa: E731
        # the blobs' 128 cells (the input of every shape), and the first call of every kind
        all_cells = C.create_string_buffer(ROW * nmax)
        assert lib.kzg355_compute_cells_and_kzg_proofs_many(all_cells, full_p, st, blobs, nmax, h) == 0
        src = all_cells.raw
        first = (sz * 64)(*range(64))
        assert lib.kzg355_recover_cells_and_kzg_proofs_many_sets(full_c, full_p, st, (sz * 1)(64), first, src, 1, h) == 0
        assert lib.kzg355_compute_cell_kzg_proofs_at_many(None, mid_p, st, blobs, 1, (sz * 1)(1), (sz * 1)(0), h) == 0
        assert lib.kzg355_recover_cells_and_kzg_proofs_at_many_sets(new_c, new_p, st, (sz * 1)(64), first, src, (sz * 1)(1), (sz * 1)(64), 1, h) == 0
        print(json.dumps({"handle": name, "msm_form": lib.kzg355_settings_msm_form(h), "table_build_ms": round(t_build, 1)}), flush=True)
        sampler = PowerSampler(lib.kzg355_settings_device(h))
        sampler.start()
        for n, known in shapes:
            ix = sorted(random.Random(1000 * n + known).sample(range(128), known))
            want = [k for k in range(128) if k not in ix]
            w = len(want)
            cells = b"".join(src[ROW * b + CELL * k:ROW * b + CELL * (k + 1)] for b in range(n) for k in ix)
            kc, ki = (sz * n)(*([known] * n)), (sz * (n * known))(*(ix * n))
            wc, wi = (sz * n)(*([w] * n)), (sz * (n * w))(*(want * n))

            def full():
                assert lib.kzg355_recover_cells_and_kzg_proofs_many_sets(full_c, full_p, st, kc, ki, cells, n, h) == 0

            def composed():
                assert lib.kzg355_recover_cells_and_kzg_proofs_many_sets(mid_c, None, st, kc, ki, cells, n, h) == 0
                for b in range(n):
                    C.memmove(C.byref(mid_blobs, BLOB * b), C.byref(mid_c, ROW * b), BLOB)
                assert lib.kzg355_compute_cell_kzg_proofs_at_many(None, mid_p, st, mid_blobs, n, wc, wi, h) == 0

            def new():
                assert lib.kzg355_recover_cells_and_kzg_proofs_at_many_sets(new_c, new_p, st, kc, ki, cells, wc, wi, n, h) == 0

            for _ in range(a.warmup):
                full(); composed(); new()
            t_full, t_comp, t_new = [], [], []
            for _ in range(a.reps):
                t_full.append(timed(full))
                t_comp.append(timed(composed))
                t_new.append(timed(new))
            fc, fp, gc, gp, mp = full_c.raw, full_p.raw, new_c.raw, new_p.raw, mid_p.raw
            for b in range(n):
                for j, k in enumerate(want):
                    s = w * b + j
                    assert gc[CELL * s:CELL * (s + 1)] == fc[ROW * b + CELL * k:ROW * b + CELL * (k + 1)], (n, known, b, k)
                    assert gp[48 * s:48 * (s + 1)] == mp[48 * s:48 * (s + 1)] == fp[PROOFS * b + 48 * k:PROOFS * b + 48 * (k + 1)], (n, known, b, k)
            lib.kzg355_reset_kernel_stats(h)
            lib.kzg355_set_kernel_timing(h, 1)
            new()
            k_new = kernel_ms(NEW)
            lib.kzg355_reset_kernel_stats(h)
            full()
            k_full = kernel_ms(FULL)
            lib.kzg355_set_kernel_timing(h, 0)
            sf, sc, sn = stats(t_full), stats(t_comp), stats(t_new)
            print(json.dumps({"handle": name, "blobs": n, "known": known, "wanted_per_blob": w, "recover_at": sn, "full_recover": sf, "composed": sc,
                              "gain_over_full_ms": round(sf["ms_median"] - sn["ms_median"], 3),
                              "spreads_new_and_full_ms": round(spread(sn) + spread(sf), 3),
                              "gain_over_composed_ms": round(sc["ms_median"] - sn["ms_median"], 3),
                              "spreads_new_and_composed_ms": round(spread(sn) + spread(sc), 3),
                              "recover_at_kernel_ms": k_new, "full_recover_kernel_ms": k_full}), flush=True)
        clk = sampler.stop()
        print(json.dumps({"handle": name, "clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}}), flush=True)
        lib.kzg355_free_trusted_setup(h)


if __name__ == "__main__":
    main()
