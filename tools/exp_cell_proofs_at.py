#!/usr/bin/env python3
"""Cost of kzg355_compute_cell_kzg_proofs_at_many (the proofs of chosen cells, one quotient and one MSM per pair) next to the call that was the
only way to a cell proof before it, kzg355_compute_cells_and_kzg_proofs_many (FK20, always 128 proofs per blob), in one process on seeded blobs.
Both calls return proofs only.  Shapes (--shapes): blobs x indices per blob; every blob asks for its first k indices of one seeded permutation
of 0..127.  Per shape the two calls alternate: --warmup rounds, then --reps timed rounds; ms per call as median (min-max).  Every proof of the
new call is compared with the yardstick's at the same index.  Kernel ms by family come from the library's event timing, one extra call per
shape.  The C entry points get preallocated buffers, so no figure holds Python object construction; the MSM table build and the first call of
either kind happen before any timed call.  Handles (--handles): "default" (the table sized from the free memory) and "bucket" (msm_bits = 8).
The shader clock is sampled from the card's hwmon files over the timed calls (best effort).
Run:  python tools/exp_cell_proofs_at.py [--reps 7] [--warmup 2] [--shapes 1x1,1x8,...] [--handles default,bucket]"""
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

NEW = ["cc_field", "cq_quotient", "digits", "msm_wide", "msm_bucket", "msm_finalize"]
OLD = ["cc_field", "cc_columns", "cc_msm", "cc_proofs"]
PROOFS_B = 128 * 48


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def timed(f):
    t = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1x1,1x8,1x128,6x8,6x128,128x8,128x128")
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
    order = random.Random(7594).sample(range(128), 128)
    ref_p, out_p = C.create_string_buffer(PROOFS_B * nmax), C.create_string_buffer(PROOFS_B * nmax)
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
        one = (sz * 1)(1)
        assert lib.kzg355_compute_cells_and_kzg_proofs_many(None, ref_p, st, blobs, 1, h) == 0                 # the proof setup of FK20
        assert lib.kzg355_compute_cell_kzg_proofs_at_many(None, out_p, st, blobs, 1, one, (sz * 1)(0), h) == 0   # the first call of the new kind
        print(json.dumps({"handle": name, "msm_form": lib.kzg355_settings_msm_form(h), "table_build_ms": round(t_build, 1)}), flush=True)
        sampler = PowerSampler(lib.kzg355_settings_device(h))
        sampler.start()
        for n, k in shapes:
            ix = order[:k]
            counts, idx = (sz * n)(*([k] * n)), (sz * (n * k))(*(ix * n))

            def old():
                assert lib.kzg355_compute_cells_and_kzg_proofs_many(None, ref_p, st, blobs, n, h) == 0

            def new():
                assert lib.kzg355_compute_cell_kzg_proofs_at_many(None, out_p, st, blobs, n, counts, idx, h) == 0

            for _ in range(a.warmup):
                old(); new()
            t_old, t_new = [], []
            for _ in range(a.reps):
                t_old.append(timed(old))
                t_new.append(timed(new))
            got, ref = out_p.raw, ref_p.raw
            for b in range(n):
                for j, c in enumerate(ix):
                    assert got[48 * (k * b + j):48 * (k * b + j + 1)] == ref[PROOFS_B * b + 48 * c:PROOFS_B * b + 48 * (c + 1)], (n, k, b, c)
            lib.kzg355_reset_kernel_stats(h)
            lib.kzg355_set_kernel_timing(h, 1)
            new()
            k_new = kernel_ms(NEW)
            lib.kzg355_reset_kernel_stats(h)
            old()
            k_old = kernel_ms(OLD)
            lib.kzg355_set_kernel_timing(h, 0)
            so, sn = stats(t_old), stats(t_new)
            print(json.dumps({"handle": name, "blobs": n, "indices_per_blob": k, "proofs_at": sn, "fk20_many": so,
                              "ratio_new_over_old": round(sn["ms_median"] / so["ms_median"], 3),
                              "gain_ms": round(so["ms_median"] - sn["ms_median"], 3),
                              "sum_of_spreads_ms": round(so["ms_max"] - so["ms_min"] + sn["ms_max"] - sn["ms_min"], 3),
                              "proofs_at_kernel_ms": k_new, "fk20_kernel_ms": k_old}), flush=True)
        clk = sampler.stop()
        print(json.dumps({"handle": name, "clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}}), flush=True)
        lib.kzg355_free_trusted_setup(h)


if __name__ == "__main__":
    main()
