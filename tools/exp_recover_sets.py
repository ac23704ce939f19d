#!/usr/bin/env python3
"""Cost of kzg355_recover_cells_and_kzg_proofs_many_sets (every blob with its own index set) next to the shared-set call it generalises, in
one process on seeded blobs.  Legs (--legs):
  * bulk: 32 sets x 6 blobs (a node catching up on 32 blocks of six blobs, each block known at its own 64..100 random columns), as ONE
    many_sets call and as 32 calls of kzg355_recover_cells_and_kzg_proofs_many, alternating; cells only and with proofs.  The sequence of
    existing calls is the yardstick.  Outputs are compared.
  * shared: m = 128 blobs at one set of 64 cells through the existing kzg355_recover_cells_and_kzg_proofs_many, cells only and with proofs,
    with the kernel ms of the recovery's own stage.  Run it once per build (--library) to compare two builds on one box.
  * vanish: rc_vanish kernel ms with 1, 32 and 512 distinct sets in one chunk of 512 blobs (cells only).
ms per call as median (min-max) of --reps timed calls after --warmup.  Kernel ms come from the library's event timing, one extra call per
shape.  The C entry points get preallocated buffers, so no figure holds Python object construction.  The library is bound with ctypes here
(not through the package), so that a build without the new entry points can run the shared leg.  The shader clock is sampled from the
card's hwmon files over the timed calls (best effort).
Run:  python tools/exp_recover_sets.py [--reps 7] [--warmup 2] [--legs bulk,shared,vanish] [--library PATH]"""
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
from synth import random_blob          # noqa: E402

RC = ["rc_vanish", "rc_interp", "rc_columns", "rc_cells"]
CC = ["cc_columns", "cc_msm", "cc_proofs"]
CELL_B, CELLS_B, PROOFS_B = 2048, 128 * 2048, 128 * 48


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
    ap.add_argument("--legs", default="bulk,shared,vanish")
    ap.add_argument("--library", default=os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so"))
    a = ap.parse_args()
    legs = a.legs.split(",")
    lib = C.CDLL(a.library)
    lib.kzg355_last_kernel_ms.restype = C.c_double
    lib.kzg355_last_kernel_ms.argtypes = [C.c_void_p, C.c_char_p]
    lib.kzg355_set_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    lib.kzg355_set_kernel_timing.restype = None
    lib.kzg355_settings_device.argtypes = [C.c_void_p]
    sz, vp = C.c_size_t, C.c_void_p
    lib.kzg355_load_trusted_setup.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(vp)]
    lib.kzg355_compute_cells_and_kzg_proofs_many.argtypes = [vp, vp, vp, C.c_char_p, sz, vp]
    lib.kzg355_recover_cells_and_kzg_proofs_many.argtypes = [vp, vp, vp, vp, C.c_char_p, sz, sz, vp]
    have_sets = hasattr(lib, "kzg355_recover_cells_and_kzg_proofs_many_sets")
    if have_sets:
        lib.kzg355_recover_cells_and_kzg_proofs_many_sets.argtypes = [vp, vp, vp, vp, vp, C.c_char_p, sz, vp]
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    h = vp()
    assert lib.kzg355_load_trusted_setup(g1, 4096, g2, 65, C.byref(h)) == 0
    kernel_ms = lambda fams: {f: round(lib.kzg355_last_kernel_ms(h, f.encode()), 3) for f in fams}
    mmax = 512 if "vanish" in legs else 192
    blobs = b"".join(random_blob(60000 + i) for i in range(mmax))
    full = C.create_string_buffer(CELLS_B * mmax)
    warm_p = C.create_string_buffer(PROOFS_B)
    st = (C.c_int * mmax)()
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(full, None, st, blobs, mmax, h) == 0
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(None, warm_p, st, blobs, 1, h) == 0       # the proof setup of the handle
    full = full.raw
    pick = lambda b, ix: b"".join(full[CELLS_B * b + CELL_B * k:CELLS_B * b + CELL_B * (k + 1)] for k in ix)
    out_c, out_p = C.create_string_buffer(CELLS_B * mmax), C.create_string_buffer(PROOFS_B * mmax)
    ref_c, ref_p = C.create_string_buffer(CELLS_B * mmax), C.create_string_buffer(PROOFS_B * mmax)
    print(json.dumps({"library": os.path.relpath(a.library, ROOT), "many_sets": have_sets, "reps": a.reps, "warmup": a.warmup}), flush=True)
    sampler = PowerSampler(lib.kzg355_settings_device(h))
    sampler.start()

    def sets_call(counts, idx, data, m, proofs):
        rc = lib.kzg355_recover_cells_and_kzg_proofs_many_sets(out_c, out_p if proofs else None, st, counts, idx, data, m, h)
        assert rc == 0 and not any(st[i] for i in range(m)), rc

    if "bulk" in legs and have_sets:
        rng = random.Random(7594)
        B, PER = 32, 6
        sets = [sorted(rng.sample(range(128), rng.randint(64, 100))) for _ in range(B)]
        m = B * PER
        counts = (sz * m)(*[len(sets[b // PER]) for b in range(m)])
        flat = [i for b in range(m) for i in sets[b // PER]]
        idx = (sz * len(flat))(*flat)
        data = b"".join(pick(b, sets[b // PER]) for b in range(m))
        block_idx = [(sz * len(s))(*s) for s in sets]
        block_data = [b"".join(pick(b, sets[j]) for b in range(PER * j, PER * j + PER)) for j in range(B)]
        ref_cv, ref_pv = (C.c_char * len(ref_c)).from_buffer(ref_c), (C.c_char * len(ref_p)).from_buffer(ref_p)

        def sequence(proofs):
            for j in range(B):
                rc = lib.kzg355_recover_cells_and_kzg_proofs_many(C.byref(ref_cv, CELLS_B * PER * j), C.byref(ref_pv, PROOFS_B * PER * j) if proofs else None,
                                                                  None, block_idx[j], block_data[j], len(sets[j]), PER, h)
                assert rc == 0, (j, rc)

        for proofs in (False, True):
            for _ in range(a.warmup):
                sequence(proofs); sets_call(counts, idx, data, m, proofs)
            t_seq, t_one = [], []
            for _ in range(a.reps):
                t_seq.append(timed(lambda: sequence(proofs)))
                t_one.append(timed(lambda: sets_call(counts, idx, data, m, proofs)))
            assert out_c.raw[:CELLS_B * m] == ref_c.raw[:CELLS_B * m] == full[:CELLS_B * m]
            assert not proofs or out_p.raw[:PROOFS_B * m] == ref_p.raw[:PROOFS_B * m]
            lib.kzg355_set_kernel_timing(h, 1)
            sets_call(counts, idx, data, m, proofs)
            k_one = kernel_ms(RC + CC if proofs else RC)
            lib.kzg355_set_kernel_timing(h, 0)
            so, ss = stats(t_one), stats(t_seq)
            print(json.dumps({"leg": "bulk", "sets": B, "blobs_per_set": PER, "proofs": proofs, "one_many_sets_call": so, "32_many_calls": ss,
                              "factor": round(ss["ms_median"] / so["ms_median"], 2),
                              "gain_ms": round(ss["ms_median"] - so["ms_median"], 3),
                              "sum_of_spreads_ms": round(so["ms_max"] - so["ms_min"] + ss["ms_max"] - ss["ms_min"], 3),
                              "one_call_kernel_ms": k_one}), flush=True)

    if "shared" in legs:
        m, ix = 128, sorted(random.Random(7594).sample(range(128), 64))
        idx = (sz * 64)(*ix)
        data = b"".join(pick(b, ix) for b in range(m))

        def shared(proofs):
            rc = lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, out_p if proofs else None, st, idx, data, 64, m, h)
            assert rc == 0 and not any(st[i] for i in range(m)), rc

        for proofs in (False, True):
            for _ in range(a.warmup):
                shared(proofs)
            ts = [timed(lambda: shared(proofs)) for _ in range(a.reps)]
            assert out_c.raw[:CELLS_B * m] == full[:CELLS_B * m]
            lib.kzg355_set_kernel_timing(h, 1)
            shared(proofs)
            k = kernel_ms(RC)
            lib.kzg355_set_kernel_timing(h, 0)
            print(json.dumps({"leg": "shared", "m": m, "known_cells": 64, "proofs": proofs, "many_call": stats(ts), "kernel_ms": k}), flush=True)

    if "vanish" in legs and have_sets:
        m = 512
        rng = random.Random(512)
        pool = [sorted(rng.sample(range(128), rng.randint(64, 100))) for _ in range(m)]
        assert len({tuple(s) for s in pool}) == m
        for n_sets in (1, 32, 512):
            sets = [pool[b % n_sets] for b in range(m)]
            counts = (sz * m)(*[len(s) for s in sets])
            flat = [i for s in sets for i in s]
            idx = (sz * len(flat))(*flat)
            data = b"".join(pick(b, sets[b]) for b in range(m))
            for _ in range(a.warmup):
                sets_call(counts, idx, data, m, False)
            ts = [timed(lambda: sets_call(counts, idx, data, m, False)) for _ in range(a.reps)]
            assert out_c.raw[:CELLS_B * m] == full[:CELLS_B * m]
            lib.kzg355_set_kernel_timing(h, 1)
            sets_call(counts, idx, data, m, False)
            k = kernel_ms(RC)
            lib.kzg355_set_kernel_timing(h, 0)
            print(json.dumps({"leg": "vanish", "m": m, "sets_in_chunk": n_sets, "call": stats(ts), "kernel_ms": k}), flush=True)

    clk = sampler.stop()
    print(json.dumps({"clock": clk and {"sclk_mhz": clk["sclk_mhz"], "samples": clk["samples"]}}), flush=True)
    lib.kzg355_free_trusted_setup.argtypes = [vp]
    lib.kzg355_free_trusted_setup(h)


if __name__ == "__main__":
    main()
