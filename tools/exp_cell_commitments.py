#!/usr/bin/env python3
"""What the commitment output of the FK20 chain costs, measured against another build of the library on one card.

The driver starts one child process per build, the two builds alternating (--rounds times each), so that neither side owns the warmer or the
cooler part of the job.  A child loads its library with plain ctypes (an older build lacks the new entry points, so the package's loader cannot
bind it), makes a default handle and times, at every n of --sizes, with preallocated buffers around the synchronous C entry point:
  * old:        kzg355_compute_cells_and_kzg_proofs_many, cells and proofs (both builds);
  * all:        kzg355_compute_commitments_cells_and_kzg_proofs_many, all three outputs (builds that have it);
  * commit:     the same call, commitments only (the chain ends after the inverse G1 transform);
  * pair:       kzg355_blob_to_kzg_commitment_many followed by the old call -- what the all-outputs call replaces (after the handle's
                MSM table is built and the commitment path has run once).
Per variant: ms per call as median, min and max of --reps timed calls after --warmup, and the `cc_proofs` family of one more call with the
library's event timing on.  The all-outputs commitments are checked against blob_to_kzg_commitment_many, the cells and proofs against the old
call.  One JSON line per (build, round, n), then a summary line per (build, n) over the rounds.
Run:  python tools/exp_cell_commitments.py --other /path/to/other/libkzg355.so [--rounds 2] [--reps 5] [--warmup 1] [--sizes 1,128,512]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOB, CELLS_B, PROOFS_B = 131072, 128 * 2048, 128 * 48


def child(a):
    lib = C.CDLL(a.child)
    vp, sz, u8p, ip = C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int)
    lib.kzg355_load_trusted_setup.argtypes = [u8p, sz, u8p, sz, C.POINTER(vp)]
    lib.kzg355_free_trusted_setup.argtypes = [vp]
    lib.kzg355_free_trusted_setup.restype = None
    lib.kzg355_compute_cells_and_kzg_proofs_many.argtypes = [u8p, u8p, ip, u8p, sz, vp]
    lib.kzg355_blob_to_kzg_commitment_many.argtypes = [u8p, ip, u8p, sz, vp]
    lib.kzg355_set_kernel_timing.argtypes = [vp, C.c_int]
    lib.kzg355_set_kernel_timing.restype = None
    lib.kzg355_last_kernel_ms.argtypes = [vp, u8p]
    lib.kzg355_last_kernel_ms.restype = C.c_double
    new = hasattr(lib, "kzg355_compute_commitments_cells_and_kzg_proofs_many")
    if new:
        lib.kzg355_compute_commitments_cells_and_kzg_proofs_many.argtypes = [u8p, u8p, u8p, ip, u8p, sz, vp]
    g = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read()
    h = vp()
    assert lib.kzg355_load_trusted_setup(g1, 4096, g2, 65, C.byref(h)) == 0
    sizes = [int(x) for x in a.sizes.split(",")]
    nmax = max(sizes)
    blobs = open(a.blobs, "rb").read()
    assert len(blobs) >= BLOB * nmax
    cells, proofs, coms, coms2 = (C.create_string_buffer(k * nmax) for k in (CELLS_B, PROOFS_B, 48, 48))
    cells2, proofs2 = C.create_string_buffer(CELLS_B * nmax), C.create_string_buffer(PROOFS_B * nmax)
    st = (C.c_int * nmax)()

    def good(rc, n):
        assert rc == 0 and not any(st[i] for i in range(n)), rc

    variants = {"old": lambda n: good(lib.kzg355_compute_cells_and_kzg_proofs_many(cells, proofs, st, blobs, n, h), n)}
    if new:
        def pair(n):
            good(lib.kzg355_blob_to_kzg_commitment_many(coms2, st, blobs, n, h), n)
            good(lib.kzg355_compute_cells_and_kzg_proofs_many(cells, proofs, st, blobs, n, h), n)
        variants["all"] = lambda n: good(lib.kzg355_compute_commitments_cells_and_kzg_proofs_many(coms, cells2, proofs2, st, blobs, n, h), n)
        variants["commit"] = lambda n: good(lib.kzg355_compute_commitments_cells_and_kzg_proofs_many(coms, None, None, st, blobs, n, h), n)
        variants["pair"] = pair
        pair(nmax)                                                  # the MSM table and the commitment path's first call: not timed
    variants["old"](1)                                              # the proof setup: not timed
    for n in sizes:
        row = {"build": a.label, "round": a.round, "n": n}
        for name, fn in variants.items():
            for _ in range(a.warmup):
                fn(n)
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                fn(n)
                ts.append(1e3 * (time.perf_counter() - t))
            lib.kzg355_set_kernel_timing(h, 1)
            fn(n)
            k = lib.kzg355_last_kernel_ms(h, b"cc_proofs")
            lib.kzg355_set_kernel_timing(h, 0)
            row[name] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "cc_proofs_ms": round(k, 3)}
        if new:
            assert coms.raw[:48 * n] == coms2.raw[:48 * n], n
            assert cells2.raw[:CELLS_B * n] == cells.raw[:CELLS_B * n] and proofs2.raw[:PROOFS_B * n] == proofs.raw[:PROOFS_B * n], n
        print(json.dumps(row), flush=True)
    lib.kzg355_free_trusted_setup(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the build to compare with (libkzg355.so of the parent commit)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1,128,512")
    ap.add_argument("--child")
    ap.add_argument("--label")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--blobs")
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from synth import random_blob
    nmax = max(int(x) for x in a.sizes.split(","))
    builds = ([("other", a.other)] if a.other else []) + [("this", os.path.join(ROOT, "kzg_rust_amd", "libkzg355.so"))]
    rows = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "blobs.bin")
        with open(path, "wb") as f:
            for i in range(nmax):
                f.write(random_blob(50000 + i))
        for r in range(a.rounds):
            for label, lib in builds:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--label", label, "--round", str(r), "--blobs", path,
                                      "--reps", str(a.reps), "--warmup", str(a.warmup), "--sizes", a.sizes], capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    print(out.stdout, out.stderr, sep="\n", flush=True)
                    return 1                                        # nothing more is started after a failed child
                for ln in out.stdout.splitlines():
                    print(ln, flush=True)
                    rows.append(json.loads(ln))
    for label, _ in builds:
        for n in sorted({r["n"] for r in rows}):
            mine = [r for r in rows if r["build"] == label and r["n"] == n]
            line = {"summary": label, "n": n}
            for v in ("old", "all", "commit", "pair"):
                if all(v in r for r in mine):
                    line[v] = {"ms_median": round(statistics.median(r[v]["ms_median"] for r in mine), 3), "ms_min": min(r[v]["ms_min"] for r in mine),
                               "ms_max": max(r[v]["ms_max"] for r in mine), "cc_proofs_ms": round(statistics.median(r[v]["cc_proofs_ms"] for r in mine), 3)}
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
