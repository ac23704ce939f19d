#!/usr/bin/env python3
"""Fixtures for the EIP-7594 cell path (kzg355_verify_cell_kzg_proof_batch).

ORACLE-derived ("self-golden"): there are no published cell vectors in the reference, so these come from tests/cell_spec.py (Python integers
+ the C oracle's g1_lincomb / pairings_verify) and are checked before anything is written:
  * setup_g1_monomial.bin: the 4096 MONOMIAL points [tau^t]G1 of the reference's data file testing_trusted_setups.json ("setup_G1"; data, not
    source; read only when --monomial-from is given), the same ceremony as trusted_setup_g1.bin (its "setup_G1_lagrange");
  * cells.json: seeded blobs (synth.random_blob, recomputed by the tests), their commitments, all 128 cell proofs of each, and a few batches with
    their challenge r, [I(tau)]_1, LL and RL.  Cells are recomputed from the blobs (compute_cells), not stored.
Checks: monomial point t equals the oracle's commitment of the blob (w_i^t)_i for t < 64; cells 0..63 equal the blob; the single-cell pairing
holds for a sample of cells; every batch verifies.
Run from the repo root:  python tests/golden/make_cell_fixtures.py [--monomial-from <testing_trusted_setups.json>]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_spec as cs                              # noqa: E402
from oracle import pyref                           # noqa: E402
from oracle.oracle import Oracle                   # noqa: E402
from synth import random_blob                      # noqa: E402

R = pyref.R
BLOB_SEEDS = [7594, 7595, 7596]


def setup(o):
    g1 = open(os.path.join(HERE, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(HERE, "trusted_setup_g2.bin"), "rb").read()
    return o.load_trusted_setup(g1, g2)


def batches():
    """(name, [(blob number, cell index)]) of the fixture batches"""
    return [
        ("one_cell", [(0, 5)]),
        ("column", [(b, 77) for b in range(len(BLOB_SEEDS))]),
        ("row", [(1, k) for k in range(128)]),
        ("mixed", [(0, 3), (2, 100), (0, 3), (1, 64), (0, 127), (2, 0), (1, 64), (2, 100)]),
    ]


def build(o, so, mono):
    blobs = [random_blob(s) for s in BLOB_SEEDS]
    commitments = [o.blob_to_kzg_commitment(b, so) for b in blobs]
    proofs = [cs.cell_proofs(o, b, mono) for b in blobs]
    out = {"note": "oracle-derived (tests/cell_spec.py + the C oracle); blobs are synth.random_blob(seed), cells recomputed with compute_cells",
           "blob_seeds": BLOB_SEEDS, "commitments": [c.hex() for c in commitments], "proofs": [[p.hex() for p in ps] for ps in proofs], "batches": []}
    cells = [cs.compute_cells(b) for b in blobs]
    for name, items in batches():
        args = ([commitments[b] for b, _ in items], [k for _, k in items], [cells[b][k] for b, k in items], [proofs[b][k] for b, k in items])
        ok, im = cs.verify_cell_kzg_proof_batch(o, *args, mono=mono, intermediates=True)
        assert ok, name
        out["batches"].append({"name": name, "items": items, "r": im["r"].hex(), "itau": im["itau"].hex(), "ll": im["ll"].hex(), "rl": im["rl"].hex()})
    return out, blobs, cells, commitments, proofs


def main():
    mono_path = os.path.join(HERE, "setup_g1_monomial.bin")
    if "--monomial-from" in sys.argv:
        ref = json.load(open(sys.argv[sys.argv.index("--monomial-from") + 1]))
        mono = [bytes.fromhex(x[2:]) for x in ref["setup_G1"]]
        assert len(mono) == 4096
        assert b"".join(bytes.fromhex(x[2:]) for x in ref["setup_G1_lagrange"]) == open(os.path.join(HERE, "trusted_setup_g1.bin"), "rb").read()
        assert b"".join(mono[:4]) == open(os.path.join(HERE, "setup_g1_monomial_first4.bin"), "rb").read()
        open(mono_path, "wb").write(b"".join(mono))
    mono = cs.load_monomial()
    o = Oracle()
    so = setup(o)
    roots = [int.from_bytes(o.roots_of_unity(so)[32 * i:32 * i + 32], "big") for i in range(4096)]
    for t in list(range(4)) + [31, 63]:
        blob = b"".join(pow(x, t, R).to_bytes(32, "big") for x in roots)
        assert o.blob_to_kzg_commitment(blob, so) == mono[t], f"monomial point {t}"
    out, blobs, cells, commitments, proofs = build(o, so, mono)
    for b, cl in zip(blobs, cells):
        assert b"".join(cl[:64]) == b, "cells 0..63 are the blob"
    for b in range(len(blobs)):
        for k in (0, 5, 64, 127):
            assert cs.single_cell_check(o, commitments[b], k, cells[b][k], proofs[b][k], mono=mono), (b, k)
    json.dump(out, open(os.path.join(HERE, "cells.json"), "w"), indent=0)
    o.free_trusted_setup(so)
    print("wrote cells.json:", len(out["batches"]), "batches")


if __name__ == "__main__":
    main()
