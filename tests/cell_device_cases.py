"""Inputs shared by tests/test_gpu_cell_device.py (GPU) and tests/test_cell_device_abi.py (CPU): the cell fixture, the batches the verdict tests
run, and the seeded generator of the differential fuzz with the kind every group is meant to be, so that a machine without a GPU can still
check that the generator draws what it says (nothing silently dropped)."""
import json
import os
import random

import cell_spec as cs
from synth import random_blob

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R
FUZZ_SEED = 0x7594D
FUZZ_SHAPES = ((1, 60), (2, 50), (6, 40), (16, 30), (64, 16), (128, 8))     # (cells per group, groups): 204 groups


def fixture():
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    blobs = [random_blob(s) for s in d["blob_seeds"]]
    d["blobs"] = blobs
    d["cells"] = [cs.compute_cells(b) for b in blobs]
    d["C"] = [bytes.fromhex(c) for c in d["commitments"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    return d


def batch(fx, items):
    return [fx["C"][b] for b, _ in items], [k for _, k in items], [fx["cells"][b][k] for b, k in items], [fx["P"][b][k] for b, k in items]


def off_curve(oracle):
    for x in range(1, 1000):
        b = bytearray(x.to_bytes(48, "big")); b[0] |= 0x80
        if oracle.g1_uncompress_only(bytes(b)) != 0:
            return bytes(b)


def not_in_subgroup(oracle):
    for x in range(1, 1000):
        b = bytearray(x.to_bytes(48, "big")); b[0] |= 0x80
        if oracle.g1_uncompress_only(bytes(b)) == 0 and oracle.g1_validate(bytes(b)) != 0:
            return bytes(b)


def fuzz_groups(fx, bad_point):
    """[(npg, [(group, kind)])]: kind is "valid", "tampered" (well-formed, may still verify when the mutation is a no-op) or "malformed"
    (BadArgs).  Within a group a cell repeats an earlier cell's blob with probability about 1/3, so duplicate commitments are everywhere and
    in every order of first appearance."""
    rng = random.Random(FUZZ_SEED)
    out = []
    for npg, count in FUZZ_SHAPES:
        groups = []
        for _ in range(count):
            items = []
            for k in range(npg):
                b = items[rng.randrange(k)][0] if k and rng.random() < 1 / 3 else rng.randrange(3)
                items.append((b, rng.randrange(128)))
            c, i, cl, p = [list(x) for x in batch(fx, items)]
            m, k = rng.randrange(10), rng.randrange(npg)
            kind = "valid"
            if m == 1 and npg > 1:
                p[k], p[(k + 1) % npg] = p[(k + 1) % npg], p[k]; kind = "tampered"
            elif m == 2:
                j = rng.randrange(64)
                cl[k] = cl[k][:32 * j] + rng.randrange(R).to_bytes(32, "big") + cl[k][32 * j + 32:]; kind = "tampered"
            elif m == 3:
                i[k] = rng.randrange(128); kind = "tampered"
            elif m == 4:
                c[k] = fx["C"][rng.randrange(3)]; kind = "tampered"
            elif m == 5:
                i[k] = 128 + rng.randrange(1 << 40); kind = "malformed"
            elif m == 6:
                j = rng.randrange(64)
                cl[k] = cl[k][:32 * j] + (R + rng.randrange(2 ** 255 - R)).to_bytes(32, "big") + cl[k][32 * j + 32:]; kind = "malformed"
            elif m == 7:
                if rng.random() < 0.5:
                    c[k] = bad_point
                else:
                    p[k] = bad_point
                kind = "malformed"
            groups.append(((c, i, cl, p), kind))
        out.append((npg, groups))
    return out


def well_formed(oracle, group):
    """what cell_spec's argument checks say about a group, without the (slow) check itself"""
    c, i, cl, p = group
    if any(int(x) >= cs.CELLS_PER_EXT_BLOB for x in i):
        return False
    if any(oracle.g1_validate(b) != 0 for b in set(c) | set(p)):
        return False
    try:
        for cell in cl:
            cs.cell_values(cell)
    except cs.BadArgs:
        return False
    return True
