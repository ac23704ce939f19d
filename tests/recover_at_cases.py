"""The units and expected answers of tests/test_gpu_cell_recover_at.py (recover_cells_and_kzg_proofs_at), built once
and pinned on the CPU by tests/test_recover_at_cases.py.  A unit is (cell_indices, cells, want_indices).  Expected cells come from
cell_spec.compute_cells and expected proofs from tests/golden/cells.json (oracle-derived), never from the calls under test; the inconsistent
unit's expected cells come from the specs' route (recover_spec.recover_coefficients_spec) and its proofs are left to the full recovery call
of the parent commit."""
import functools
import json
import os
import random

import cell_spec as cs
import fk20_spec as fk
import recover_spec as rs
from synth import random_blob

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R
CELLS = cs.CELLS_PER_EXT_BLOB
FIXED = [0, 1, 63, 64, 127, 5, 5]                                 # known and missing, unordered, repeated
WANT_KINDS = ("missing", "fixed", "shuffled")


@functools.lru_cache(maxsize=None)
def fixture():
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    d["blobs"] = [random_blob(s) for s in d["blob_seeds"]]
    d["cells"] = [cs.compute_cells(b) for b in d["blobs"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    return d


def index_sets():
    """the nine shapes of tests/test_gpu_cell_recover_sets.py::index_sets, restated"""
    rng = random.Random(7594)
    return [("first64", list(range(64))), ("last64", list(range(64, 128))), ("odd", list(range(1, 128, 2))), ("even", list(range(0, 128, 2))),
            ("random64", sorted(rng.sample(range(128), 64))), ("random65", sorted(rng.sample(range(128), 65))),
            ("random100", sorted(rng.sample(range(128), 100))), ("127cells", sorted(rng.sample(range(128), 127))), ("all128", list(range(128)))]


def missing(ix):
    known = set(ix)
    return [k for k in range(CELLS) if k not in known]


def unit(b, ix, want):
    """fixture blob b known at ix, asking for want"""
    cells = fixture()["cells"][b]
    return (list(ix), [cells[k] for k in ix], list(want))


def expected(b, want):
    """(cells, proofs) of fixture blob b at want"""
    fx = fixture()
    return [fx["cells"][b][k] for k in want], [fx["P"][b][k] for k in want]


def flat(exp):
    """the two output buffers of a call whose units have the answers exp: (cells_out bytes, proofs_out bytes)"""
    return b"".join(b"".join(c) for c, _ in exp), b"".join(b"".join(p) for _, p in exp)


# ---- 1. the nine index-set shapes as nine units of one call over the three fixture blobs
@functools.lru_cache(maxsize=None)
def nine(kind):
    """(units, expected per unit): every unit wants its own missing cells, ascending (all128: none); FIXED; or all 128 in a shuffled order"""
    assert kind in WANT_KINDS
    units, exp = [], []
    for j, (_, ix) in enumerate(index_sets()):
        want = missing(ix) if kind == "missing" else FIXED if kind == "fixed" else random.Random(128 + j).sample(range(CELLS), CELLS)
        units.append(unit(j % 3, ix, want))
        exp.append(expected(j % 3, want))
    return units, exp


# ---- 3. a refused blob between two good ones, once per per-blob refusal
def _spoil(cells, at=3):
    """r itself in the first element of cell `at`"""
    out = list(cells)
    out[at] = R.to_bytes(32, "big") + out[at][32:]
    return out


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, units, statuses (1 = BADARGS), expected of the two neighbours)]: unit 1 is refused, units 0 and 2 are good and their slots
    sit where the counts as given put them.  The last two: a unit that wants nothing shifts nothing and is still checked."""
    sets = dict(index_sets())
    cells = fixture()["cells"]
    left, right = unit(1, sets["random65"], [64, 2]), unit(2, sets["127cells"], [127, 0, 9])
    e_left, e_right = expected(1, [64, 2]), expected(2, [127, 0, 9])
    ok_ix = sets["random100"]
    ok_cells = [cells[0][k] for k in ok_ix]
    mids = {
        "63 known cells": (list(range(63)), [cells[0][k] for k in range(63)], [5, 6, 7]),
        "129 known cells": (list(range(128)) + [128], [cells[0][k % 128] for k in range(129)], [5, 6, 7]),
        "known index 128": (list(range(63)) + [128], [cells[0][k] for k in range(64)], [5, 6, 7]),
        "known indices not ascending": (list(range(62)) + [70, 69], [cells[0][k] for k in list(range(62)) + [70, 69]], [5, 6, 7]),
        "cell element >= r": (ok_ix, _spoil(ok_cells), [5, 6, 7]),
        "wanted index 128": (ok_ix, ok_cells, [5, 128, 7]),
        "129 wanted": (ok_ix, ok_cells, [i % 128 for i in range(129)]),
    }
    out = [(name, [left, mid, right], [0, 1, 0], [e_left, e_right]) for name, mid in mids.items()]
    out.append(("nothing wanted", [left, (ok_ix, ok_cells, []), right], [0, 0, 0], [e_left, e_right]))
    out.append(("nothing wanted, spoiled", [left, (ok_ix, _spoil(ok_cells), []), right], [0, 1, 0], [e_left, e_right]))
    return out


# ---- 4. more than 64 cells that lie on no polynomial of degree < 4096, next to a consistent unit
INCONSISTENT_WANT = [0, 1, 63, 64, 127, 5, 5, 30, 31]            # 30 is known (and is the changed cell), 0 and 127 are missing


@functools.lru_cache(maxsize=None)
def inconsistent():
    """(units, the changed unit's 4096 coefficients by the specs' route, its expected cells at INCONSISTENT_WANT, the good unit's expected):
    unit 0 is 65 cells of fixture blob 2 with one bit of one element changed, unit 1 a consistent neighbour"""
    fx = fixture()
    ix = list(range(30, 95))
    bad = [fx["cells"][2][k] for k in ix]
    t = bytearray(bad[0])
    t[31] ^= 1
    bad[0] = bytes(t)
    f = rs.recover_coefficients_spec(ix, bad)
    full = cs.compute_cells(fk.blob_from_coefficients(f))
    good_ix = dict(index_sets())["random64"]
    units = [(ix, bad, list(INCONSISTENT_WANT)), unit(0, good_ix, missing(good_ix))]
    return units, f, [full[k] for k in INCONSISTENT_WANT], expected(0, missing(good_ix))
