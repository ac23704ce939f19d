"""CPU (-m "not gpu"): the cell restatement tests/cell_spec.py and its fixtures.  tests/golden/cells.json regenerates from the oracle (commitments,
a sample of the cell proofs, every batch's r / [I(tau)]_1 / LL / RL), the monomial points are the ceremony's, the extension is systematic, the
restatement accepts the valid batches and rejects the tampered / malformed ones; and the public surface (Cell, header constants) is in place."""
import json
import os

import pytest

import cell_spec as cs
from synth import random_blob

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R


@pytest.fixture(scope="module")
def osetup(oracle):
    g = os.path.join(HERE, "golden")
    so = oracle.load_trusted_setup(open(os.path.join(g, "trusted_setup_g1.bin"), "rb").read(), open(os.path.join(g, "trusted_setup_g2.bin"), "rb").read())
    yield so
    oracle.free_trusted_setup(so)


@pytest.fixture(scope="module")
def fx():
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    d["blobs"] = [random_blob(s) for s in d["blob_seeds"]]
    d["cells"] = [cs.compute_cells(b) for b in d["blobs"]]
    d["C"] = [bytes.fromhex(c) for c in d["commitments"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    return d


def batch(fx, items):
    return [fx["C"][b] for b, _ in items], [k for _, k in items], [fx["cells"][b][k] for b, k in items], [fx["P"][b][k] for b, k in items]


def test_monomial_points_are_the_ceremony(oracle, osetup):
    mono = cs.load_monomial()
    assert len(mono) == 4096
    roots = [int.from_bytes(oracle.roots_of_unity(osetup)[32 * i:32 * i + 32], "big") for i in range(4096)]
    for t in (0, 1, 63):
        blob = b"".join(pow(x, t, R).to_bytes(32, "big") for x in roots)
        assert oracle.blob_to_kzg_commitment(blob, osetup) == mono[t]


def test_extension_is_systematic(fx):
    for b, cl in zip(fx["blobs"], fx["cells"]):
        assert len(cl) == 128 and all(len(c) == 2048 for c in cl)
        assert b"".join(cl[:64]) == b


def test_fixtures_regenerate(oracle, osetup, fx):
    mono = cs.load_monomial()
    assert [oracle.blob_to_kzg_commitment(b, osetup) for b in fx["blobs"]] == fx["C"]
    for b in range(len(fx["blobs"])):
        ks = (0, 63, 64, 127) if b == 0 else (b * 37 % 128,)
        assert cs.cell_proofs(oracle, fx["blobs"][b], mono, ks) == [fx["P"][b][k] for k in ks]
    for bt in fx["batches"]:
        ok, im = cs.verify_cell_kzg_proof_batch(oracle, *batch(fx, [tuple(x) for x in bt["items"]]), intermediates=True)
        assert ok, bt["name"]
        assert (im["r"].hex(), im["itau"].hex(), im["ll"].hex(), im["rl"].hex()) == (bt["r"], bt["itau"], bt["ll"], bt["rl"]), bt["name"]


def test_single_cell_pairing(oracle, fx):
    for b, k in ((0, 1), (1, 64), (2, 126)):
        assert cs.single_cell_check(oracle, fx["C"][b], k, fx["cells"][b][k], fx["P"][b][k])
    assert not cs.single_cell_check(oracle, fx["C"][0], 2, fx["cells"][0][1], fx["P"][0][1])


def test_restatement_verdicts(oracle, fx):
    V = lambda *a: cs.verify_cell_kzg_proof_batch(oracle, *a)   # noqa: E731
    assert V([], [], [], []) is True
    c, i, cl, p = batch(fx, [(0, 3), (1, 70), (2, 11), (0, 3), (1, 3)])
    assert V(c, i, cl, p) is True
    assert V(c, i, cl, [p[1], p[0]] + p[2:]) is False                                   # swapped proof
    bad = bytearray(cl[1]); bad[63] ^= 1
    assert V(c, i, [cl[0], bytes(bad)] + cl[2:], p) is False                           # changed element
    assert V(c, [4] + i[1:], cl, p) is False                                           # wrong index
    assert V([c[1]] + c[1:], i, cl, p) is False                                        # wrong commitment
    with pytest.raises(cs.BadArgs):
        V(c, [128] + i[1:], cl, p)
    with pytest.raises(cs.BadArgs):
        V(c, i, [R.to_bytes(32, "big") + cl[0][32:]] + cl[1:], p)
    flags = bytearray(c[0]); flags[0] &= 0x7f
    with pytest.raises(cs.BadArgs):
        V([bytes(flags)] + c[1:], i, cl, p)


def test_public_surface_without_a_device():
    import kzg_rust_amd as kz
    assert (kz.BYTES_PER_CELL, kz.FIELD_ELEMENTS_PER_CELL, kz.CELLS_PER_EXT_BLOB) == (2048, 64, 128)
    assert kz.Cell(bytes(2048)).to_bytes() == bytes(2048)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Cell(bytes(2047))
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "kzg355.h")).read()
    for d in ("#define KZG355_BYTES_PER_CELL 2048", "#define KZG355_FIELD_ELEMENTS_PER_CELL 64", "#define KZG355_CELLS_PER_EXT_BLOB 128"):
        assert d in hdr
