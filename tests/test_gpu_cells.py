"""-m gpu: verify_cell_kzg_proof_batch (EIP-7594 cells) on the device against tests/golden/cells.json (oracle-derived) and the CPU restatement
tests/cell_spec.py: the derived monomial prefix, the stage intermediates byte for byte, verdicts on valid / tampered / malformed batches, the
_many form against the single calls, a differential fuzz, one large _many call, and the Python / C / C++ paths side by side."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import cell_spec as cs
from synth import random_blob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def settings(kz, setup_bytes):
    g1, g2 = setup_bytes
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    blobs = [random_blob(s) for s in d["blob_seeds"]]
    d["cells"] = [cs.compute_cells(b) for b in blobs]
    d["C"] = [bytes.fromhex(c) for c in d["commitments"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    return d


def batch(fx, items):
    return [fx["C"][b] for b, _ in items], [k for _, k in items], [fx["cells"][b][k] for b, k in items], [fx["P"][b][k] for b, k in items]


def test_monomial_prefix_matches_the_ceremony(kz, settings):
    mono = open(os.path.join(HERE, "golden", "setup_g1_monomial.bin"), "rb").read()
    assert b"".join(kz.Kzg.debug_cell_setup_monomial(settings)) == mono[:64 * 48]


def test_intermediates_byte_exact(kz, settings, fx):
    assert len(fx["batches"]) >= 4
    for b in fx["batches"]:
        res, out = kz.Kzg.debug_cell_batch_intermediates([batch(fx, [tuple(x) for x in b["items"]])], settings)
        assert res == [True], b["name"]
        o = out[0]
        assert o[:32].hex() == b["r"], b["name"]
        assert o[32:80].hex() == b["itau"], b["name"]
        assert o[80:128].hex() == b["ll"], b["name"]
        assert o[128:176].hex() == b["rl"], b["name"]


def test_valid_batches(kz, settings, fx):
    V = kz.Kzg.verify_cell_kzg_proof_batch
    assert V(*batch(fx, [(0, 9)]), settings) is True                                       # one cell
    assert V(*batch(fx, [(b, 33) for b in range(3)]), settings) is True                    # a column
    assert V(*batch(fx, [(2, k) for k in range(128)]), settings) is True                   # a row
    mixed = [(0, 1), (1, 1), (0, 1), (2, 127), (1, 64), (1, 64), (0, 90), (2, 5)]
    assert V(*batch(fx, mixed), settings) is True                                          # repeated commitments and (commitment, index) pairs
    assert V([], [], [], [], settings) is True                                             # n = 0


def test_tampered_batches_are_false(kz, settings, fx):
    V = kz.Kzg.verify_cell_kzg_proof_batch
    c, i, cl, p = batch(fx, [(0, 3), (1, 70), (2, 11)])
    assert V(c, i, cl, [p[1], p[0], p[2]], settings) is False                              # swapped proofs
    bad = bytearray(cl[1]); bad[31] ^= 1
    assert V(c, i, [cl[0], bytes(bad), cl[2]], p, settings) is False                         # changed element
    assert V(c, [3, 71, 11], cl, p, settings) is False                                     # wrong index
    assert V([c[0], c[2], c[2]], i, cl, p, settings) is False                              # wrong commitment


def _off_curve(oracle):
    for x in range(1, 1000):
        b = bytearray(x.to_bytes(48, "big")); b[0] |= 0x80
        if oracle.g1_uncompress_only(bytes(b)) != 0:
            return bytes(b)


def _not_in_subgroup(oracle):
    for x in range(1, 1000):
        b = bytearray(x.to_bytes(48, "big")); b[0] |= 0x80
        if oracle.g1_uncompress_only(bytes(b)) == 0 and oracle.g1_validate(bytes(b)) != 0:
            return bytes(b)


def test_bad_inputs_are_badargs(kz, settings, fx, oracle):
    V = kz.Kzg.verify_cell_kzg_proof_batch
    c, i, cl, p = batch(fx, [(0, 3), (1, 70)])
    with pytest.raises(kz.BadArgs):
        V(c, [3, 128], cl, p, settings)
    nc = cl[0][:32 * 7] + R.to_bytes(32, "big") + cl[0][32 * 8:]
    with pytest.raises(kz.BadArgs):
        V(c, i, [nc, cl[1]], p, settings)
    flags = bytearray(c[0]); flags[0] &= 0x7f
    for bad in (_off_curve(oracle), _not_in_subgroup(oracle), bytes(flags)):
        assert bad is not None
        with pytest.raises(kz.BadArgs):
            V([bad, c[1]], i, cl, p, settings)
        with pytest.raises(kz.BadArgs):
            V(c, i, cl, [p[0], bad], settings)
    with pytest.raises(kz.InvalidBytesLength):
        kz.Cell(b"\x00" * 2047)


def test_many_matches_single_calls(kz, settings, fx, oracle):
    rng = random.Random(11)
    groups = []
    for g in range(12):
        items = [(rng.randrange(3), rng.randrange(128)) for _ in range(5)]
        c, i, cl, p = batch(fx, items)
        kind = g % 4
        if kind == 1:
            p = [p[1], p[0]] + p[2:]
        elif kind == 2:
            i = [128] + i[1:]
        elif kind == 3:
            cl = [cl[0][:32] + R.to_bytes(32, "big") + cl[0][64:]] + cl[1:]
        groups.append((c, i, cl, p))
    many = kz.Kzg.verify_cell_kzg_proof_batch_many(groups, settings)
    for g, (grp, got) in enumerate(zip(groups, many)):
        try:
            single = kz.Kzg.verify_cell_kzg_proof_batch(*grp, settings)
        except kz.Error as e:
            single = type(e)
        want = {0: True, 1: False, 2: kz.BadArgs, 3: kz.BadArgs}[g % 4]
        assert (type(got) if isinstance(got, kz.Error) else got) == single == want, g


def test_differential_fuzz_against_the_spec(kz, settings, fx, oracle):
    rng = random.Random(0x7594)
    mono = cs.load_monomial(64)
    g2 = cs.g2_points()
    groups, want = [], []
    for t in range(240):
        c, i, cl, p = [list(x) for x in batch(fx, [(rng.randrange(3), rng.randrange(128)) for _ in range(4)])]
        m = rng.randrange(8)
        k = rng.randrange(4)
        if m == 1:
            p[k], p[(k + 1) % 4] = p[(k + 1) % 4], p[k]
        elif m == 2:
            j = rng.randrange(64)
            cl[k] = cl[k][:32 * j] + rng.randrange(R).to_bytes(32, "big") + cl[k][32 * j + 32:]
        elif m == 3:
            i[k] = rng.randrange(128)
        elif m == 4:
            c[k] = fx["C"][rng.randrange(3)]
        elif m == 5:
            i[k] = 128 + rng.randrange(1000)
        elif m == 6:
            j = rng.randrange(64)
            cl[k] = cl[k][:32 * j] + (R + rng.randrange(2 ** 255 - R)).to_bytes(32, "big") + cl[k][32 * j + 32:]
        groups.append((c, i, cl, p))
        try:
            want.append(cs.verify_cell_kzg_proof_batch(oracle, c, i, cl, p, mono=mono, g2=g2))
        except cs.BadArgs:
            want.append("BadArgs")
    got = kz.Kzg.verify_cell_kzg_proof_batch_many(groups, settings)
    got = ["BadArgs" if isinstance(x, kz.BadArgs) else x for x in got]
    assert got == want
    assert True in want and False in want and "BadArgs" in want


def test_large_many_call(kz, settings, fx):
    rng = random.Random(5)
    groups, want = [], []
    for g in range(128):
        c, i, cl, p = batch(fx, [(rng.randrange(3), rng.randrange(128)) for _ in range(64)])
        bad = g % 9 == 4 and p[0] != p[1]
        if bad:
            p = [p[1], p[0]] + p[2:]
        groups.append((c, i, cl, p))
        want.append(not bad)
    assert kz.Kzg.verify_cell_kzg_proof_batch_many(groups, settings) == want


def test_python_c_and_cpp_paths_agree(kz, settings, fx, tmp_path):
    good = batch(fx, [(0, 3), (1, 70), (2, 11), (0, 3)])
    bad = (good[0], good[1], good[2], [good[3][1], good[3][0]] + good[3][2:])
    lib = kz.kzg.lib()
    for args, want in ((good, True), (bad, False)):
        assert kz.Kzg.verify_cell_kzg_proof_batch(*args, settings) is want
        ok = C.c_bool()
        n = len(args[0])
        rc = lib.kzg355_verify_cell_kzg_proof_batch(C.byref(ok), b"".join(args[0]), (C.c_size_t * n)(*args[1]), b"".join(args[2]), b"".join(args[3]), n,
                                                     settings.handle)
        assert rc == 0 and ok.value is want
    runner = os.path.join(HERE, "native", "cpp_cell_runner")
    inp = str(tmp_path / "cells_in.bin")
    with open(inp, "wb") as f:
        for args in (good, bad):
            f.write(len(args[0]).to_bytes(4, "little"))
            for k in range(len(args[0])):
                f.write(args[0][k] + args[1][k].to_bytes(8, "little") + args[2][k] + args[3][k])
    out = subprocess.run([runner, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), inp],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["true", "false"]
