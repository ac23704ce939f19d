"""-m gpu: compute_cells_and_kzg_proofs (EIP-7594 cells and their FK20 proofs) on the device against tests/golden/cells.json (oracle-derived),
the CPU restatements tests/cell_spec.py / tests/fk20_spec.py and closed forms: the derived monomial points, the fixture blobs byte for byte
(single, _many, Python / C / C++), the H intermediates, special blobs, BADARGS cases, the NULL-output forms, round trips through both cell
verifiers, a chunked _many call, a concurrent first call and the 4844 path after it."""
import ctypes as C
import json
import os
import random
import subprocess
import threading

import pytest

import cell_spec as cs
import fk20_spec as fk
from synth import random_blob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R
INF = bytes([0xc0]) + bytes(47)
BADARGS = 1


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def load(kz, setup_bytes):
    g1, g2 = setup_bytes
    return kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])


@pytest.fixture(scope="module")
def settings(kz, setup_bytes):
    s = load(kz, setup_bytes)
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    d["blobs"] = [random_blob(s) for s in d["blob_seeds"]]
    d["cells"] = [cs.compute_cells(b) for b in d["blobs"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    return d


@pytest.fixture(scope="module")
def mono():
    return cs.load_monomial()


def raw(xs):
    return [bytes(x) for x in xs]


def blob_of_power(e, c=0):
    """the blob of X^e + c: values at w4096^rev12(i)"""
    w = fk.W4096
    return b"".join(((pow(pow(w, cs.rev(i, 12), R), e, R) + c) % R).to_bytes(32, "big") for i in range(cs.N_FE))


def test_derived_monomial_points_are_the_ceremony(kz, settings):
    want = open(os.path.join(HERE, "golden", "setup_g1_monomial.bin"), "rb").read()
    assert b"".join(kz.Kzg.debug_cell_setup_monomial_all(settings)) == want


def test_fixture_blobs_single_and_many(kz, settings, fx):
    for b in range(len(fx["blobs"])):
        cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(fx["blobs"][b], settings)
        assert raw(cells) == fx["cells"][b], b
        assert raw(proofs) == fx["P"][b], b
    res = kz.Kzg.compute_cells_and_kzg_proofs_many(fx["blobs"], settings)
    assert [(raw(c), raw(p)) for c, p in res] == [(fx["cells"][b], fx["P"][b]) for b in range(len(fx["blobs"]))]
    assert raw(kz.Kzg.compute_cells(fx["blobs"][1], settings)) == fx["cells"][1]
    assert raw(kz.Kzg.compute_kzg_cell_proofs(fx["blobs"][2], settings)) == fx["P"][2]


def test_h_intermediates_match_the_restatement(kz, settings, fx, oracle, mono):
    [h] = kz.Kzg.debug_cell_compute_h([fx["blobs"][0]], settings)
    assert h[:63] == fk.h_points(oracle, fx["blobs"][0], mono)
    assert h[63] == INF


def test_zero_blob(kz, settings):
    cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(bytes(cs.N_FE * 32), settings)
    assert raw(cells) == [bytes(cs.BYTES_PER_CELL)] * 128
    assert raw(proofs) == [INF] * 128
    assert kz.Kzg.debug_cell_compute_h([bytes(cs.N_FE * 32)], settings)[0] == [INF] * 64


def test_x64_plus_c_gives_the_generator(kz, settings, mono):
    blob = blob_of_power(64, 0x1234567)
    cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(blob, settings)
    assert mono[0].hex().startswith("97f1d3a7")                 # [tau^0]_1 = G1
    assert raw(proofs) == [mono[0]] * 128
    assert raw(cells) == cs.compute_cells(blob)


@pytest.mark.parametrize("t", [0, 1, 37, 63])
def test_x_64_plus_t_gives_tau_t(kz, settings, mono, t):
    proofs = kz.Kzg.compute_kzg_cell_proofs(blob_of_power(64 + t), settings)
    assert raw(proofs) == [mono[t]] * 128


def test_x4095(kz, settings, oracle, mono):
    proofs = raw(kz.Kzg.compute_kzg_cell_proofs(blob_of_power(4095), settings))
    pts = [mono[63 + 64 * s] for s in range(63)]
    for k in range(128):
        a = fk.a_k(k)
        assert proofs[k] == cs.lincomb(oracle, pts, [pow(a, 62 - s, R) for s in range(63)]), k


def test_non_canonical_element(kz, settings, fx):
    bad = bytearray(fx["blobs"][0])
    bad[32 * 1000:32 * 1001] = R.to_bytes(32, "big")
    bad = bytes(bad)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells_and_kzg_proofs(bad, settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells(bad, settings)
    res = kz.Kzg.compute_cells_and_kzg_proofs_many([fx["blobs"][1], bad, fx["blobs"][2]], settings)
    assert isinstance(res[1], kz.BadArgs)
    assert (raw(res[0][0]), raw(res[0][1])) == (fx["cells"][1], fx["P"][1])
    assert (raw(res[2][0]), raw(res[2][1])) == (fx["cells"][2], fx["P"][2])
    lib = kz.kzg.lib()
    st = (C.c_int * 3)()
    rc = lib.kzg355_compute_cells_and_kzg_proofs_many(C.create_string_buffer(3 * 128 * 2048), None, st, fx["blobs"][1] + bad + fx["blobs"][2], 3,
                                                      settings.handle)
    assert rc == BADARGS and list(st) == [0, BADARGS, 0]


def test_null_outputs_and_refusals(kz, settings, fx, setup_bytes):
    lib = kz.kzg.lib()
    blob = fx["blobs"][0]
    full_c, full_p = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
    assert lib.kzg355_compute_cells_and_kzg_proofs(full_c, full_p, blob, settings.handle) == 0
    only_c, only_p = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
    assert lib.kzg355_compute_cells_and_kzg_proofs(only_c, None, blob, settings.handle) == 0
    assert lib.kzg355_compute_cells_and_kzg_proofs(None, only_p, blob, settings.handle) == 0
    assert only_c.raw == full_c.raw == b"".join(fx["cells"][0])
    assert only_p.raw == full_p.raw == b"".join(fx["P"][0])
    assert lib.kzg355_compute_cells_and_kzg_proofs(None, None, blob, settings.handle) == BADARGS
    st = (C.c_int * 2)(7, 7)
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(None, None, st, blob + blob, 2, settings.handle) == BADARGS
    assert list(st) == [BADARGS, BADARGS]
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(full_c, full_p, None, b"", 0, settings.handle) == 0
    # a minimal-preset handle
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        assert lib.kzg355_compute_cells_and_kzg_proofs(full_c, full_p, blob, sm.handle) == BADARGS
        st = (C.c_int * 2)(7, 7)
        assert lib.kzg355_compute_cells_and_kzg_proofs_many(full_c, None, st, blob + blob, 2, sm.handle) == BADARGS
        assert list(st) == [BADARGS, BADARGS]
    finally:
        sm.free()


def test_round_trip_through_both_verifiers(kz, settings, oracle, mono):
    rng = random.Random(77)
    for seed in (9001, 9002):
        blob = random_blob(seed)
        cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(blob, settings)
        com = kz.Kzg.blob_to_kzg_commitment(blob, settings)
        assert kz.Kzg.verify_cell_kzg_proof_batch([com] * 128, list(range(128)), cells, proofs, settings) is True
        sub = rng.sample(range(128), 3)
        assert cs.verify_cell_kzg_proof_batch(oracle, [bytes(com)] * 3, sub, [bytes(cells[k]) for k in sub], [bytes(proofs[k]) for k in sub], mono=mono)
        two = rng.sample(range(128), 2)
        assert cs.cell_proofs(oracle, blob, mono, cells=two) == [bytes(proofs[k]) for k in two]
        # tampering: one cell element changed, or one proof swapped
        k = sub[0]
        tc = bytearray(bytes(cells[k])); tc[31] ^= 1
        bad_cells = list(cells); bad_cells[k] = kz.Cell(bytes(tc))
        assert kz.Kzg.verify_cell_kzg_proof_batch([com] * 128, list(range(128)), bad_cells, proofs, settings) is False
        bad_proofs = list(proofs); bad_proofs[k] = proofs[(k + 1) % 128]
        assert kz.Kzg.verify_cell_kzg_proof_batch([com] * 128, list(range(128)), cells, bad_proofs, settings) is False


def test_chunked_many_matches_single_calls(kz, settings):
    n = 600                                                      # crosses the 512-blob chunk inside the call
    blobs = [random_blob(20000 + i) for i in range(n)]
    res = kz.Kzg.compute_cells_and_kzg_proofs_many(blobs, settings)
    assert len(res) == n and not any(isinstance(r, kz.Error) for r in res)
    for i in sorted(set([0, 511, 512, n - 1] + random.Random(3).sample(range(n), 4))):
        c, p = kz.Kzg.compute_cells_and_kzg_proofs(blobs[i], settings)
        assert (raw(res[i][0]), raw(res[i][1])) == (raw(c), raw(p)), i
        assert raw(res[i][0]) == cs.compute_cells(blobs[i]), i
    # every blob's 128 cells and proofs against its commitment (both calls are pinned to the oracle elsewhere)
    coms = kz.Kzg.blob_to_kzg_commitment_many(blobs, settings)
    assert not any(isinstance(c, kz.Error) for c in coms)
    groups = [([coms[i]] * 128, list(range(128)), res[i][0], res[i][1]) for i in range(n)]
    assert kz.Kzg.verify_cell_kzg_proof_batch_many(groups, settings) == [True] * n


def test_concurrent_first_call_and_4844_after(kz, setup_bytes, fx, oracle, oracle_settings):
    s = load(kz, setup_bytes)
    try:
        out, errs = [None] * 4, []

        def work(t):
            try:
                out[t] = kz.Kzg.compute_cells_and_kzg_proofs(fx["blobs"][t % 3], s)
            except Exception as e:                              # noqa: BLE001 -- reported below
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs
        for t in range(4):
            assert (raw(out[t][0]), raw(out[t][1])) == (fx["cells"][t % 3], fx["P"][t % 3])
        assert raw(kz.Kzg.compute_kzg_cell_proofs(fx["blobs"][1], s)) == fx["P"][1]
        # the 4844 path of the same handle is untouched
        blob = random_blob(31337)
        com = kz.Kzg.blob_to_kzg_commitment(blob, s)
        assert bytes(com) == oracle.blob_to_kzg_commitment(blob, oracle_settings)
        pr = kz.Kzg.compute_blob_kzg_proof(blob, com, s)
        assert bytes(pr) == oracle.compute_blob_kzg_proof(blob, bytes(com), oracle_settings)
        assert kz.Kzg.verify_blob_kzg_proof(blob, com, pr, s) is True
    finally:
        s.free()


def test_python_c_and_cpp_paths_agree(kz, settings, fx, tmp_path):
    inp, outp = str(tmp_path / "blobs.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(b"".join(fx["blobs"]))
    runner = os.path.join(HERE, "native", "cpp_cell_compute_runner")
    r = subprocess.run([runner, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), inp, outp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["ok"] * 3
    got = open(outp, "rb").read()
    per = 128 * 2048 + 128 * 48
    lib = kz.kzg.lib()
    for b in range(3):
        c_c, c_p = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
        assert lib.kzg355_compute_cells_and_kzg_proofs(c_c, c_p, fx["blobs"][b], settings.handle) == 0
        py_c, py_p = kz.Kzg.compute_cells_and_kzg_proofs(fx["blobs"][b], settings)
        want = b"".join(fx["cells"][b]) + b"".join(fx["P"][b])
        assert got[per * b:per * (b + 1)] == want
        assert c_c.raw + c_p.raw == want
        assert b"".join(raw(py_c)) + b"".join(raw(py_p)) == want
