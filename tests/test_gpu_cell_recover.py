"""-m gpu: recover_cells_and_kzg_proofs (EIP-7594 recovery of all cells and proofs from at least half of a blob's cells) on the device.
Expected cells come from cell_spec.compute_cells and expected proofs from tests/golden/cells.json (oracle-derived), never from the library,
except where a test says so: the fixture blobs over nine shapes of index set byte for byte, the NULL-output forms, every refusal (Python and
raw ctypes with the status array), 32 random index sets, the zero blob and X^4095, an inconsistent input against the spec's route, a chunked
_many call, a concurrent first call with the 4844 path after it, and Python / C / C++ side by side."""
import ctypes as C
import json
import os
import random
import subprocess
import threading

import pytest

import cell_spec as cs
import fk20_spec as fk
import recover_spec as rs
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


def raw(xs):
    return [bytes(x) for x in xs]


def index_sets():
    rng = random.Random(7594)
    return [("first64", list(range(64))), ("last64", list(range(64, 128))), ("odd", list(range(1, 128, 2))), ("even", list(range(0, 128, 2))),
            ("random64", sorted(rng.sample(range(128), 64))), ("random65", sorted(rng.sample(range(128), 65))),
            ("random100", sorted(rng.sample(range(128), 100))), ("127cells", sorted(rng.sample(range(128), 127))), ("all128", list(range(128)))]


def idx_array(ix):
    return (C.c_size_t * max(len(ix), 1))(*ix)


@pytest.mark.parametrize("name,ix", index_sets(), ids=[n for n, _ in index_sets()])
def test_fixture_blobs_over_index_sets(kz, settings, fx, name, ix):
    for b in range(3):
        cells, proofs = kz.Kzg.recover_cells_and_kzg_proofs(ix, [fx["cells"][b][k] for k in ix], settings)
        assert raw(cells) == fx["cells"][b], (name, b)
        assert raw(proofs) == fx["P"][b], (name, b)


def test_null_output_forms(kz, settings, fx):
    lib = kz.kzg.lib()
    ix = index_sets()[4][1]
    known = b"".join(fx["cells"][0][k] for k in ix)
    full_c, full_p = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
    assert lib.kzg355_recover_cells_and_kzg_proofs(full_c, full_p, idx_array(ix), known, len(ix), settings.handle) == 0
    only_c, only_p = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
    assert lib.kzg355_recover_cells_and_kzg_proofs(only_c, None, idx_array(ix), known, len(ix), settings.handle) == 0
    assert lib.kzg355_recover_cells_and_kzg_proofs(None, only_p, idx_array(ix), known, len(ix), settings.handle) == 0
    assert only_c.raw == full_c.raw == b"".join(fx["cells"][0])
    assert only_p.raw == full_p.raw == b"".join(fx["P"][0])
    assert lib.kzg355_recover_cells_and_kzg_proofs(None, None, idx_array(ix), known, len(ix), settings.handle) == BADARGS
    st = (C.c_int * 2)(7, 7)
    assert lib.kzg355_recover_cells_and_kzg_proofs_many(None, None, st, idx_array(ix), known + known, len(ix), 2, settings.handle) == BADARGS
    assert list(st) == [BADARGS, BADARGS]
    assert raw(kz.Kzg.recover_cells(ix, [fx["cells"][0][k] for k in ix], settings)) == fx["cells"][0]


def test_refusals(kz, settings, fx, setup_bytes):
    lib = kz.kzg.lib()
    cells = fx["cells"][0]
    out_c, out_p = C.create_string_buffer(3 * 128 * 2048), C.create_string_buffer(3 * 128 * 48)

    def call(ix, n=None, data=None):
        n = len(ix) if n is None else n
        data = b"".join(cells[k % 128] for k in ix) if data is None else data
        return lib.kzg355_recover_cells_and_kzg_proofs(out_c, out_p, idx_array(ix), data, n, settings.handle)

    bad_sets = {"63 cells": list(range(63)), "129 cells": list(range(128)) + [128], "index 128": list(range(63)) + [128],
                "huge index": list(range(63)) + [(1 << 64) - 1], "duplicate": list(range(63)) + [62], "duplicate first": [0] + list(range(64)),
                "descending pair": list(range(62)) + [70, 69], "reversed": list(range(64))[::-1], "no cells": []}
    for name, ix in bad_sets.items():
        assert call(ix) == BADARGS, name
        with pytest.raises(kz.BadArgs):
            kz.Kzg.recover_cells_and_kzg_proofs(ix, [cells[k % 128] for k in ix], settings)
        with pytest.raises(kz.BadArgs):
            kz.Kzg.recover_cells(ix, [cells[k % 128] for k in ix], settings)
        st = (C.c_int * 3)(7, 7, 7)
        data = b"".join(cells[k % 128] for k in ix) * 3
        assert lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, out_p, st, idx_array(ix), data, len(ix), 3, settings.handle) == BADARGS, name
        assert list(st) == [BADARGS] * 3, name
    ix = list(range(64))
    assert call(ix) == 0
    # NULL inputs with n > 0
    assert lib.kzg355_recover_cells_and_kzg_proofs(out_c, out_p, None, b"".join(cells[:64]), 64, settings.handle) == BADARGS
    assert lib.kzg355_recover_cells_and_kzg_proofs(out_c, out_p, idx_array(ix), None, 64, settings.handle) == BADARGS
    assert lib.kzg355_recover_cells_and_kzg_proofs(out_c, out_p, idx_array(ix), b"".join(cells[:64]), 64, None) == BADARGS
    # m = 0: nothing to do, with or without a status array; the index set is still checked
    assert lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, out_p, None, idx_array(ix), None, 64, 0, settings.handle) == 0
    st = (C.c_int * 1)(7)
    assert lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, out_p, st, idx_array(ix), b"", 64, 0, settings.handle) == 0 and list(st) == [7]
    assert lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, out_p, None, idx_array(ix), None, 63, 0, settings.handle) == BADARGS
    assert kz.Kzg.recover_cells_and_kzg_proofs_many(ix, [], settings) == []
    # a length mismatch never reaches the library
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs(ix, cells[:63], settings)
    # a minimal-preset handle
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        assert lib.kzg355_recover_cells_and_kzg_proofs(out_c, out_p, idx_array(ix), b"".join(cells[:64]), 64, sm.handle) == BADARGS
        st = (C.c_int * 2)(7, 7)
        assert lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, None, st, idx_array(ix), b"".join(cells[:64]) * 2, 64, 2, sm.handle) == BADARGS
        assert list(st) == [BADARGS, BADARGS]
    finally:
        sm.free()


def test_non_canonical_element(kz, settings, fx):
    lib = kz.kzg.lib()
    ix = index_sets()[5][1]                                       # 65 cells
    rows = [[fx["cells"][b][k] for k in ix] for b in (1, 0, 2)]
    bad = list(rows[1])
    bad[40] = bad[40][:32 * 17] + R.to_bytes(32, "big") + bad[40][32 * 18:]
    for last in (R.to_bytes(32, "big"), b"\xff" * 32):            # r itself and the largest 256-bit value, in the last element of the last cell
        worst = list(rows[1])
        worst[-1] = worst[-1][:-32] + last
        with pytest.raises(kz.BadArgs):
            kz.Kzg.recover_cells(ix, worst, settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs(ix, bad, settings)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells(ix, bad, settings)
    res = kz.Kzg.recover_cells_and_kzg_proofs_many(ix, [rows[0], bad, rows[2]], settings)
    assert isinstance(res[1], kz.BadArgs)
    assert (raw(res[0][0]), raw(res[0][1])) == (fx["cells"][1], fx["P"][1])
    assert (raw(res[2][0]), raw(res[2][1])) == (fx["cells"][2], fx["P"][2])
    st = (C.c_int * 3)(7, 7, 7)
    out_c = C.create_string_buffer(3 * 128 * 2048)
    rc = lib.kzg355_recover_cells_and_kzg_proofs_many(out_c, None, st, idx_array(ix), b"".join(rows[0]) + b"".join(bad) + b"".join(rows[2]), len(ix), 3,
                                                      settings.handle)
    assert rc == BADARGS and list(st) == [0, BADARGS, 0]
    assert out_c.raw[:128 * 2048] == b"".join(fx["cells"][1]) and out_c.raw[2 * 128 * 2048:] == b"".join(fx["cells"][2])
    # r - 1 is canonical
    blob = (R - 1).to_bytes(32, "big") * cs.N_FE
    cells = cs.compute_cells(blob)
    assert raw(kz.Kzg.recover_cells(ix, [cells[k] for k in ix], settings)) == cells


def test_random_index_sets_cells_only(kz, settings):
    blob = random_blob(7600)
    cells = cs.compute_cells(blob)
    rng = random.Random(20260)
    sizes = [64, 128] + [rng.randint(64, 128) for _ in range(34)]
    assert len(sizes) >= 32
    for n in sizes:
        ix = sorted(rng.sample(range(128), n))
        assert raw(kz.Kzg.recover_cells(ix, [cells[k] for k in ix], settings)) == cells, ix


def test_zero_blob_and_x4095(kz, settings):
    ix = index_sets()[4][1]
    cells, proofs = kz.Kzg.recover_cells_and_kzg_proofs(ix, [bytes(cs.BYTES_PER_CELL)] * len(ix), settings)
    assert raw(cells) == [bytes(cs.BYTES_PER_CELL)] * 128
    assert raw(proofs) == [INF] * 128
    w = fk.W4096
    blob = b"".join(pow(pow(w, cs.rev(i, 12), R), 4095, R).to_bytes(32, "big") for i in range(cs.N_FE))      # X^4095
    want = cs.compute_cells(blob)
    for ix in (index_sets()[1][1], index_sets()[6][1]):
        cells, proofs = kz.Kzg.recover_cells_and_kzg_proofs(ix, [want[k] for k in ix], settings)
        assert raw(cells) == want
        assert raw(proofs) == raw(kz.Kzg.compute_kzg_cell_proofs(blob, settings))      # pinned to the oracle by test_gpu_cell_compute.py::test_x4095


def test_inconsistent_input_follows_the_spec(kz, settings, fx):
    ix = list(range(20, 100))
    bad = [fx["cells"][2][k] for k in ix]
    t = bytearray(bad[3])
    t[31] ^= 1
    bad[3] = bytes(t)
    f = rs.recover_coefficients_spec(ix, bad)
    assert f != cs.blob_coefficients(fx["blobs"][2])
    f2, high = rs.recover_coefficients_columns(ix, bad)
    assert f2 == f and high is True
    cells, proofs = kz.Kzg.recover_cells_and_kzg_proofs(ix, bad, settings)
    assert raw(cells) == rs.cells_from_coefficients(f)
    assert raw(proofs) == raw(kz.Kzg.compute_kzg_cell_proofs(fk.blob_from_coefficients(f), settings))
    assert raw(kz.Kzg.recover_cells(ix, bad, settings)) == raw(cells)


def test_chunked_many_with_one_shared_index_set(kz, settings):
    m = 600                                                      # crosses the 512-blob chunk inside the call
    blobs = [random_blob(30000 + i) for i in range(m)]
    ix = sorted(random.Random(600).sample(range(128), 64))
    full = kz.Kzg._compute_cells(blobs, settings, True, False)   # the known cells of all blobs (checked against cell_spec below)
    rows = [[full[i][0][k] for k in ix] for i in range(m)]
    res = kz.Kzg.recover_cells_and_kzg_proofs_many(ix, rows, settings)
    assert len(res) == m and not any(isinstance(r, kz.Error) for r in res)
    picks = sorted(set([0, 511, 512, m - 1] + random.Random(4).sample(range(m), 4)))
    want = kz.Kzg.compute_cells_and_kzg_proofs_many([blobs[i] for i in picks], settings)
    for i, (wc, wp) in zip(picks, want):
        assert (raw(res[i][0]), raw(res[i][1])) == (raw(wc), raw(wp)), i
        assert raw(res[i][0]) == cs.compute_cells(blobs[i]), i
    coms = kz.Kzg.blob_to_kzg_commitment_many(blobs, settings)
    assert not any(isinstance(c, kz.Error) for c in coms)
    groups = [([coms[i]] * 128, list(range(128)), res[i][0], res[i][1]) for i in range(m)]
    assert kz.Kzg.verify_cell_kzg_proof_batch_many(groups, settings) == [True] * m


def test_concurrent_first_call_and_4844_after(kz, setup_bytes, fx, oracle, oracle_settings):
    s = load(kz, setup_bytes)
    try:
        out, errs = [None] * 4, []
        sets = [index_sets()[i][1] for i in (4, 5, 6, 2)]

        def work(t):
            try:
                out[t] = kz.Kzg.recover_cells_and_kzg_proofs(sets[t], [fx["cells"][t % 3][k] for k in sets[t]], s)
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
        blob = random_blob(31338)
        com = kz.Kzg.blob_to_kzg_commitment(blob, s)
        assert bytes(com) == oracle.blob_to_kzg_commitment(blob, oracle_settings)
        pr = kz.Kzg.compute_blob_kzg_proof(blob, com, s)
        assert bytes(pr) == oracle.compute_blob_kzg_proof(blob, bytes(com), oracle_settings)
        assert kz.Kzg.verify_blob_kzg_proof(blob, com, pr, s) is True
    finally:
        s.free()


def test_python_c_and_cpp_agree(kz, settings, fx, tmp_path):
    ix = index_sets()[6][1]                                       # 100 cells
    ixp, inp, outp = str(tmp_path / "indices.bin"), str(tmp_path / "cells.bin"), str(tmp_path / "out.bin")
    with open(ixp, "wb") as f:
        f.write(bytes(ix))
    with open(inp, "wb") as f:
        f.write(b"".join(fx["cells"][b][k] for b in range(3) for k in ix))
    runner = os.path.join(HERE, "native", "cpp_cell_recover_runner")
    r = subprocess.run([runner, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), ixp, inp, outp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["ok"] * 3
    got = open(outp, "rb").read()
    per = 128 * 2048 + 128 * 48
    lib = kz.kzg.lib()
    for b in range(3):
        known = [fx["cells"][b][k] for k in ix]
        c_c, c_p = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
        assert lib.kzg355_recover_cells_and_kzg_proofs(c_c, c_p, idx_array(ix), b"".join(known), len(ix), settings.handle) == 0
        py_c, py_p = kz.Kzg.recover_cells_and_kzg_proofs(ix, known, settings)
        want = b"".join(fx["cells"][b]) + b"".join(fx["P"][b])
        assert got[per * b:per * (b + 1)] == want
        assert c_c.raw + c_p.raw == want
        assert b"".join(raw(py_c)) + b"".join(raw(py_p)) == want
    # a refusal through the mirror: a descending pair
    with open(ixp, "wb") as f:
        f.write(bytes(list(range(62)) + [70, 69]))
    with open(inp, "wb") as f:
        f.write(b"".join(fx["cells"][0][k] for k in list(range(62)) + [70, 69]))
    r = subprocess.run([runner, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), ixp, inp, outp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split()[0] == "err", (r.stdout, r.stderr)
