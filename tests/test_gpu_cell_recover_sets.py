"""-m gpu: recover_cells_and_kzg_proofs_many_sets, the recovery call whose blobs each bring their own index set, on the device.  Expected cells
come from cell_spec.compute_cells and expected proofs from tests/golden/cells.json (oracle-derived), never from the call under test: the nine
shapes of index set as nine units of one call (and with either output alone), shared sets that are not adjacent, units that fail next to units
that do not (every per-blob refusal, in Python and raw ctypes with the status array), the refusals of the whole call, an inconsistent unit
against the spec's route, 600 blobs across the 512-blob chunk with five and with 600 distinct sets, the device-resident form byte for byte
against the host form, the shared-set call against five equal lists, and Python / C / C++ side by side."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import cell_spec as cs
import recover_spec as rs
from synth import random_blob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R
BADARGS = 1
CELL, ROW, PROOFS = 2048, 128 * 2048, 128 * 48


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
    d["blobs"] = [random_blob(s) for s in d["blob_seeds"]]
    d["cells"] = [cs.compute_cells(b) for b in d["blobs"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    return d


def raw(xs):
    return [bytes(x) for x in xs]


def index_sets():
    """the nine shapes of tests/test_gpu_cell_recover.py, restated"""
    rng = random.Random(7594)
    return [("first64", list(range(64))), ("last64", list(range(64, 128))), ("odd", list(range(1, 128, 2))), ("even", list(range(0, 128, 2))),
            ("random64", sorted(rng.sample(range(128), 64))), ("random65", sorted(rng.sample(range(128), 65))),
            ("random100", sorted(rng.sample(range(128), 100))), ("127cells", sorted(rng.sample(range(128), 127))), ("all128", list(range(128)))]


def unit(cells, ix):
    return (list(ix), [cells[k] for k in ix])


def c_call(kz, settings, units, cells=True, proofs=True, status=True):
    """the host form through ctypes: (return value, statuses, cells_out bytes, proofs_out bytes)"""
    m = len(units)
    flat = [i for ix, _ in units for i in ix]
    counts, idx = (C.c_size_t * max(m, 1))(*[len(ix) for ix, _ in units]), (C.c_size_t * max(len(flat), 1))(*flat)
    c_out = C.create_string_buffer(ROW * m) if cells else None
    p_out = C.create_string_buffer(PROOFS * m) if proofs else None
    st = (C.c_int * m)(*([7] * m)) if status else None
    rc = kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_many_sets(c_out, p_out, st, counts, idx, b"".join(b"".join(row) for _, row in units), m,
                                                                    settings.handle)
    return rc, list(st) if status else None, c_out.raw if cells else None, p_out.raw if proofs else None


def nine_units(fx):
    return [unit(fx["cells"][j % 3], ix) for j, (_, ix) in enumerate(index_sets())]


# ---- 1. every shape of set in one call
def test_every_shape_of_set_in_one_call(kz, settings, fx):
    units = nine_units(fx)
    res = kz.Kzg.recover_cells_and_kzg_proofs_many_sets(units, settings)
    assert len(res) == 9
    for j, (name, _) in enumerate(index_sets()):
        assert raw(res[j][0]) == fx["cells"][j % 3], name
        assert raw(res[j][1]) == fx["P"][j % 3], name
    want_c = b"".join(b"".join(fx["cells"][j % 3]) for j in range(9))
    want_p = b"".join(b"".join(fx["P"][j % 3]) for j in range(9))
    assert c_call(kz, settings, units) == (0, [0] * 9, want_c, want_p)
    assert c_call(kz, settings, units, proofs=False) == (0, [0] * 9, want_c, None)
    assert c_call(kz, settings, units, cells=False) == (0, [0] * 9, None, want_p)
    assert c_call(kz, settings, units, status=False) == (0, None, want_c, want_p)
    only = kz.Kzg.recover_cells_many_sets(units, settings)
    assert [raw(x) for x in only] == [fx["cells"][j % 3] for j in range(9)]


# ---- 2. shared sets that are not adjacent
@pytest.fixture(scope="module")
def scattered():
    """24 random blobs with random counts; units 3, 11 and 19 share one index list and units 7 and 20 carry all 128 cells"""
    rng = random.Random(2424)
    cells = [cs.compute_cells(random_blob(52000 + i)) for i in range(24)]
    sets = [sorted(rng.sample(range(128), rng.randint(64, 128))) for _ in range(24)]
    sets[11] = sets[19] = sets[3]
    sets[7] = sets[20] = list(range(128))
    return cells, [unit(cells[i], sets[i]) for i in range(24)]


def test_shared_sets_that_are_not_adjacent(kz, settings, scattered):
    cells, units = scattered
    assert units[3][0] == units[11][0] == units[19][0] and len({tuple(u[0]) for u in units}) == 21
    res = kz.Kzg.recover_cells_many_sets(units, settings)
    for i in range(24):
        assert raw(res[i]) == cells[i], i
        assert raw(kz.Kzg.recover_cells(units[i][0], units[i][1], settings)) == raw(res[i]), i


# ---- 3. independence of the units
def five_units(fx):
    sets = [s for _, s in index_sets()]
    units = [unit(fx["cells"][0], sets[4]), unit(fx["cells"][1], list(range(62)) + [70, 69]), unit(fx["cells"][2], sets[6]),
             unit(fx["cells"][0], sets[5]), unit(fx["cells"][1], sets[2])]
    last = units[3][1][-1]
    units[3][1][-1] = last[:-32] + R.to_bytes(32, "big")          # r itself in the last element of the last cell
    return units, {0: 0, 2: 2, 4: 1}


def test_independence_of_the_units(kz, settings, fx):
    units, good = five_units(fx)
    rc, st, c_out, p_out = c_call(kz, settings, units)
    assert rc == BADARGS and st == [0, BADARGS, 0, BADARGS, 0]
    res = kz.Kzg.recover_cells_and_kzg_proofs_many_sets(units, settings)
    assert isinstance(res[1], kz.BadArgs) and isinstance(res[3], kz.BadArgs)
    for u, b in good.items():
        assert c_out[ROW * u:ROW * (u + 1)] == b"".join(fx["cells"][b]) and p_out[PROOFS * u:PROOFS * (u + 1)] == b"".join(fx["P"][b]), u
        assert (raw(res[u][0]), raw(res[u][1])) == (fx["cells"][b], fx["P"][b]), u
    only = kz.Kzg.recover_cells_many_sets(units, settings)
    assert isinstance(only[1], kz.BadArgs) and isinstance(only[3], kz.BadArgs) and raw(only[4]) == fx["cells"][1]


# ---- 4. every per-blob refusal among good neighbours
BAD_LISTS = {"63 cells": list(range(63)), "129 cells": list(range(128)) + [128], "no cells": [], "index 128": list(range(63)) + [128],
             "huge index": list(range(63)) + [(1 << 64) - 1], "duplicate": list(range(63)) + [62], "reversed": list(range(64))[::-1]}


@pytest.mark.parametrize("name", list(BAD_LISTS))
def test_a_refused_unit_between_good_neighbours(kz, settings, fx, name):
    ix = BAD_LISTS[name]
    sets = [s for _, s in index_sets()]
    units = [unit(fx["cells"][1], sets[5]), (ix, [fx["cells"][0][k % 128] for k in ix]), unit(fx["cells"][2], sets[7])]
    rc, st, c_out, p_out = c_call(kz, settings, units)
    assert rc == BADARGS and st == [0, BADARGS, 0]
    # the right neighbour's cells sit behind the refused unit's, however many it brought: the layout follows the counts
    assert c_out[:ROW] == b"".join(fx["cells"][1]) and c_out[2 * ROW:] == b"".join(fx["cells"][2])
    assert p_out[:PROOFS] == b"".join(fx["P"][1]) and p_out[2 * PROOFS:] == b"".join(fx["P"][2])
    res = kz.Kzg.recover_cells_and_kzg_proofs_many_sets(units, settings)
    assert isinstance(res[1], kz.BadArgs)
    assert (raw(res[0][0]), raw(res[0][1]), raw(res[2][0]), raw(res[2][1])) == (fx["cells"][1], fx["P"][1], fx["cells"][2], fx["P"][2])


# ---- 5. whole-call refusals
def test_whole_call_refusals(kz, settings, fx, setup_bytes):
    lib = kz.kzg.lib()
    fn = lib.kzg355_recover_cells_and_kzg_proofs_many_sets
    m = 3
    ix = list(range(64))
    counts, idx = (C.c_size_t * m)(64, 64, 64), (C.c_size_t * (64 * m))(*(ix * m))
    data = b"".join(b"".join(fx["cells"][b][:64]) for b in range(3))
    out_c, out_p = C.create_string_buffer(ROW * m), C.create_string_buffer(PROOFS * m)

    def refused(*args):
        st = (C.c_int * m)(7, 7, 7)
        return fn(args[0], args[1], st, *args[2:]) == BADARGS and list(st) == [BADARGS] * m

    assert refused(None, None, counts, idx, data, m, settings.handle)
    assert refused(out_c, out_p, None, idx, data, m, settings.handle)
    assert refused(out_c, out_p, counts, None, data, m, settings.handle)
    assert refused(out_c, out_p, counts, idx, None, m, settings.handle)
    assert refused(out_c, out_p, counts, idx, data, m, None)
    huge = (C.c_size_t * m)(64, (1 << 64) - 64, 64)                # the sum of the counts passes 2^64
    assert refused(out_c, out_p, huge, idx, data, m, settings.handle)
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        assert refused(out_c, out_p, counts, idx, data, m, sm.handle)
    finally:
        sm.free()
    # the same arguments are a good call
    st = (C.c_int * m)(7, 7, 7)
    assert fn(out_c, out_p, st, counts, idx, data, m, settings.handle) == 0 and list(st) == [0] * m
    assert out_c.raw == b"".join(b"".join(fx["cells"][b]) for b in range(3))
    # m == 0: nothing to do and nothing touched, with NULL arrays
    st = (C.c_int * 1)(7)
    assert fn(out_c, out_p, st, None, None, None, 0, settings.handle) == 0 and list(st) == [7]
    assert fn(out_c, out_p, None, None, None, None, 0, settings.handle) == 0
    assert kz.Kzg.recover_cells_and_kzg_proofs_many_sets([], settings) == [] and kz.Kzg.recover_cells_many_sets([], settings) == []


# ---- 6. inconsistent input next to consistent input
def test_inconsistent_input_next_to_consistent_input(kz, settings, fx):
    ix = list(range(20, 100))
    bad = [fx["cells"][2][k] for k in ix]
    t = bytearray(bad[3])
    t[31] ^= 1
    bad[3] = bytes(t)
    f = rs.recover_coefficients_spec(ix, bad)
    assert f != cs.blob_coefficients(fx["blobs"][2])
    sets = [s for _, s in index_sets()]
    units = [unit(fx["cells"][0], sets[6]), (ix, bad), unit(fx["cells"][1], ix)]
    res = kz.Kzg.recover_cells_and_kzg_proofs_many_sets(units, settings)
    assert raw(res[1][0]) == rs.cells_from_coefficients(f)
    single = kz.Kzg.recover_cells_and_kzg_proofs(ix, bad, settings)
    assert (raw(res[1][0]), raw(res[1][1])) == (raw(single[0]), raw(single[1]))
    assert (raw(res[0][0]), raw(res[0][1])) == (fx["cells"][0], fx["P"][0])
    assert (raw(res[2][0]), raw(res[2][1])) == (fx["cells"][1], fx["P"][1])


# ---- 7. chunks
@pytest.fixture(scope="module")
def chunked(kz, settings):
    """600 blobs (more than the 512-blob chunk), their cells from the compute path (checked against cell_spec where they are used), the units
    of the two calls and the host form's cells_out for each"""
    m = 600
    blobs = [random_blob(60000 + i) for i in range(m)]
    full = [raw(r[0]) for r in kz.Kzg._compute_cells(blobs, settings, True, False)]
    rng = random.Random(600)
    five = [sorted(rng.sample(range(128), n)) for n in (64, 71, 90, 113, 128)]
    few = [unit(full[i], five[i % 5]) for i in range(m)]         # 511 -> set 1, 512 -> set 2; every set on both sides of the chunk boundary
    many = [unit(full[i], sorted(rng.sample(range(128), rng.randint(64, 127)))) for i in range(m)]
    assert len({tuple(u[0]) for u in many}) == m                  # 600 distinct sets: more tables than one chunk holds
    assert sum(len(u[0]) for u in few[:512]) not in (512 * n for n in range(64, 129))
    picks = sorted(set([0, 511, 512, m - 1] + random.Random(4).sample(range(m), 4)))
    want = {i: cs.compute_cells(blobs[i]) for i in picks}
    host = {}
    for name, units in (("few", few), ("many", many)):
        rc, st, c_out, _ = c_call(kz, settings, units, proofs=False)
        assert rc == 0 and st == [0] * m, name
        host[name] = c_out
    return {"m": m, "few": few, "many": many, "want": want, "host": host}


@pytest.mark.parametrize("name", ["few", "many"])
def test_chunked_call(chunked, name):
    out = chunked["host"][name]
    for i, cells in chunked["want"].items():
        assert out[ROW * i:ROW * (i + 1)] == b"".join(cells), (name, i)


# ---- 8. device form
@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def u8(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def device_call(kz, torch, settings, units, cells=True, proofs=False):
    m = len(units)
    d_in = u8(torch, b"".join(b"".join(row) for _, row in units))
    dc = torch.zeros(ROW * m, dtype=torch.uint8, device="cuda") if cells else None
    dp = torch.zeros(PROOFS * m, dtype=torch.uint8, device="cuda") if proofs else None
    res = kz.Kzg.recover_cells_and_kzg_proofs_many_sets_device([len(ix) for ix, _ in units], [i for ix, _ in units for i in ix], d_in, settings,
                                                               cells_out=dc, proofs_out=dp)
    return res, bytes(dc.cpu().numpy()) if cells else None, bytes(dp.cpu().numpy()) if proofs else None


def test_device_form_matches_the_host_form(kz, torch, settings, scattered, chunked):
    _, units = scattered
    rc, st, want, _ = c_call(kz, settings, units, proofs=False)
    assert rc == 0
    assert device_call(kz, torch, settings, units) == ([None] * 24, want, None)
    for name in ("few", "many"):
        res, got, _ = device_call(kz, torch, settings, chunked[name])
        assert res == [None] * chunked["m"] and got == chunked["host"][name], name


def test_device_form_units_three_to_five_and_alignment(kz, torch, settings, fx):
    units = nine_units(fx)
    res, dc, dp = device_call(kz, torch, settings, units, proofs=True)
    assert res == [None] * 9
    rc, st, hc, hp = c_call(kz, settings, units[3:6])            # a host call of units 3 to 5 alone
    assert rc == 0 and dc[3 * ROW:6 * ROW] == hc and dp[3 * PROOFS:6 * PROOFS] == hp
    assert hc == b"".join(b"".join(fx["cells"][j % 3]) for j in (3, 4, 5))
    # a refused unit on the device form, and a d_cells pointer 8 bytes off
    bad, _ = five_units(fx)
    res, dc, dp = device_call(kz, torch, settings, bad, proofs=True)
    assert [type(r).__name__ for r in res] == ["NoneType", "BadArgs", "NoneType", "BadArgs", "NoneType"]
    assert dc[2 * ROW:3 * ROW] == b"".join(fx["cells"][2]) and dp[4 * PROOFS:] == b"".join(fx["P"][1])
    m = 3
    d_in = u8(torch, bytes(8) + b"".join(b"".join(fx["cells"][b][:64]) for b in range(3)))
    out = torch.zeros(ROW * m, dtype=torch.uint8, device="cuda")
    counts, idx = (C.c_size_t * m)(64, 64, 64), (C.c_size_t * (64 * m))(*(list(range(64)) * m))
    fn = kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_many_sets_device
    st = (C.c_int * m)(7, 7, 7)
    assert fn(out.data_ptr(), None, st, counts, idx, d_in.data_ptr() + 8, m, settings.handle) == BADARGS and list(st) == [BADARGS] * m
    assert fn(None, None, st, counts, idx, d_in.data_ptr() + 16, m, settings.handle) == BADARGS
    aligned = u8(torch, b"".join(b"".join(fx["cells"][b][:64]) for b in range(3)))
    assert fn(out.data_ptr(), None, st, counts, idx, aligned.data_ptr(), m, settings.handle) == 0 and list(st) == [0] * m
    assert bytes(out.cpu().numpy()) == b"".join(b"".join(fx["cells"][b]) for b in range(3))


# ---- 9. the shared-set call is the special case of equal lists
def test_shared_set_call_and_five_equal_lists(kz, settings, fx):
    ix = index_sets()[4][1]
    rows = [[fx["cells"][b % 3][k] for k in ix] for b in range(5)]
    shared = kz.Kzg.recover_cells_and_kzg_proofs_many(ix, rows, settings)
    sets = kz.Kzg.recover_cells_and_kzg_proofs_many_sets([(ix, row) for row in rows], settings)
    for b in range(5):
        assert (raw(shared[b][0]), raw(shared[b][1])) == (raw(sets[b][0]), raw(sets[b][1])) == (fx["cells"][b % 3], fx["P"][b % 3]), b


# ---- 10. Python, C and C++ side by side
def test_python_c_and_cpp_agree(kz, settings, fx, tmp_path):
    sets = [s for _, s in index_sets()]
    units = [unit(fx["cells"][0], sets[6]), unit(fx["cells"][1], sets[4]), unit(fx["cells"][2], sets[7])]
    paths = [str(tmp_path / n) for n in ("counts.bin", "indices.bin", "cells.bin", "out.bin")]
    runner = os.path.join(HERE, "native", "cpp_cell_recover_sets_runner")
    setup = [os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin")]

    def run(us):
        for p, data in zip(paths, (bytes(len(ix) for ix, _ in us), bytes(i for ix, _ in us for i in ix), b"".join(b"".join(row) for _, row in us))):
            with open(p, "wb") as f:
                f.write(data)
        r = subprocess.run([runner] + setup + paths, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout.split("\n")[:-1], open(paths[3], "rb").read()

    lines, got = run(units)
    assert lines == ["ok"] * 3
    want = b"".join(b"".join(fx["cells"][b]) + b"".join(fx["P"][b]) for b in range(3))
    assert got == want
    rc, st, c_out, p_out = c_call(kz, settings, units)
    assert rc == 0 and b"".join(c_out[ROW * b:ROW * (b + 1)] + p_out[PROOFS * b:PROOFS * (b + 1)] for b in range(3)) == want
    py = kz.Kzg.recover_cells_and_kzg_proofs_many_sets(units, settings)
    assert b"".join(b"".join(raw(c)) + b"".join(raw(p)) for c, p in py) == want
    # a refusal through the mirror: a descending pair in the middle unit
    ix = list(range(62)) + [70, 69]
    lines, got = run([units[0], unit(fx["cells"][1], ix), units[2]])
    assert lines == ["ok", "err 1", "ok"]
    assert got == b"".join(b"".join(fx["cells"][b]) + b"".join(fx["P"][b]) for b in (0, 2))
