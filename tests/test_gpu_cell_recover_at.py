"""-m gpu: recover_cells_and_kzg_proofs_at, the chosen cells of recovered blobs and their proofs: the recovery of
recover_cells_and_kzg_proofs, then every wanted (blob, cell) pair through its own quotient and one MSM.  Expected
cells come from cell_spec.compute_cells and expected proofs from tests/golden/cells.json (oracle-derived), built once in
tests/recover_at_cases.py and pinned on the CPU by tests/test_recover_at_cases.py; where no fixture exists they come from the full recovery
calls, never from the calls under test.  The nine shapes of index set with three kinds of want list on a bucket-form and a wide-table
handle; the single call, the C++ mirror and the Python helper; statuses by position; an inconsistent unit; the chunk borders; the
device-resident form; replicas; the round trip through verify_cell_kzg_proof_batch; the calls that share the workspace's buffers before and
after; and the table, two threads and a minimal-preset handle."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import threading

import pytest

import recover_at_cases as cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BADARGS = 1
CELL, ROW, PROOFS = 2048, 128 * 2048, 128 * 48
ENGINE_H = open(os.path.join(HERE, "..", "kzg_rust_amd", "csrc", "engine.h")).read()
CQ_CHUNK = int(re.search(r"CQ_CHUNK = (\d+);", ENGINE_H).group(1))
CC_CHUNK = int(re.search(r"CC_CHUNK = (\d+);", ENGINE_H).group(1))


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, **options):
    g1, g2 = setup_bytes
    return kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], **options)


@pytest.fixture(scope="module")
def s8(kz, setup_bytes):
    """bucket form, no table"""
    s = _load(kz, setup_bytes, msm_bits=8)
    yield s
    s.free()


@pytest.fixture(scope="module")
def s12(kz, setup_bytes):
    """the smallest wide table"""
    s = _load(kz, setup_bytes, msm_bits=12)
    yield s
    s.free()


@pytest.fixture(scope="module", params=["bucket", "wide"])
def handle(request, s8, s12):
    return s8 if request.param == "bucket" else s12


@pytest.fixture(scope="module")
def fx():
    return cases.fixture()


def raw(xs):
    return [bytes(x) for x in xs]


def arrays(units):
    """the four host arrays of a call and its known cells: (cell_counts, cell_indices, cells bytes, want_counts, want_indices, slots)"""
    m = len(units)
    kflat = [i for ix, _, _ in units for i in ix]
    wflat = [i for _, _, w in units for i in w]
    sz = lambda v: (C.c_size_t * max(len(v), 1))(*v)               # noqa: E731
    return (sz([len(ix) for ix, _, _ in units]), sz(kflat), b"".join(b"".join(row) for _, row, _ in units), sz([len(w) for _, _, w in units]),
            sz(wflat), len(wflat)) if m else (None, None, None, None, None, 0)


def c_sets(kz, s, units, cells=True, proofs=True, status=True):
    """the host form through ctypes: (return value, statuses, cells_out bytes, proofs_out bytes)"""
    m = len(units)
    kc, ki, data, wc, wi, total = arrays(units)
    c_out = C.create_string_buffer(CELL * max(total, 1)) if cells else None
    p_out = C.create_string_buffer(48 * max(total, 1)) if proofs else None
    st = (C.c_int * max(m, 1))(*([7] * max(m, 1))) if status else None
    rc = kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_at_many_sets(c_out, p_out, st, kc, ki, data, wc, wi, m, s.handle)
    return rc, list(st)[:m] if status else None, c_out.raw[:CELL * total] if cells else None, p_out.raw[:48 * total] if proofs else None


def full_sets(kz, s, units):
    """the full recovery of the parent commit on the same known cells: (cells_out, proofs_out), 128 per unit"""
    m = len(units)
    kc, ki, data, _, _, _ = arrays(units)
    c_out, p_out, st = C.create_string_buffer(ROW * m), C.create_string_buffer(PROOFS * m), (C.c_int * m)()
    assert kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_many_sets(c_out, p_out, st, kc, ki, data, m, s.handle) == 0
    return c_out.raw, p_out.raw


def picked(full_c, full_p, units):
    """what the units' want lists pick out of the full recovery's outputs"""
    pairs = [(b, k) for b, (_, _, w) in enumerate(units) for k in w]
    return (b"".join(full_c[ROW * b + CELL * k:ROW * b + CELL * (k + 1)] for b, k in pairs),
            b"".join(full_p[PROOFS * b + 48 * k:PROOFS * b + 48 * (k + 1)] for b, k in pairs))


# ---- 1. the nine shapes of index set, three kinds of want list, every output combination
@pytest.mark.parametrize("kind", cases.WANT_KINDS)
def test_nine_index_set_shapes(kz, handle, kind):
    units, exp = cases.nine(kind)
    want_c, want_p = cases.flat(exp)
    assert c_sets(kz, handle, units) == (0, [0] * 9, want_c, want_p)
    assert c_sets(kz, handle, units, proofs=False) == (0, [0] * 9, want_c, None)
    assert c_sets(kz, handle, units, cells=False) == (0, [0] * 9, None, want_p)
    assert c_sets(kz, handle, units, status=False) == (0, None, want_c, want_p)
    res = kz.Kzg.recover_cells_and_kzg_proofs_at_many_sets(units, handle)
    assert [(raw(c), raw(p)) for c, p in res] == [(c, p) for c, p in exp]


# ---- 2. the single call, the C++ mirror and the Python helper
def test_single_call(kz, handle):
    units, exp = cases.nine("fixed")
    for j in (0, 5, 8):
        ix, cells, want = units[j]
        c, p = kz.Kzg.recover_cells_and_kzg_proofs_at(ix, cells, want, handle)
        assert (raw(c), raw(p)) == exp[j], j
    # the C entry point with either output alone, and no wanted index at all
    lib = kz.kzg.lib()
    ix, cells, want = units[4]
    kc, ki, data, wc, wi, total = arrays([units[4]])
    c_out, p_out = C.create_string_buffer(CELL * total), C.create_string_buffer(48 * total)
    fn = lib.kzg355_recover_cells_and_kzg_proofs_at
    assert fn(c_out, None, ki, data, len(ix), wi, total, handle.handle) == 0
    assert fn(None, p_out, ki, data, len(ix), wi, total, handle.handle) == 0
    assert (c_out.raw, p_out.raw) == cases.flat([exp[4]])
    assert fn(c_out, p_out, ki, data, len(ix), None, 0, handle.handle) == 0
    assert fn(None, None, ki, data, len(ix), wi, total, handle.handle) == BADARGS
    assert (c_out.raw, p_out.raw) == cases.flat([exp[4]])


def test_cpp_mirror(tmp_path):
    units, exp = cases.nine("fixed")
    pick = [6, 4, 8]
    us, ex = [units[j] for j in pick], [exp[j] for j in pick]
    paths = [str(tmp_path / n) for n in ("counts.bin", "indices.bin", "cells.bin", "want_counts.bin", "want_indices.bin", "out.bin")]
    data = (bytes(len(ix) for ix, _, _ in us), bytes(i for ix, _, _ in us for i in ix), b"".join(b"".join(row) for _, row, _ in us),
            bytes(len(w) for _, _, w in us), bytes(i for _, _, w in us for i in w))
    for p, d in zip(paths, data):
        with open(p, "wb") as f:
            f.write(d)
    runner = os.path.join(HERE, "native", "cpp_cell_recover_at_runner")
    setup = [os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin")]
    expect = b"".join(b"".join(c) + b"".join(p) for c, p in ex)
    for mode in ([], ["single"]):
        r = subprocess.run([runner] + setup + paths + mode, capture_output=True, text=True, timeout=600, env=dict(os.environ, KZG355_MSM="bucket"))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n")[:-1] == ["ok"] * 3
        assert open(paths[5], "rb").read() == expect, mode


def test_python_helper_returns_the_complement(kz, s12, fx):
    for j, (name, ix) in enumerate(cases.index_sets()):
        b = j % 3
        missing, c, p = kz.Kzg.recover_missing_cells_and_kzg_proofs(ix, [fx["cells"][b][k] for k in ix], s12)
        assert missing == [k for k in range(128) if k not in ix], name
        assert (raw(c), raw(p)) == cases.expected(b, missing), name
    assert missing == [] and c == [] and p == []                   # all128: nothing is missing


# ---- 3. status by position
@pytest.mark.parametrize("row", range(9))
def test_status_by_position(kz, handle, row):
    name, units, statuses, (e_left, e_right) = cases.refusals()[row]
    rc, st, c, p = c_sets(kz, handle, units)
    assert (rc, st) == (BADARGS if 1 in statuses else 0, statuses), name
    nl, nm, nr = (len(u[2]) for u in units)
    assert (c[:CELL * nl], p[:48 * nl]) == cases.flat([e_left]), name
    assert (c[CELL * (nl + nm):], p[48 * (nl + nm):]) == cases.flat([e_right]), name      # the layout follows the counts as given
    assert len(c) == CELL * (nl + nm + nr)
    res = kz.Kzg.recover_cells_and_kzg_proofs_at_many_sets(units, handle)
    assert (raw(res[0][0]), raw(res[0][1])) == e_left and (raw(res[2][0]), raw(res[2][1])) == e_right, name
    if statuses[1]:
        assert isinstance(res[1], kz.BadArgs), name
        with pytest.raises(kz.BadArgs):
            kz.Kzg.recover_cells_and_kzg_proofs_at(*units[1], handle)
    else:
        assert res[1] == ([], []), name


# ---- 4. more than 64 cells on no polynomial of degree < 4096, next to a consistent unit
def test_inconsistent_input(kz, handle):
    units, _, exp_cells, exp_good = cases.inconsistent()
    ix, bad, want = units[0]
    full = kz.Kzg.recover_cells_and_kzg_proofs(ix, bad, handle)    # the existing call on the same input
    exp_proofs = [bytes(full[1][k]) for k in want]
    assert [bytes(full[0][k]) for k in want] == exp_cells
    rc, st, c, p = c_sets(kz, handle, units)
    assert (rc, st) == (0, [0, 0])
    assert (c, p) == cases.flat([(exp_cells, exp_proofs), exp_good])
    single = kz.Kzg.recover_cells_and_kzg_proofs_at(ix, bad, want, handle)
    assert (raw(single[0]), raw(single[1])) == (exp_cells, exp_proofs)


# ---- 5. chunk borders, against the full recovery of the same handle
@pytest.mark.parametrize("n", [CQ_CHUNK // 128 + 1, CQ_CHUNK // 128])
def test_pair_chunk_border(kz, s12, fx, n):
    assert CQ_CHUNK % 128 == 0
    rng = random.Random(n)
    units = []
    for b in range(n):
        ix = sorted(rng.sample(range(128), 64))
        units.append((ix, [fx["cells"][b % 3][k] for k in ix], rng.sample(range(128), 128)))
    rc, st, c, p = c_sets(kz, s12, units)
    assert (rc, st) == (0, [0] * n)
    assert (c, p) == picked(*full_sets(kz, s12, units), units)
    assert c[:CELL * 128] == b"".join(fx["cells"][0][k] for k in units[0][2])


def test_blob_chunk_border(kz, s12, fx):
    n = CC_CHUNK + 1
    sets = [cases.index_sets()[j][1] for j in (0, 1, 4)]           # first64, last64, random64
    rows = [[[fx["cells"][b][k] for k in ix] for ix in sets] for b in range(3)]
    units = [(sets[(i // 3) % 3], rows[i % 3][(i // 3) % 3], [(5 * i + 3) % 128]) for i in range(n)]
    rc, st, c, p = c_sets(kz, s12, units)
    assert (rc, st) == (0, [0] * n)
    assert (c, p) == picked(*full_sets(kz, s12, units), units)
    for i in (0, CC_CHUNK - 1, CC_CHUNK):                          # the fixture at both sides of the border
        k = units[i][2][0]
        assert (c[CELL * i:CELL * (i + 1)], p[48 * i:48 * (i + 1)]) == (fx["cells"][i % 3][k], fx["P"][i % 3][k]), i


# ---- 6. the device form
def test_device_form(kz, handle):
    import torch
    units, _ = cases.nine("fixed")
    units = units + [cases.refusals()[7][1][1]]                    # and a unit that wants nothing
    m = len(units)
    _, host_st, host_c, host_p = c_sets(kz, handle, units)
    assert host_st == [0] * m
    counts, kflat = [len(ix) for ix, _, _ in units], [i for ix, _, _ in units for i in ix]
    wcounts, wflat = [len(w) for _, _, w in units], [i for _, _, w in units for i in w]
    total = len(wflat)
    d_cells = torch.frombuffer(bytearray(b"".join(b"".join(row) for _, row, _ in units)), dtype=torch.uint8).cuda()
    call = kz.Kzg.recover_cells_and_kzg_proofs_at_many_sets_device
    for cells, proofs in ((True, False), (False, True), (True, True)):
        dc = torch.zeros(CELL * total, dtype=torch.uint8, device="cuda") if cells else None
        dp = torch.zeros(48 * total, dtype=torch.uint8, device="cuda") if proofs else None
        assert call(counts, kflat, d_cells, wcounts, wflat, handle, cells_out=dc, proofs_out=dp) == [None] * m
        assert dc is None or bytes(dc.cpu().numpy()) == host_c
        assert dp is None or bytes(dp.cpu().numpy()) == host_p
    # a refused unit on the device form: its neighbours' slots are the host form's
    name, bad_units, statuses, _ = cases.refusals()[5]
    _, _, bad_c, bad_p = c_sets(kz, handle, bad_units)
    bw = [i for _, _, w in bad_units for i in w]
    d_bad = torch.frombuffer(bytearray(b"".join(b"".join(row) for _, row, _ in bad_units)), dtype=torch.uint8).cuda()
    dc, dp = torch.zeros(CELL * len(bw), dtype=torch.uint8, device="cuda"), torch.zeros(48 * len(bw), dtype=torch.uint8, device="cuda")
    res = call([len(ix) for ix, _, _ in bad_units], [i for ix, _, _ in bad_units for i in ix], d_bad, [len(w) for _, _, w in bad_units], bw, handle,
               cells_out=dc, proofs_out=dp)
    assert [type(r).__name__ for r in res] == ["NoneType", "BadArgs", "NoneType"], name
    got_c, got_p = bytes(dc.cpu().numpy()), bytes(dp.cpu().numpy())
    assert (got_c[:CELL * 2], got_p[:48 * 2]) == (bad_c[:CELL * 2], bad_p[:48 * 2]) and (got_c[CELL * 5:], got_p[48 * 5:]) == (bad_c[CELL * 5:], bad_p[48 * 5:])
    # a pointer misaligned by 8 refuses the call as a whole
    kc, ki, data, wc, wi, _ = arrays(units)
    pad = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    dc, dp = torch.zeros(CELL * total + 16, dtype=torch.uint8, device="cuda"), torch.zeros(48 * total + 16, dtype=torch.uint8, device="cuda")
    fn = kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_at_many_sets_device
    for shift in ((8, 0, 0), (0, 8, 0), (0, 0, 8)):
        st = (C.c_int * m)(*([7] * m))
        assert fn(dc.data_ptr() + shift[0], dp.data_ptr() + shift[1], st, kc, ki, pad.data_ptr() + shift[2], wc, wi, m, handle.handle) == BADARGS
        assert list(st) == [BADARGS] * m
    with pytest.raises(kz.BadArgs):
        call(counts, kflat, d_cells, wcounts, wflat, handle)


# ---- 7. replicas on one card
def test_replicas(kz, s8, setup_bytes, fx):
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer")     # no wide table per replica
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s3 = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], devices=[0, 0, 0])
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        assert s3.device_count == 3
        rng = random.Random(5)
        sets = [s for _, s in cases.index_sets()]
        known = [sets[5], sets[6], sets[4], sets[7], sets[2]]      # 65, 100, 64, 127 and 64 cells: the two prefix sums differ at every range
        units = [cases.unit(b % 3, known[b], [rng.randrange(128) for _ in range(c)]) for b, c in enumerate((3, 0, 64, 1, 7))]
        single = c_sets(kz, s8, units)
        assert single[:2] == (0, [0] * 5)
        assert (single[2], single[3]) == cases.flat([cases.expected(b % 3, units[b][2]) for b in range(5)])
        before = s3.cell_calls_per_device()
        assert c_sets(kz, s3, units) == single
        assert [a - b for a, b in zip(s3.cell_calls_per_device(), before)] == [1, 1, 1]      # ranges of 1, 2 and 2 blobs
        # a refusal lands at its own position on its own replica
        units[3] = (units[3][0], units[3][1], [128])
        rc, st, c, p = c_sets(kz, s3, units)
        assert (rc, st) == (BADARGS, [0, 0, 0, BADARGS, 0])
        assert (c[:CELL * 67], p[:48 * 67]) == (single[2][:CELL * 67], single[3][:48 * 67])
        assert (c[CELL * 68:], p[48 * 68:]) == (single[2][CELL * 68:], single[3][48 * 68:])
    finally:
        s3.free()


# ---- 8. round trip through the cell batch check
def test_round_trip(kz, handle, fx):
    ix = cases.index_sets()[6][1]                                  # 100 known cells of fixture blob 1
    missing, cells, proofs = kz.Kzg.recover_missing_cells_and_kzg_proofs(ix, [fx["cells"][1][k] for k in ix], handle)
    assert len(missing) == 28
    c = kz.KzgCommitment(bytes.fromhex(fx["commitments"][1]))
    assert kz.Kzg.verify_cell_kzg_proof_batch([c] * 28, missing, cells, proofs, handle) is True
    swapped = [proofs[1], proofs[0]] + list(proofs[2:])
    assert kz.Kzg.verify_cell_kzg_proof_batch([c] * 28, missing, cells, swapped, handle) is False


# ---- 9. neighbours: the calls that share the workspace's buffers
def test_neighbours_before_and_after(kz, handle, fx):
    blobs = [kz.Blob(b) for b in fx["blobs"]]
    ix = cases.index_sets()[5][1]

    def blob_path():
        cms = kz.Kzg.blob_to_kzg_commitment_many(blobs, handle)
        return raw(cms), raw(kz.Kzg.compute_blob_kzg_proof_many(blobs, cms, handle))

    def full_recover():
        c, p = kz.Kzg.recover_cells_and_kzg_proofs(ix, [fx["cells"][2][k] for k in ix], handle)
        return raw(c), raw(p)

    def proofs_at():
        c, p = kz.Kzg.compute_cell_kzg_proofs_at(blobs[1], cases.FIXED, handle)
        return raw(c), raw(p)

    def cell_verify():
        c = kz.KzgCommitment(bytes.fromhex(fx["commitments"][0]))
        return kz.Kzg.verify_cell_kzg_proof_batch([c] * 3, [0, 64, 127], [fx["cells"][0][k] for k in (0, 64, 127)], [fx["P"][0][k] for k in (0, 64, 127)], handle)

    before = blob_path(), full_recover(), proofs_at(), cell_verify()
    assert before[0][0] == [bytes.fromhex(x) for x in fx["commitments"]] and before[1] == (fx["cells"][2], fx["P"][2])
    assert before[2] == cases.expected(1, cases.FIXED) and before[3] is True
    for kind in ("shuffled", "missing"):
        units, exp = cases.nine(kind)
        res = kz.Kzg.recover_cells_and_kzg_proofs_at_many_sets(units[:4], handle)
        assert [(raw(c), raw(p)) for c, p in res] == exp[:4]
        assert (blob_path(), full_recover(), proofs_at(), cell_verify()) == before, kind


# ---- 10. the table, two threads, a minimal-preset handle
def test_cells_alone_build_no_table(kz, setup_bytes, s8, s12, fx):
    s = _load(kz, setup_bytes, msm_bits=12)
    try:
        units, exp = cases.nine("fixed")
        rc, st, c, _ = c_sets(kz, s, units, proofs=False)
        assert (rc, st) == (0, [0] * 9) and c == cases.flat(exp)[0]
        assert s.msm_shape()[0] == 0
    finally:
        s.free()
    # the module's two handles are what their names say
    for h in (s12, s8):
        kz.Kzg.recover_cells_and_kzg_proofs_at(*cases.nine("fixed")[0][0], h)
    assert s12.msm_shape()[0] == 12 and s12.msm_form == 12 and s8.msm_shape()[0] == 0 and s8.msm_form == 8


def test_first_call_from_two_threads(kz, setup_bytes):
    s = _load(kz, setup_bytes, msm_bits=12)
    units, exp = cases.nine("fixed")
    out = [None, None]

    def work(t):
        out[t] = kz.Kzg.recover_cells_and_kzg_proofs_at(*units[t + 4], s)

    try:
        assert s.msm_shape()[0] == 0
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for t in range(2):
            assert out[t] is not None and (raw(out[t][0]), raw(out[t][1])) == exp[t + 4], t
        assert s.msm_shape()[0] == 12                            # the first call that wanted proofs built the table, once
    finally:
        s.free()


def test_minimal_preset_handle_refuses(kz, setup_bytes):
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        units, _ = cases.nine("fixed")
        assert c_sets(kz, sm, units[:2])[:2] == (BADARGS, [BADARGS, BADARGS])
        kc, ki, data, wc, wi, total = arrays([units[0]])
        c_out, p_out = C.create_string_buffer(CELL * total), C.create_string_buffer(48 * total)
        assert kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_at(c_out, p_out, ki, data, 64, wi, total, sm.handle) == BADARGS
    finally:
        sm.free()
