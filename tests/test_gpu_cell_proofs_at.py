"""-m gpu: compute_cell_kzg_proofs_at, the cells of a blob at chosen indices and their proofs, each proof the commitment to its own quotient
(DESIGN.md section 15).  Expected cells come from cell_spec.compute_cells and expected proofs from tests/golden/cells.json (oracle-derived) or
from closed forms, never from the call under test: the fixtures through the single call, the _many call and the C++ mirror on a bucket-form
and a wide-table handle; all 128 indices against the FK20 fixture; blobs whose quotients are known; statuses by position; the chunk border
against compute_cells_and_kzg_proofs_many; the device-resident form; replicas; the round trip through verify_cell_kzg_proof_batch; and the
calls that share the workspace's buffers before and after."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import threading

import pytest

import cell_spec as cs
import fk20_spec as fk
from synth import random_blob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R
BADARGS = 1
CELL, BLOB = 2048, 131072
G1_INF = fk.G1_INF
IDX = [0, 1, 63, 64, 127, 5, 5]
CQ_CHUNK = int(re.search(r"CQ_CHUNK = (\d+);", open(os.path.join(HERE, "..", "kzg_rust_amd", "csrc", "engine.h")).read()).group(1))


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


def want(fx, b, ix):
    return [fx["cells"][b][k] for k in ix], [fx["P"][b][k] for k in ix]


def c_many(kz, s, blobs, lists, cells=True, proofs=True, status=True):
    """the host form through ctypes: (return value, statuses, cells_out bytes, proofs_out bytes)"""
    n = len(blobs)
    flat = [i for ix in lists for i in ix]
    total = len(flat)
    counts, idx = (C.c_size_t * max(n, 1))(*[len(ix) for ix in lists]), (C.c_size_t * max(len(flat), 1))(*flat)
    c_out = C.create_string_buffer(CELL * max(total, 1)) if cells else None
    p_out = C.create_string_buffer(48 * max(total, 1)) if proofs else None
    st = (C.c_int * max(n, 1))(*([7] * max(n, 1))) if status else None
    rc = kz.kzg.lib().kzg355_compute_cell_kzg_proofs_at_many(c_out, p_out, st, b"".join(blobs), n, counts, idx, s.handle)
    return rc, list(st)[:n] if status else None, c_out.raw[:CELL * total] if cells else None, p_out.raw[:48 * total] if proofs else None


def many_lists():
    return [IDX, [], [127, 3, 3, 64, 0, 99]]


# ---- 1. the fixtures
def test_fixtures_single_call(kz, handle, fx):
    for b, blob in enumerate(fx["blobs"]):
        cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(blob), IDX, handle)
        assert (raw(cells), raw(proofs)) == want(fx, b, IDX), b
        assert raw(kz.Kzg.compute_kzg_cell_proofs_at(kz.Blob(blob), IDX, handle)) == want(fx, b, IDX)[1]
    # the C entry point with either output alone, and no index at all
    lib, blob = kz.kzg.lib(), fx["blobs"][0]
    idx = (C.c_size_t * len(IDX))(*IDX)
    c_out, p_out = C.create_string_buffer(CELL * len(IDX)), C.create_string_buffer(48 * len(IDX))
    assert lib.kzg355_compute_cell_kzg_proofs_at(c_out, None, blob, idx, len(IDX), handle.handle) == 0
    assert lib.kzg355_compute_cell_kzg_proofs_at(None, p_out, blob, idx, len(IDX), handle.handle) == 0
    assert (c_out.raw, p_out.raw) == tuple(b"".join(x) for x in want(fx, 0, IDX))
    assert lib.kzg355_compute_cell_kzg_proofs_at(c_out, p_out, blob, None, 0, handle.handle) == 0
    assert lib.kzg355_compute_cell_kzg_proofs_at(None, None, blob, idx, len(IDX), handle.handle) == BADARGS


def test_fixtures_many_call(kz, handle, fx):
    lists = many_lists()
    res = kz.Kzg.compute_cell_kzg_proofs_at_many([kz.Blob(b) for b in fx["blobs"]], lists, handle)
    assert [(raw(c), raw(p)) for c, p in res] == [want(fx, b, lists[b]) for b in range(3)]
    want_c = b"".join(b"".join(want(fx, b, lists[b])[0]) for b in range(3))
    want_p = b"".join(b"".join(want(fx, b, lists[b])[1]) for b in range(3))
    assert c_many(kz, handle, fx["blobs"], lists) == (0, [0] * 3, want_c, want_p)
    assert c_many(kz, handle, fx["blobs"], lists, proofs=False) == (0, [0] * 3, want_c, None)
    assert c_many(kz, handle, fx["blobs"], lists, cells=False) == (0, [0] * 3, None, want_p)
    assert c_many(kz, handle, fx["blobs"], lists, status=False) == (0, None, want_c, want_p)


def test_fixtures_cpp_mirror(fx, tmp_path):
    lists = many_lists()
    paths = [str(tmp_path / n) for n in ("blobs.bin", "counts.bin", "indices.bin", "out.bin")]
    for p, data in zip(paths, (b"".join(fx["blobs"]), bytes(len(ix) for ix in lists), bytes(i for ix in lists for i in ix))):
        with open(p, "wb") as f:
            f.write(data)
    runner = os.path.join(HERE, "native", "cpp_cell_proofs_at_runner")
    setup = [os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin")]
    expect = b"".join(b"".join(want(fx, b, lists[b])[0]) + b"".join(want(fx, b, lists[b])[1]) for b in range(3))
    for mode in ([], ["single"]):
        r = subprocess.run([runner] + setup + paths + mode, capture_output=True, text=True, timeout=600, env=dict(os.environ, KZG355_MSM="bucket"))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n")[:-1] == ["ok"] * 3
        assert open(paths[3], "rb").read() == expect, mode


# ---- 2. both routes agree: all 128 proofs of FK20
def test_all_128_indices_equal_fk20(kz, handle, fx):
    ix = list(range(128))
    cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(fx["blobs"][0]), ix, handle)
    assert raw(proofs) == fx["P"][0]
    assert raw(cells) == fx["cells"][0]


# ---- 3. closed forms
@pytest.mark.parametrize("k", [0, 1, 127])
def test_blob_of_x64_minus_a_k(kz, handle, mono, k):
    f = [0] * 65
    f[0], f[64] = (-fk.a_k(k)) % R, 1
    ix = [k, 0, 1, 64, 127, 77]
    cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(fk.blob_from_coefficients(f)), ix, handle)
    assert raw(proofs) == [mono[0]] * len(ix)                    # the quotient by X^64 - a_j is 1 at every j
    assert bytes(cells[0]) == bytes(CELL)                        # X^64 = a_k on the whole coset of cell k


def test_polynomial_below_degree_64(kz, handle):
    rng = random.Random(64)
    blob = fk.blob_from_coefficients([rng.randrange(R) for _ in range(64)])
    ix = [0, 1, 63, 64, 127]
    cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(blob), ix, handle)
    assert raw(proofs) == [G1_INF] * len(ix)
    full = cs.compute_cells(blob)
    assert raw(cells) == [full[k] for k in ix]


def test_blob_of_x4095(kz, handle, oracle, mono):
    blob = fk.blob_from_coefficients([0] * 4095 + [1])
    ix = [0, 1, 127]
    cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(blob), ix, handle)
    for k, p in zip(ix, proofs):
        a = fk.a_k(k)
        assert bytes(p) == fk.sparse_lincomb(oracle, [mono[64 * u + 63] for u in range(63)], [pow(a, 62 - u, R) for u in range(63)]), k
    full = cs.compute_cells(blob)
    assert raw(cells) == [full[k] for k in ix]


def test_zero_blob(kz, handle):
    cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(bytes(BLOB)), IDX, handle)
    assert raw(proofs) == [G1_INF] * len(IDX) and raw(cells) == [bytes(CELL)] * len(IDX)


# ---- 4. status by position
def test_status_by_position(kz, handle, fx):
    blobs = fx["blobs"]
    first, last = [64, 2], [127, 0, 9]
    wc0, wp0 = (b"".join(x) for x in want(fx, 0, first))
    wc2, wp2 = (b"".join(x) for x in want(fx, 2, last))
    spoiled = R.to_bytes(32, "big") + blobs[1][32:]
    cases = [("element", [blobs[0], spoiled, blobs[2]], [5, 6, 7]), ("index", blobs, [5, 128, 7]), ("count", blobs, [i % 128 for i in range(129)])]
    for name, bl, mid in cases:
        rc, st, c, p = c_many(kz, handle, bl, [first, mid, last])
        assert (rc, st) == (BADARGS, [0, BADARGS, 0]), name
        off = len(first) + len(mid)
        assert (c[:CELL * 2], p[:48 * 2]) == (wc0, wp0) and (c[CELL * off:], p[48 * off:]) == (wc2, wp2), name
        res = kz.Kzg.compute_cell_kzg_proofs_at_many([kz.Blob(b) for b in bl], [first, mid, last], handle)
        assert type(res[1]).__name__ == "BadArgs" and (raw(res[0][0]), raw(res[0][1])) == want(fx, 0, first), name
        assert (raw(res[2][0]), raw(res[2][1])) == want(fx, 2, last), name
        with pytest.raises(kz.BadArgs):
            kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(bl[1]), mid, handle)
    # a count of 0 in the middle is no error and shifts nothing; its blob is still checked
    assert c_many(kz, handle, blobs, [first, [], last]) == (0, [0, 0, 0], wc0 + wc2, wp0 + wp2)
    assert c_many(kz, handle, [blobs[0], spoiled, blobs[2]], [first, [], last]) == (BADARGS, [0, BADARGS, 0], wc0 + wc2, wp0 + wp2)


# ---- 5. the chunk border, against the FK20 call of the same handle
@pytest.mark.parametrize("n", [CQ_CHUNK // 128 + 1, CQ_CHUNK // 128])
def test_chunk_border(kz, s12, n):
    assert CQ_CHUNK % 128 == 0
    blobs = [random_blob(7594000 + i) for i in range(n)]
    lib = kz.kzg.lib()
    full_c, full_p, st = C.create_string_buffer(128 * CELL * n), C.create_string_buffer(128 * 48 * n), (C.c_int * n)()
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(full_c, full_p, st, b"".join(blobs), n, s12.handle) == 0
    rng = random.Random(n)
    lists = [rng.sample(range(128), 128) for _ in range(n)]
    rc, st, c, p = c_many(kz, s12, blobs, lists)
    assert (rc, st) == (0, [0] * n)
    fc, fp = full_c.raw, full_p.raw
    for j, (b, k) in enumerate((b, k) for b in range(n) for k in lists[b]):
        assert c[CELL * j:CELL * (j + 1)] == fc[CELL * (128 * b + k):CELL * (128 * b + k + 1)], (b, k)
        assert p[48 * j:48 * (j + 1)] == fp[48 * (128 * b + k):48 * (128 * b + k + 1)], (b, k)


# ---- 6. the device form
def test_device_form(kz, handle, fx):
    import torch
    lists = many_lists()
    counts, flat = [len(ix) for ix in lists], [i for ix in lists for i in ix]
    total = len(flat)
    want_c = b"".join(b"".join(want(fx, b, lists[b])[0]) for b in range(3))
    want_p = b"".join(b"".join(want(fx, b, lists[b])[1]) for b in range(3))
    d_blobs = torch.frombuffer(bytearray(b"".join(fx["blobs"])), dtype=torch.uint8).cuda()
    for cells, proofs in ((True, False), (False, True), (True, True)):
        dc = torch.zeros(CELL * total, dtype=torch.uint8, device="cuda") if cells else None
        dp = torch.zeros(48 * total, dtype=torch.uint8, device="cuda") if proofs else None
        assert kz.Kzg.compute_cell_kzg_proofs_at_many_device(d_blobs, 3, counts, flat, handle, cells_out=dc, proofs_out=dp) == [None] * 3
        assert dc is None or bytes(dc.cpu().numpy()) == want_c
        assert dp is None or bytes(dp.cpu().numpy()) == want_p
    # a pointer misaligned by 8 refuses the call as a whole
    pad = torch.zeros(BLOB * 3 + 16, dtype=torch.uint8, device="cuda")
    dc, dp = torch.zeros(CELL * total + 16, dtype=torch.uint8, device="cuda"), torch.zeros(48 * total + 16, dtype=torch.uint8, device="cuda")
    cn, ix = (C.c_size_t * 3)(*counts), (C.c_size_t * total)(*flat)
    call = kz.kzg.lib().kzg355_compute_cell_kzg_proofs_at_many_device
    for shift in ((8, 0, 0), (0, 8, 0), (0, 0, 8)):
        st = (C.c_int * 3)(7, 7, 7)
        assert call(dc.data_ptr() + shift[0], dp.data_ptr() + shift[1], st, pad.data_ptr() + shift[2], 3, cn, ix, handle.handle) == BADARGS
        assert list(st) == [BADARGS] * 3
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cell_kzg_proofs_at_many_device(d_blobs, 3, counts, flat, handle)


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
        blobs = fx["blobs"] + [random_blob(7594100), random_blob(7594101)]
        lists = [[rng.randrange(128) for _ in range(c)] for c in (3, 0, 128, 1, 7)]
        single = c_many(kz, s8, blobs, lists)
        assert single[:2] == (0, [0] * 5)
        assert single[2][:CELL * 3] == b"".join(want(fx, 0, lists[0])[0]) and single[3][:48 * 3] == b"".join(want(fx, 0, lists[0])[1])
        assert single[3][48 * 3:48 * 131] == b"".join(want(fx, 2, lists[2])[1])
        before = s3.cell_calls_per_device()
        assert c_many(kz, s3, blobs, lists) == single
        assert [a - b for a, b in zip(s3.cell_calls_per_device(), before)] == [1, 1, 1]      # ranges of 1, 2 and 2 blobs
        # a refusal lands at its own position on its own replica
        lists[3] = [128]
        rc, st, c, p = c_many(kz, s3, blobs, lists)
        assert (rc, st) == (BADARGS, [0, 0, 0, BADARGS, 0])
        assert (c[:CELL * 131], p[:48 * 131]) == (single[2][:CELL * 131], single[3][:48 * 131])
        assert (c[CELL * 132:], p[48 * 132:]) == (single[2][CELL * 132:], single[3][48 * 132:])
    finally:
        s3.free()


# ---- 8. round trip through the cell batch check
def test_round_trip(kz, handle, fx):
    blob = kz.Blob(fx["blobs"][1])
    ix = [3, 127, 64, 0, 3]
    cells, proofs = kz.Kzg.compute_cell_kzg_proofs_at(blob, ix, handle)
    c = kz.Kzg.blob_to_kzg_commitment(blob, handle)
    assert bytes(c) == bytes.fromhex(fx["commitments"][1])
    assert kz.Kzg.verify_cell_kzg_proof_batch([c] * len(ix), ix, cells, proofs, handle) is True
    swapped = [proofs[1], proofs[0]] + list(proofs[2:])
    assert kz.Kzg.verify_cell_kzg_proof_batch([c] * len(ix), ix, cells, swapped, handle) is False


# ---- 9. neighbours: the calls that share the workspace's buffers, the first call from two threads, a minimal-preset handle
def test_neighbours_before_and_after(kz, handle, fx):
    blobs = [kz.Blob(b) for b in fx["blobs"]]

    def blob_path():
        cms = kz.Kzg.blob_to_kzg_commitment_many(blobs, handle)
        return raw(cms), raw(kz.Kzg.compute_blob_kzg_proof_many(blobs, cms, handle))

    def fk20():
        c, p = kz.Kzg.compute_cells_and_kzg_proofs(blobs[2], handle)
        return raw(c), raw(p)

    before, before_fk = blob_path(), fk20()
    assert before[0] == [bytes.fromhex(x) for x in fx["commitments"]] and before_fk == (fx["cells"][2], fx["P"][2])
    res = kz.Kzg.compute_cell_kzg_proofs_at_many(blobs, [list(range(128)), IDX, [7] * 40], handle)
    assert [(raw(c), raw(p)) for c, p in res] == [want(fx, 0, list(range(128))), want(fx, 1, IDX), want(fx, 2, [7] * 40)]
    assert blob_path() == before and fk20() == before_fk


def test_first_call_from_two_threads(kz, setup_bytes, fx):
    s = _load(kz, setup_bytes, msm_bits=12)
    out = [None, None]

    def work(t):
        out[t] = kz.Kzg.compute_cell_kzg_proofs_at(kz.Blob(fx["blobs"][t]), IDX, s)

    try:
        assert s.msm_shape()[0] == 0
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for t in range(2):
            assert out[t] is not None and (raw(out[t][0]), raw(out[t][1])) == want(fx, t, IDX), t
        assert s.msm_shape()[0] == 12                            # the first call that wanted proofs built the table
    finally:
        s.free()


def test_cells_alone_build_no_table(kz, setup_bytes, s8, s12, fx):
    s = _load(kz, setup_bytes, msm_bits=12)
    try:
        rc, st, c, _ = c_many(kz, s, fx["blobs"], many_lists(), proofs=False)
        assert (rc, st) == (0, [0] * 3) and c == b"".join(b"".join(want(fx, b, ix)[0]) for b, ix in enumerate(many_lists()))
        assert s.msm_shape()[0] == 0
    finally:
        s.free()
    # the module's two handles are what their names say
    kz.Kzg.compute_kzg_cell_proofs_at(kz.Blob(fx["blobs"][0]), [0], s12)
    kz.Kzg.compute_kzg_cell_proofs_at(kz.Blob(fx["blobs"][0]), [0], s8)
    assert s12.msm_shape()[0] == 12 and s12.msm_form == 12 and s8.msm_shape()[0] == 0 and s8.msm_form == 8


def test_minimal_preset_handle_refuses(kz, setup_bytes, fx):
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        lib, blob = kz.kzg.lib(), fx["blobs"][0]
        idx = (C.c_size_t * 2)(0, 1)
        c_out, p_out = C.create_string_buffer(CELL * 2), C.create_string_buffer(48 * 2)
        assert lib.kzg355_compute_cell_kzg_proofs_at(c_out, p_out, blob, idx, 2, sm.handle) == BADARGS
        assert c_many(kz, sm, [blob, blob], [[0], [1]])[:2] == (BADARGS, [BADARGS, BADARGS])
    finally:
        sm.free()
