"""-m gpu: the three EIP-7594 cell calls on device-resident data (kzg355_*_many_device).  Device memory is torch tensors.  The verify call is run
with its preparation pinned to the device kernels (prep_form 1) and to the host (prep_form 2): intermediates byte for byte against
tests/golden/cells.json, verdict and status parity with the host form on valid / tampered / malformed batches, a seeded differential fuzz, and
the route a prep_form 0 call takes by its shape.  Compute and recover write into device tensors that must equal the host forms' outputs, and one
test chains compute -> verify -> recover without a cell ever visiting the host."""
import ctypes as C
import random

import pytest

import cell_spec as cs
import cell_device_cases as cases
from synth import random_blob

pytestmark = pytest.mark.gpu

R = cs.R
CELL, ROW = 2048, 128 * 2048


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def settings(kz, setup_bytes):
    g1, g2 = setup_bytes
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    return cases.fixture()


def u8(torch, data):
    return torch.frombuffer(bytearray(data) if len(data) else bytearray(1), dtype=torch.uint8)[:len(data)].cuda()


def to_device(torch, groups):
    """groups of (commitments, indices, cells, proofs), all of one size -> the four group-major device tensors"""
    idx = [int(i) for g in groups for i in g[1]]
    return (u8(torch, b"".join(b"".join(g[0]) for g in groups)),
            torch.tensor([i - (1 << 64) if i >= 1 << 63 else i for i in idx], dtype=torch.int64).cuda(),
            u8(torch, b"".join(b"".join(g[2]) for g in groups)), u8(torch, b"".join(b"".join(g[3]) for g in groups)))


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def device_verdicts(kz, torch, groups, settings, prep_form):
    d = to_device(torch, groups)
    res, out = kz.Kzg.debug_cell_batch_intermediates_device(*d, len(groups[0][0]), len(groups), settings, prep_form=prep_form)
    return norm(res), out


def raw_status(kz, torch, groups, settings, prep_form):
    """ok[] and status[] as the C call leaves them"""
    d = to_device(torch, groups)
    G = len(groups)
    ok, st, out = (C.c_bool * G)(), (C.c_int * G)(), C.create_string_buffer(176 * G)
    rc = kz.kzg.lib().kzg355_debug_cell_batch_intermediates_device(out, ok, st, *[t.data_ptr() for t in d], len(groups[0][0]), G, prep_form, settings.handle)
    return rc, list(ok), list(st)


def host_status(kz, groups, settings):
    G = len(groups)
    ok, st = (C.c_bool * G)(), (C.c_int * G)()
    idx = [i for g in groups for i in g[1]]
    rc = kz.kzg.lib().kzg355_verify_cell_kzg_proof_batch_many(ok, st, b"".join(b"".join(g[0]) for g in groups), (C.c_size_t * len(idx))(*idx),
                                                               b"".join(b"".join(g[2]) for g in groups), b"".join(b"".join(g[3]) for g in groups),
                                                               len(groups[0][0]), G, settings.handle)
    return rc, list(ok), list(st)


# ---- 1. intermediates, byte for byte, on both preparations
@pytest.mark.parametrize("prep_form", [1, 2])
def test_intermediates_byte_exact(kz, torch, settings, fx, prep_form):
    assert len(fx["batches"]) >= 4
    for b in fx["batches"]:
        res, out = device_verdicts(kz, torch, [cases.batch(fx, [tuple(x) for x in b["items"]])], settings, prep_form)
        assert res == [True], b["name"]
        o = out[0]
        assert (o[:32].hex(), o[32:80].hex(), o[80:128].hex(), o[128:176].hex()) == (b["r"], b["itau"], b["ll"], b["rl"]), b["name"]


# ---- 2. verdict parity with the host form
def parity_cases(fx, oracle):
    B = lambda items: cases.batch(fx, items)
    out = {}
    out["one_cell"] = B([(0, 9)])
    out["column"] = B([(b, 33) for b in range(3)])
    out["row"] = B([(2, k) for k in range(128)])
    out["repeats"] = B([(0, 1), (1, 1), (0, 1), (2, 127), (1, 64), (1, 64), (0, 90), (2, 5)])
    c, i, cl, p = B([(0, 3), (1, 70), (2, 11)])
    out["swapped_proofs"] = (c, i, cl, [p[1], p[0], p[2]])
    bad = bytearray(cl[1]); bad[31] ^= 1
    out["changed_element"] = (c, i, [cl[0], bytes(bad), cl[2]], p)
    out["wrong_index"] = (c, [3, 71, 11], cl, p)
    out["wrong_commitment"] = ([c[0], c[2], c[2]], i, cl, p)
    out["index_128"] = (c, [3, 128, 11], cl, p)
    out["index_huge"] = (c, [3, 70, (1 << 64) - 1], cl, p)
    nc = cl[0][:32 * 7] + R.to_bytes(32, "big") + cl[0][32 * 8:]
    out["non_canonical"] = (c, i, [nc, cl[1], cl[2]], p)
    flags = bytearray(c[0]); flags[0] &= 0x7f
    for name, pt in (("off_curve", cases.off_curve(oracle)), ("not_in_subgroup", cases.not_in_subgroup(oracle)), ("flags", bytes(flags))):
        assert pt is not None
        out["bad_commitment_" + name] = ([pt, c[1], c[2]], i, cl, p)
        out["bad_proof_" + name] = (c, i, cl, [p[0], pt, p[2]])
    return out


WANT = {"one_cell": True, "column": True, "row": True, "repeats": True, "swapped_proofs": False, "changed_element": False, "wrong_index": False,
        "wrong_commitment": False}


@pytest.mark.parametrize("prep_form", [1, 2])
def test_verdict_parity_with_the_host_form(kz, torch, settings, fx, oracle, prep_form):
    pc = parity_cases(fx, oracle)
    for name, grp in pc.items():
        host = host_status(kz, [grp], settings)
        dev = raw_status(kz, torch, [grp], settings, prep_form)
        assert dev == host, name
        want = WANT.get(name, "BadArgs")
        assert (host[1][0] if host[2][0] == 0 else "BadArgs") == want and (want != "BadArgs" or host[2][0] == kz.BadArgs.code), name
    # good and bad groups mixed in one _many call: every three-cell case side by side
    three = [n for n, g in pc.items() if len(g[0]) == 3]
    assert len(three) >= 12
    groups = [pc[n] for n in three]
    host = host_status(kz, groups, settings)
    assert raw_status(kz, torch, groups, settings, prep_form) == host
    assert [host[1][k] if host[2][k] == 0 else "BadArgs" for k in range(len(three))] == [WANT.get(n, "BadArgs") for n in three]


# ---- 3. seeded differential fuzz, device route against host route, r against the CPU transcript
def test_differential_fuzz(kz, torch, settings, fx, oracle):
    total, seen = 0, set()
    for npg, groups in cases.fuzz_groups(fx, cases.not_in_subgroup(oracle)):
        gs = [g for g, _ in groups]
        host = host_status(kz, gs, settings)
        d1, out1 = device_verdicts(kz, torch, gs, settings, 1)
        assert raw_status(kz, torch, gs, settings, 1) == host, npg
        assert raw_status(kz, torch, gs, settings, 2) == host, npg
        for t, ((grp, kind), got) in enumerate(zip(groups, d1)):
            assert (got == "BadArgs") == (kind == "malformed"), (npg, t, kind, got)
            assert kind != "valid" or got is True, (npg, t)
            seen.add(got)
            if t % 3 == 0:
                assert int.from_bytes(out1[t][:32], "big") == cs.challenge(*grp)[0], (npg, t)
        total += len(gs)
    assert total >= 200 and {True, False, "BadArgs"} <= seen


# ---- 4. which preparation a call takes by its shape
def test_route_by_size(kz, torch, settings, fx):
    G = 8192                                                     # many short groups: one cell each, every other one with a foreign proof
    rng = random.Random(4)
    groups, want = [], []
    for g in range(G):
        b, k = rng.randrange(3), rng.randrange(128)
        grp = cases.batch(fx, [(b, k)])
        bad = g % 2 == 1
        if bad:
            grp = (grp[0], grp[1], grp[2], [fx["P"][b][(k + 1) % 128]])
        groups.append(grp)
        want.append(not bad)
    d = to_device(torch, groups)
    before = settings.cell_device_prep_calls
    assert kz.Kzg.verify_cell_kzg_proof_batch_many_device(*d, 1, G, settings) == want
    assert settings.cell_device_prep_calls - before == 1
    row = cases.batch(fx, [(1, k) for k in range(128)])        # a lone group with a 270 KB transcript
    for grp, verdict in ((row, True), ((row[0], row[1], row[2], [row[3][1], row[3][0]] + row[3][2:]), False)):
        d = to_device(torch, [grp])
        before = settings.cell_device_prep_calls
        assert kz.Kzg.verify_cell_kzg_proof_batch_many_device(*d, 128, 1, settings) == [verdict]
        assert settings.cell_device_prep_calls == before


# ---- 5. compute
def host_compute(kz, settings, blobs, cells=True, proofs=True):
    n = len(blobs)
    c = C.create_string_buffer(ROW * n) if cells else None
    p = C.create_string_buffer(48 * 128 * n) if proofs else None
    st = (C.c_int * n)()
    rc = kz.kzg.lib().kzg355_compute_cells_and_kzg_proofs_many(c, p, st, b"".join(blobs), n, settings.handle)
    return rc, list(st), c.raw if cells else None, p.raw if proofs else None


@pytest.mark.parametrize("n", [1, 3, 513])
def test_compute_matches_the_host_form(kz, torch, settings, n):
    blobs = [random_blob(41000 + i) for i in range(n)]
    rc, st, hc, hp = host_compute(kz, settings, blobs)
    assert rc == 0 and st == [0] * n
    d_blobs = u8(torch, b"".join(blobs))
    for cells, proofs in ((True, True), (True, False), (False, True)):
        dc = torch.zeros(ROW * n, dtype=torch.uint8, device="cuda") if cells else None
        dp = torch.zeros(48 * 128 * n, dtype=torch.uint8, device="cuda") if proofs else None
        assert kz.Kzg.compute_cells_and_kzg_proofs_many_device(d_blobs, n, settings, cells_out=dc, proofs_out=dp) == [None] * n
        assert not cells or bytes(dc.cpu().numpy()) == hc
        assert not proofs or bytes(dp.cpu().numpy()) == hp


def test_compute_statuses_and_refusals(kz, torch, settings):
    n = 5
    blobs = [random_blob(42000 + i) for i in range(n)]
    blobs[2] = blobs[2][:32 * 100] + R.to_bytes(32, "big") + blobs[2][32 * 101:]
    rc, st, hc, hp = host_compute(kz, settings, blobs)
    assert rc == kz.BadArgs.code and st == [0, 0, kz.BadArgs.code, 0, 0]
    d_blobs = u8(torch, b"".join(blobs))
    dc = torch.zeros(ROW * n, dtype=torch.uint8, device="cuda")
    dp = torch.zeros(48 * 128 * n, dtype=torch.uint8, device="cuda")
    res = kz.Kzg.compute_cells_and_kzg_proofs_many_device(d_blobs, n, settings, cells_out=dc, proofs_out=dp)
    assert [type(r).__name__ for r in res] == ["NoneType", "NoneType", "BadArgs", "NoneType", "NoneType"]
    gc, gp = bytes(dc.cpu().numpy()), bytes(dp.cpu().numpy())
    for i in (0, 1, 3, 4):                                       # the neighbours are exact
        assert gc[ROW * i:ROW * (i + 1)] == hc[ROW * i:ROW * (i + 1)] and gp[6144 * i:6144 * (i + 1)] == hp[6144 * i:6144 * (i + 1)], i
    lib = kz.kzg.lib()
    st = (C.c_int * n)(*([7] * n))
    assert lib.kzg355_compute_cells_and_kzg_proofs_many_device(None, None, st, d_blobs.data_ptr(), n, settings.handle) == kz.BadArgs.code
    assert list(st) == [kz.BadArgs.code] * n
    for args in ((dc.data_ptr() + 8, dp.data_ptr(), d_blobs.data_ptr()), (dc.data_ptr(), dp.data_ptr() + 4, d_blobs.data_ptr()),
                 (dc.data_ptr(), dp.data_ptr(), d_blobs.data_ptr() + 1)):
        st = (C.c_int * n)(*([7] * n))
        assert lib.kzg355_compute_cells_and_kzg_proofs_many_device(args[0], args[1], st, args[2], n, settings.handle) == kz.BadArgs.code
        assert list(st) == [kz.BadArgs.code] * n
    assert lib.kzg355_compute_cells_and_kzg_proofs_many_device(dc.data_ptr(), None, None, None, 0, settings.handle) == 0


# ---- 6. recover
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("known", [64, 65, 128])
def test_recover_matches_the_host_form(kz, torch, settings, m, known):
    blobs = [random_blob(43000 + i) for i in range(m)]
    _, _, hc, _ = host_compute(kz, settings, blobs, proofs=False)
    ix = sorted(random.Random(known * 10 + m).sample(range(128), known))
    inp = b"".join(hc[ROW * i + CELL * k:ROW * i + CELL * (k + 1)] for i in range(m) for k in ix)
    c, p, st = C.create_string_buffer(ROW * m), C.create_string_buffer(6144 * m), (C.c_int * m)()
    assert kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_many(c, p, st, (C.c_size_t * known)(*ix), inp, known, m, settings.handle) == 0
    d_in = u8(torch, inp)
    for cells, proofs in ((True, True), (True, False), (False, True)):
        dc = torch.zeros(ROW * m, dtype=torch.uint8, device="cuda") if cells else None
        dp = torch.zeros(6144 * m, dtype=torch.uint8, device="cuda") if proofs else None
        assert kz.Kzg.recover_cells_and_kzg_proofs_many_device(ix, d_in, m, settings, cells_out=dc, proofs_out=dp) == [None] * m
        assert not cells or bytes(dc.cpu().numpy()) == c.raw
        assert not proofs or bytes(dp.cpu().numpy()) == p.raw


def test_recover_refusals_match_the_host_form(kz, torch, settings):
    m = 2
    lib = kz.kzg.lib()
    d_in = torch.zeros(CELL * 128 * m, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(ROW * m, dtype=torch.uint8, device="cuda")
    h_in, hc = bytes(CELL * 128 * m), C.create_string_buffer(ROW * m)
    sets = [list(range(63)), list(range(64))[::-1], [0] + list(range(64))[:-1], list(range(63)) + [128], list(range(128)) + [5]]
    for ix in sets:
        n = len(ix)
        idx = (C.c_size_t * n)(*ix)
        sh, sd = (C.c_int * m)(7, 7), (C.c_int * m)(7, 7)
        rh = lib.kzg355_recover_cells_and_kzg_proofs_many(hc, None, sh, idx, h_in, n, m, settings.handle)
        rd = lib.kzg355_recover_cells_and_kzg_proofs_many_device(dc.data_ptr(), None, sd, idx, d_in.data_ptr(), n, m, settings.handle)
        assert (rd, list(sd)) == (rh, list(sh)) == (kz.BadArgs.code, [kz.BadArgs.code] * m), ix[:3]
    idx = (C.c_size_t * 64)(*range(64))
    sd = (C.c_int * m)(7, 7)
    assert lib.kzg355_recover_cells_and_kzg_proofs_many_device(None, None, sd, idx, d_in.data_ptr(), 64, m, settings.handle) == kz.BadArgs.code
    assert list(sd) == [kz.BadArgs.code] * m
    assert lib.kzg355_recover_cells_and_kzg_proofs_many_device(dc.data_ptr(), None, sd, idx, d_in.data_ptr() + 2, 64, m, settings.handle) == kz.BadArgs.code
    assert lib.kzg355_recover_cells_and_kzg_proofs_many_device(dc.data_ptr(), None, None, idx, None, 64, 0, settings.handle) == 0


# ---- 7. compute -> verify -> recover, every cell staying on the card
def test_chained_on_the_card(kz, torch, settings, fx):
    blobs = fx["blobs"] + [random_blob(44000)]
    nb = len(blobs)
    assert nb == 4
    coms = [c.to_bytes() for c in kz.Kzg.blob_to_kzg_commitment_many(blobs, settings)]
    assert coms[:3] == fx["C"]
    d_blobs = u8(torch, b"".join(blobs))
    cells = torch.zeros(nb * 128 * CELL, dtype=torch.uint8, device="cuda")
    proofs = torch.zeros(nb * 128 * 48, dtype=torch.uint8, device="cuda")
    assert kz.Kzg.compute_cells_and_kzg_proofs_many_device(d_blobs, nb, settings, cells_out=cells, proofs_out=proofs) == [None] * nb
    # each blob's row as one group: the commitment repeated 128 times, indices 0..127, its cells and proofs as they lie
    d_c = u8(torch, b"".join(coms)).view(nb, 1, 48).expand(nb, 128, 48).contiguous().view(-1)
    d_i = torch.arange(128, dtype=torch.int64, device="cuda").repeat(nb)
    V = kz.Kzg.verify_cell_kzg_proof_batch_many_device
    assert V(d_c, d_i, cells, proofs, 128, nb, settings) == [True] * nb
    for form in (1, 2):
        assert kz.Kzg.debug_cell_batch_intermediates_device(d_c, d_i, cells, proofs, 128, nb, settings, prep_form=form)[0] == [True] * nb
    flipped = cells.clone()
    flipped[(2 * 128 + 77) * CELL + 31] ^= 1                     # one byte of one resident cell of blob 2
    assert V(d_c, d_i, flipped, proofs, 128, nb, settings) == [True, True, False, True]
    for form in (1, 2):
        assert kz.Kzg.debug_cell_batch_intermediates_device(d_c, d_i, flipped, proofs, 128, nb, settings, prep_form=form)[0] == [True, True, False, True]
    keep = sorted(random.Random(7).sample(range(128), 64))       # drop 64 columns, recover from the rest
    known = cells.view(nb, 128, CELL)[:, torch.tensor(keep, device="cuda"), :].contiguous().view(-1)
    rc_cells, rc_proofs = torch.zeros_like(cells), torch.zeros_like(proofs)
    assert kz.Kzg.recover_cells_and_kzg_proofs_many_device(keep, known, nb, settings, cells_out=rc_cells, proofs_out=rc_proofs) == [None] * nb
    assert bool(torch.equal(rc_cells, cells)) and bool(torch.equal(rc_proofs, proofs))


# ---- 8. the Python wrapper's own checks, and addresses against tensors
def test_wrapper_checks_and_integer_addresses(kz, torch, settings, fx):
    grp = cases.batch(fx, [(0, 3), (1, 70), (2, 11), (0, 3)])
    d = to_device(torch, [grp])
    V = kz.Kzg.verify_cell_kzg_proof_batch_many_device
    assert V(*d, 4, 1, settings) == [True]
    assert V(*[t.data_ptr() for t in d], 4, 1, settings) == [True]
    before = settings.cell_device_prep_calls
    with pytest.raises(kz.BadArgs):
        V(d[0][:-1], d[1], d[2], d[3], 4, 1, settings)                     # a short commitment buffer
    with pytest.raises(kz.BadArgs):
        V(d[0], d[1].to(torch.int32), d[2], d[3], 4, 1, settings)          # indices of the wrong width
    with pytest.raises(kz.BadArgs):
        V(d[0], d[1], d[2].to(torch.int16), d[3], 4, 1, settings)
    with pytest.raises(kz.BadArgs):
        V(d[0], d[1], d[2], d[3], 4, 2, settings)                          # twice the groups the buffers hold
    with pytest.raises(kz.BadArgs):
        kz.Kzg.debug_cell_batch_intermediates_device(*d, 4, 1, settings, prep_form=3)
    blob = u8(torch, random_blob(45000))
    out = torch.zeros(ROW, dtype=torch.uint8, device="cuda")
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells_and_kzg_proofs_many_device(blob, 1, settings)                                    # no output
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells_and_kzg_proofs_many_device(blob, 1, settings, cells_out=out[:-16])
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_cells_and_kzg_proofs_many_device(blob, 2, settings, cells_out=out)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.recover_cells_and_kzg_proofs_many_device(list(range(64)), out[:CELL * 63], 1, settings, cells_out=out)
    assert settings.cell_device_prep_calls == before             # no verify call reached the library
    assert kz.Kzg.compute_cells_and_kzg_proofs_many_device(blob, 1, settings, cells_out=out) == [None]
    again = torch.zeros_like(out)
    assert kz.Kzg.compute_cells_and_kzg_proofs_many_device(blob.data_ptr(), 1, settings, cells_out=again.data_ptr()) == [None]
    assert bool(torch.equal(out, again))
    # the C call's own pointer rules: misaligned device pointers and a prep_form out of range
    G = 1
    ok, st, dbg = (C.c_bool * G)(), (C.c_int * G)(7), C.create_string_buffer(176)
    p = [t.data_ptr() for t in d]
    lib = kz.kzg.lib()
    for k, off in ((0, 8), (1, 4), (2, 1), (3, 2)):
        q = list(p); q[k] += off
        st[0] = 7
        assert lib.kzg355_verify_cell_kzg_proof_batch_many_device(ok, st, *q, 4, G, settings.handle) == kz.BadArgs.code and st[0] == kz.BadArgs.code
    st[0] = 7
    assert lib.kzg355_debug_cell_batch_intermediates_device(dbg, ok, st, *p, 4, G, 3, settings.handle) == kz.BadArgs.code and st[0] == kz.BadArgs.code
    assert lib.kzg355_verify_cell_kzg_proof_batch_many_device(ok, st, None, None, None, None, 0, G, settings.handle) == 0 and ok[0] is True
