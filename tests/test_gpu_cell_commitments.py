"""-m gpu: the blobs' commitments out of the FK20 chain of the compute and recover calls (slot 63 of the convolution whose
slots 0..62 give the proofs).  Expected commitments come from the CPU oracle, from the reference vectors, from closed forms over the ceremony's
monomial points, or from blob_to_kzg_commitment_many of a bucket-form handle (8-bit MSM, no wide table) -- never from the call under test;
expected cells and proofs from tests/golden/cells.json or from the calls this one extends.  Slot 63 is the only reader of the comb table's
points [tau^4032 .. tau^4095]_1, so the closed forms aim there."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import cell_spec as cs
import fk20_spec as fk
from synth import random_blob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = cs.R
INF = fk.G1_INF
BADARGS = 1
CELL, BLOB, ROW, PROOFS = 2048, 131072, 128 * 2048, 128 * 48
GUARD = 64


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, **options):
    g1, g2 = setup_bytes
    return kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], **options)


@pytest.fixture(scope="module")
def s8(kz, setup_bytes):
    """bucket form: its blob_to_kzg_commitment* builds no wide table"""
    s = _load(kz, setup_bytes, msm_bits=8)
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx(oracle, oracle_settings):
    d = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    d["blobs"] = [random_blob(s) for s in d["blob_seeds"]]
    d["cells"] = [cs.compute_cells(b) for b in d["blobs"]]
    d["P"] = [[bytes.fromhex(p) for p in ps] for ps in d["proofs"]]
    d["K"] = [oracle.blob_to_kzg_commitment(b, oracle_settings) for b in d["blobs"]]
    return d


@pytest.fixture(scope="module")
def mono():
    return cs.load_monomial()


def raw(xs):
    return [bytes(x) for x in xs]


def triple(r):
    return bytes(r[0]), raw(r[1]), raw(r[2])


def blob_of_power(e, c=0):
    """the blob of X^e + c: values at w4096^rev12(i)"""
    w = fk.W4096
    return b"".join(((pow(pow(w, cs.rev(i, 12), R), e, R) + c) % R).to_bytes(32, "big") for i in range(cs.N_FE))


class Guarded:
    """a device byte tensor of n bytes between two runs of guard bytes, 16-byte aligned (or `shift` bytes off)"""
    def __init__(self, n, shift=0):
        import torch
        self.n, self.shift = n, shift
        self.whole = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.whole[GUARD + shift:GUARD + shift + n]
        assert self.t.data_ptr() % 16 == shift % 16

    def bytes(self):
        return bytes(self.t.cpu().numpy())

    def intact(self):
        w = bytes(self.whole.cpu().numpy())
        lo, hi = GUARD + self.shift, GUARD + self.shift + self.n
        return w[:lo] == b"\xa5" * lo and w[hi:] == b"\xa5" * (len(w) - hi)

    def untouched(self):
        return bytes(self.whole.cpu().numpy()) == b"\xa5" * (2 * GUARD + self.n)


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


# ------------------------------------------------------------------------------------------------ 1: the fixture blobs
def test_fixture_blobs_every_form_and_output_combination(kz, s8, fx):
    n = len(fx["blobs"])
    want = [(fx["K"][b], fx["cells"][b], fx["P"][b]) for b in range(n)]
    old_before = [(raw(c), raw(p)) for c, p in kz.Kzg.compute_cells_and_kzg_proofs_many(fx["blobs"], s8)]
    assert old_before == [(w[1], w[2]) for w in want]
    for b in range(n):
        assert triple(kz.Kzg.compute_commitment_cells_and_kzg_proofs(fx["blobs"][b], s8)) == want[b], b
    assert [triple(r) for r in kz.Kzg.compute_commitment_cells_and_kzg_proofs_many(fx["blobs"], s8)] == want
    only = kz.Kzg._compute_commitments_cells(fx["blobs"], s8, True, False, False)
    assert [(bytes(k), c, p) for k, c, p in only] == [(w[0], None, None) for w in want]
    with_cells = kz.Kzg._compute_commitments_cells(fx["blobs"], s8, True, True, False)
    assert [(bytes(k), raw(c), p) for k, c, p in with_cells] == [(w[0], w[1], None) for w in want]
    with_proofs = kz.Kzg._compute_commitments_cells(fx["blobs"], s8, True, False, True)
    assert [(bytes(k), c, raw(p)) for k, c, p in with_proofs] == [(w[0], None, w[2]) for w in want]
    # commitments_out == NULL: the call it extends, byte for byte
    no_k = kz.Kzg._compute_commitments_cells(fx["blobs"], s8, False, True, True)
    assert [(k, raw(c), raw(p)) for k, c, p in no_k] == [(None, w[1], w[2]) for w in want]
    # and the old entry points on the same handle return what they did before
    assert [(raw(c), raw(p)) for c, p in kz.Kzg.compute_cells_and_kzg_proofs_many(fx["blobs"], s8)] == old_before
    assert raw(kz.Kzg.compute_kzg_cell_proofs(fx["blobs"][1], s8)) == fx["P"][1]
    assert raw(kz.Kzg.compute_cells(fx["blobs"][2], s8)) == fx["cells"][2]
    assert kz.Kzg.debug_cell_compute_h([fx["blobs"][0]], s8)[0][63] == INF            # H_63 stays infinity


def test_all_outputs_null_is_badargs_with_a_real_handle(kz, s8, fx):
    lib = kz.kzg.lib()
    blob = fx["blobs"][0]
    idx = (C.c_size_t * 64)(*range(64))
    counts = (C.c_size_t * 2)(64, 64)
    idx2 = (C.c_size_t * 128)(*(list(range(64)) * 2))
    known = b"".join(fx["cells"][0][:64]) * 2
    for call in (lambda st: lib.kzg355_compute_commitments_cells_and_kzg_proofs_many(None, None, None, st, blob + blob, 2, s8.handle),
                 lambda st: lib.kzg355_recover_commitments_cells_and_kzg_proofs_many(None, None, None, st, idx, known, 64, 2, s8.handle),
                 lambda st: lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(None, None, None, st, counts, idx2, known, 2, s8.handle)):
        st = (C.c_int * 2)(7, 7)
        assert call(st) == BADARGS and list(st) == [BADARGS, BADARGS]
    k = C.create_string_buffer(96)
    assert lib.kzg355_compute_commitments_cells_and_kzg_proofs_many(k, None, None, None, b"", 0, s8.handle) == 0      # n == 0


# ------------------------------------------------------------------------------------------------ 2: the reference vectors
def test_reference_vectors_in_one_call(kz, s8, golden_vectors, golden_blobs):
    cases = golden_vectors["blob_to_kzg_commitment"]
    sized = [c for c in cases if len(golden_blobs[c["input"]["blob"]["blob"]]) == BLOB]
    good, bad = [c for c in sized if c["output"]], [c for c in sized if not c["output"]]
    assert len(good) == 6 and len(bad) == 2
    order = good[:1] + bad[:1] + good[1:3] + bad[1:] + good[3:]                          # each invalid blob between valid neighbours
    res = kz.Kzg.compute_commitment_cells_and_kzg_proofs_many([golden_blobs[c["input"]["blob"]["blob"]] for c in order], s8)
    for c, r in zip(order, res):
        if c["output"]:
            assert bytes(r[0]).hex() == c["output"][2:], c["name"]
            assert raw(r[1])[:64] == [golden_blobs[c["input"]["blob"]["blob"]][CELL * k:CELL * (k + 1)] for k in range(64)]
        else:
            assert isinstance(r, kz.BadArgs), c["name"]
    for c in cases:                                                                      # the two of another length never reach the call
        b = golden_blobs[c["input"]["blob"]["blob"]]
        if len(b) != BLOB:
            assert not c["output"]
            with pytest.raises(kz.InvalidBytesLength):
                kz.Kzg.compute_commitment_cells_and_kzg_proofs(b, s8)


# ------------------------------------------------------------------------------------------------ 3: closed forms
def test_closed_forms(kz, s8, oracle, oracle_settings, mono):
    rng = random.Random(4032)
    const = rng.randrange(R)
    high = [0] * (cs.N_FE - cs.CELL_FE) + [rng.randrange(1, R) for _ in range(cs.CELL_FE)]
    powers = [0, 63, 64, 4032, 4095]
    blobs = [bytes(BLOB)] + [blob_of_power(t) for t in powers] + [const.to_bytes(32, "big") * cs.N_FE, fk.blob_from_coefficients(high)]
    want = [INF] + [mono[t] for t in powers] + [cs.lincomb(oracle, [mono[0]], [const]), cs.lincomb(oracle, mono[cs.N_FE - cs.CELL_FE:], high[-cs.CELL_FE:])]
    assert mono[0].hex().startswith("97f1d3a7")                                          # [tau^0]_1 = G1
    res = kz.Kzg.compute_commitment_cells_and_kzg_proofs_many(blobs, s8)
    assert [bytes(r[0]) for r in res] == want
    only = kz.Kzg._compute_commitments_cells(blobs, s8, True, False, False)
    assert [bytes(r[0]) for r in only] == want
    assert raw(res[0][2]) == [INF] * 128                                                 # the zero blob's proofs, as before
    assert want[-1] == oracle.blob_to_kzg_commitment(blobs[-1], oracle_settings) and want[-2] == oracle.blob_to_kzg_commitment(blobs[-2], oracle_settings)


# ------------------------------------------------------------------------------------------------ 4: a fresh handle
def test_first_call_of_a_fresh_handle_wants_commitments_only(kz, setup_bytes, fx, oracle, oracle_settings):
    s = _load(kz, setup_bytes, msm_bits=8)
    try:
        only = kz.Kzg._compute_commitments_cells(fx["blobs"][:2], s, True, False, False)
        assert [bytes(r[0]) for r in only] == fx["K"][:2]
        assert triple(kz.Kzg.compute_commitment_cells_and_kzg_proofs(fx["blobs"][2], s)) == (fx["K"][2], fx["cells"][2], fx["P"][2])
        # the 4844 path of the same handle is untouched
        blob = random_blob(31337)
        com = kz.Kzg.blob_to_kzg_commitment(blob, s)
        assert bytes(com) == oracle.blob_to_kzg_commitment(blob, oracle_settings)
        pr = kz.Kzg.compute_blob_kzg_proof(blob, com, s)
        assert bytes(pr) == oracle.compute_blob_kzg_proof(blob, bytes(com), oracle_settings)
        assert kz.Kzg.verify_blob_kzg_proof(blob, com, pr, s) is True
    finally:
        s.free()


# ------------------------------------------------------------------------------------------------ 5: the chunk border, resident
def test_513_resident_blobs_commitments_and_proofs(kz, s8):
    n = 513                                                                              # chunks of 512: the last chunk is one blob
    distinct = [random_blob(51300 + i) for i in range(7)]
    pick = [i % 4 for i in range(n)]
    pick[0], pick[511], pick[512] = 4, 5, 6
    d_blobs = on_device(b"".join(distinct[p] for p in pick))
    k_out, p_out = Guarded(48 * n), Guarded(PROOFS * n)
    res = kz.Kzg.compute_commitment_cells_and_kzg_proofs_many_device(d_blobs, n, s8, commitments_out=k_out.t, proofs_out=p_out.t)
    assert res == [None] * n
    assert k_out.intact() and p_out.intact()
    coms = kz.Kzg.blob_to_kzg_commitment_many(distinct, s8)
    got = k_out.bytes()
    assert [got[48 * i:48 * i + 48] for i in range(n)] == [bytes(coms[p]) for p in pick]
    proofs = p_out.bytes()
    for i in (0, 511, 512):
        assert proofs[PROOFS * i:PROOFS * (i + 1)] == b"".join(raw(kz.Kzg.compute_kzg_cell_proofs(distinct[pick[i]], s8))), i
    assert proofs[PROOFS * 1:PROOFS * 2] == proofs[PROOFS * 5:PROOFS * 6] != proofs[PROOFS * 2:PROOFS * 3]


# ------------------------------------------------------------------------------------------------ 6: recovery
def test_recover_shared_sets(kz, s8, fx):
    n = len(fx["blobs"])
    for ix in (list(range(0, 128, 2)), [k for k in range(128) if k != 77]):
        assert len(ix) in (64, 127)
        rows = [[fx["cells"][b][k] for k in ix] for b in range(n)]
        old = kz.Kzg.recover_cells_and_kzg_proofs_many(ix, rows, s8)
        res = kz.Kzg.recover_commitment_cells_and_kzg_proofs_many(ix, rows, s8)
        assert [triple(r) for r in res] == [(fx["K"][b], raw(old[b][0]), raw(old[b][1])) for b in range(n)]
        assert [(raw(c), raw(p)) for c, p in old] == [(fx["cells"][b], fx["P"][b]) for b in range(n)]
        assert triple(kz.Kzg.recover_commitment_cells_and_kzg_proofs(ix, rows[1], s8)) == (fx["K"][1], fx["cells"][1], fx["P"][1])
        only = kz.Kzg._recover_commitments(ix, rows, s8, True, False, False)              # commitments-only recovery
        assert [(bytes(k), c, p) for k, c, p in only] == [(fx["K"][b], None, None) for b in range(n)]


def test_recover_many_sets_with_a_refused_unit_in_the_middle(kz, s8, fx):
    sets = [list(range(64, 128)), list(range(0, 128, 2)), list(range(63)), sorted(random.Random(6).sample(range(128), 90))]
    owner = [0, 1, 2, 2]
    units = [(ix, [fx["cells"][b][k] for k in ix]) for ix, b in zip(sets, owner)]
    res = kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_sets(units, s8)
    old = kz.Kzg.recover_cells_and_kzg_proofs_many_sets(units, s8)
    assert isinstance(res[2], kz.BadArgs) and isinstance(old[2], kz.BadArgs)
    for u in (0, 1, 3):
        b = owner[u]
        assert triple(res[u]) == (fx["K"][b], fx["cells"][b], fx["P"][b]), u
        assert (raw(old[u][0]), raw(old[u][1])) == (fx["cells"][b], fx["P"][b]), u
    only = kz.Kzg._recover_commitments_sets(units, s8, True, False, False)
    assert isinstance(only[2], kz.BadArgs) and [bytes(only[u][0]) for u in (0, 1, 3)] == [fx["K"][owner[u]] for u in (0, 1, 3)]
    lib = kz.kzg.lib()
    st = (C.c_int * 4)(7, 7, 7, 7)
    counts = (C.c_size_t * 4)(*[len(ix) for ix in sets])
    idx = (C.c_size_t * sum(len(ix) for ix in sets))(*[i for ix in sets for i in ix])
    k = C.create_string_buffer(48 * 4)
    rc = lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(k, None, None, st, counts, idx, b"".join(b"".join(row) for _, row in units), 4, s8.handle)
    assert rc == BADARGS and list(st) == [0, 0, BADARGS, 0]


def test_recover_from_inconsistent_cells_commits_to_what_it_keeps(kz, s8, fx, oracle, oracle_settings):
    ix = list(range(30, 110))                                                            # 80 cells, one of them tampered
    cells = [fx["cells"][0][k] for k in ix]
    t = bytearray(cells[41]); t[32 * 17 + 31] ^= 1
    cells[41] = bytes(t)
    k, c, p = triple(kz.Kzg.recover_commitment_cells_and_kzg_proofs(ix, cells, s8))
    old_c, old_p = kz.Kzg.recover_cells_and_kzg_proofs(ix, cells, s8)
    assert (c, p) == (raw(old_c), raw(old_p))
    assert k == oracle.blob_to_kzg_commitment(b"".join(c[:64]), oracle_settings)
    assert k != fx["K"][0]                                                               # the comparison that shows the tampering up


# ------------------------------------------------------------------------------------------------ 7: recovery, resident
def test_recover_device_forms_between_guards(kz, s8, fx):
    n = len(fx["blobs"])
    ix = list(range(0, 128, 2))
    d_cells = on_device(b"".join(fx["cells"][b][k] for b in range(n) for k in ix))
    k_out, c_out, p_out = Guarded(48 * n), Guarded(ROW * n), Guarded(PROOFS * n)
    res = kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_device(ix, d_cells, n, s8, commitments_out=k_out.t, cells_out=c_out.t, proofs_out=p_out.t)
    assert res == [None] * n and k_out.intact() and c_out.intact() and p_out.intact()
    assert k_out.bytes() == b"".join(fx["K"])
    assert c_out.bytes() == b"".join(b"".join(fx["cells"][b]) for b in range(n))
    assert p_out.bytes() == b"".join(b"".join(fx["P"][b]) for b in range(n))
    k_only = Guarded(48 * n)
    assert kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_device(ix, d_cells, n, s8, commitments_out=k_only.t) == [None] * n
    assert k_only.intact() and k_only.bytes() == b"".join(fx["K"])
    # the sets form: three sets, and a unit of 63 cells in the middle
    sets = [list(range(64, 128)), list(range(63)), [k for k in range(128) if k % 3], list(range(0, 128, 2))]
    owner = [2, 0, 1, 0]
    d_cells = on_device(b"".join(fx["cells"][b][k] for ix_, b in zip(sets, owner) for k in ix_))
    counts, flat = [len(s) for s in sets], [i for s in sets for i in s]
    k_out, c_out, p_out = Guarded(48 * 4), Guarded(ROW * 4), Guarded(PROOFS * 4)
    res = kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_sets_device(counts, flat, d_cells, s8, commitments_out=k_out.t, cells_out=c_out.t,
                                                                          proofs_out=p_out.t)
    assert [type(r).__name__ for r in res] == ["NoneType", "BadArgs", "NoneType", "NoneType"]
    assert k_out.intact() and c_out.intact() and p_out.intact()
    kb, cb, pb = k_out.bytes(), c_out.bytes(), p_out.bytes()
    for u in (0, 2, 3):
        b = owner[u]
        assert kb[48 * u:48 * (u + 1)] == fx["K"][b], u
        assert cb[ROW * u:ROW * (u + 1)] == b"".join(fx["cells"][b]), u
        assert pb[PROOFS * u:PROOFS * (u + 1)] == b"".join(fx["P"][b]), u
    # a commitments pointer off a 16-byte boundary refuses the call as a whole, and nothing is written
    lib = kz.kzg.lib()
    off, c2, p2 = Guarded(48 * 4, shift=8), Guarded(ROW * 4), Guarded(PROOFS * 4)
    cnt = (C.c_size_t * 4)(*counts)
    idx = (C.c_size_t * len(flat))(*flat)
    st = (C.c_int * 4)(7, 7, 7, 7)
    rc = lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(off.t.data_ptr(), c2.t.data_ptr(), p2.t.data_ptr(), st, cnt, idx,
                                                                              d_cells.data_ptr(), 4, s8.handle)
    assert rc == BADARGS and list(st) == [BADARGS] * 4
    shared = (C.c_size_t * 64)(*range(0, 128, 2))
    st3 = (C.c_int * 3)(7, 7, 7)
    rc = lib.kzg355_recover_commitments_cells_and_kzg_proofs_many_device(off.t.data_ptr(), c2.t.data_ptr(), p2.t.data_ptr(), st3, shared,
                                                                         d_cells.data_ptr(), 64, 3, s8.handle)
    assert rc == BADARGS and list(st3) == [BADARGS] * 3
    st3 = (C.c_int * 3)(7, 7, 7)
    rc = lib.kzg355_compute_commitments_cells_and_kzg_proofs_many_device(off.t.data_ptr(), c2.t.data_ptr(), p2.t.data_ptr(), st3, d_cells.data_ptr(), 3,
                                                                         s8.handle)
    assert rc == BADARGS and list(st3) == [BADARGS] * 3
    import torch
    torch.cuda.synchronize()
    assert off.untouched() and c2.untouched() and p2.untouched()


# ------------------------------------------------------------------------------------------------ 8: a handle over several replicas
def _load_replicas(kz, setup_bytes, devices):
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer")                               # no wide table per replica
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], devices=devices)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def test_handle_over_two_replicas(kz, setup_bytes, s8, fx):
    s2 = _load_replicas(kz, setup_bytes, [0, 0])
    try:
        assert s2.device_count == 2
        blobs = [fx["blobs"][i % 3] for i in range(4)] + [random_blob(808)]
        before = s2.cell_calls_per_device()
        got = [triple(r) for r in kz.Kzg.compute_commitment_cells_and_kzg_proofs_many(blobs, s2)]
        spread = [a - b for a, b in zip(s2.cell_calls_per_device(), before)]
        assert spread == [1, 1]
        one = [triple(r) for r in kz.Kzg.compute_commitment_cells_and_kzg_proofs_many(blobs, s8)]
        assert got == one
        assert [g[0] for g in got[:4]] == [fx["K"][i % 3] for i in range(4)]
        sets = [list(range(64, 128)), list(range(0, 128, 2)), list(range(1, 128, 2)), [k for k in range(128) if k != 5], list(range(64))]
        cells = [raw(g[1]) for g in got]
        units = [(ix, [cells[u][k] for k in ix]) for u, ix in enumerate(sets)]
        before = s2.cell_calls_per_device()
        rec = [triple(r) for r in kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_sets(units, s2)]
        assert [a - b for a, b in zip(s2.cell_calls_per_device(), before)] == [1, 1]
        assert rec == got
        assert [triple(r) for r in kz.Kzg.recover_commitment_cells_and_kzg_proofs_many_sets(units, s8)] == got
    finally:
        s2.free()


# ------------------------------------------------------------------------------------------------ 9: the C++ mirror
def test_cpp_mirror_gives_the_same_bytes(kz, s8, fx, tmp_path):
    src, exe = tmp_path / "consumer.cpp", tmp_path / "consumer"
    src.write_text('#include <fstream>\n#include <iostream>\n#include <iterator>\n#include "kzg355.hpp"\n'
                   "using namespace kzg355;\n"
                   "static std::vector<uint8_t> slurp(const char *path) {\n"
                   "    std::ifstream f(path, std::ios::binary);\n"
                   "    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());\n}\n"
                   "static void put(std::ofstream &out, const Kzg::CommitmentCellsProofs &r) {\n"
                   "    out.write(reinterpret_cast<const char *>(r.commitment.data()), 48);\n"
                   "    for (const Cell &c : r.cells) out.write(reinterpret_cast<const char *>(c.data()), KZG355_BYTES_PER_CELL);\n"
                   "    for (const KzgProof &p : r.proofs) out.write(reinterpret_cast<const char *>(p.data()), 48);\n}\n"
                   "int main(int, char **argv) {\n"
                   "    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), in = slurp(argv[3]);\n"
                   "    std::vector<std::vector<uint8_t>> g1v, g2v;\n"
                   "    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);\n"
                   "    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);\n"
                   "    auto rs = Kzg::load_trusted_setup(g1v, g2v);\n"
                   "    if (rs.is_err()) return 1;\n"
                   "    KzgSettings s = rs.value();\n"
                   "    std::ofstream out(argv[4], std::ios::binary);\n"
                   "    auto a = Kzg::compute_commitment_cells_and_kzg_proofs(Blob::from_bytes(in.data(), KZG355_BYTES_PER_BLOB).value(), s);\n"
                   "    if (a.is_err()) return 3;\n"
                   "    put(out, a.value());\n"
                   "    std::vector<size_t> ix;\n"
                   "    std::vector<Cell> known;\n"
                   "    for (size_t k = 0; k < 128; k += 2) { ix.push_back(k); known.push_back(a.value().cells[k]); }\n"
                   "    auto b = Kzg::recover_commitment_cells_and_kzg_proofs(ix, known, s);\n"
                   "    if (b.is_err()) return 4;\n"
                   "    put(out, b.value());\n"
                   "    auto c = Kzg::recover_commitment_cells_and_kzg_proofs_many_sets({Kzg::RecoverUnit{ix, known}}, s);\n"
                   "    if (c.is_err() || c.value()[0].is_err()) return 5;\n"
                   "    put(out, c.value()[0].value());\n"
                   "    return 0;\n}\n")
    so_dir = os.path.join(ROOT, "kzg_rust_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + so_dir, "-lkzg355",
                    "-Wl,-rpath," + so_dir], check=True)
    inp, outp = str(tmp_path / "blob.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(fx["blobs"][1])
    r = subprocess.run([str(exe), os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), inp, outp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    k, c, p = triple(kz.Kzg.compute_commitment_cells_and_kzg_proofs(fx["blobs"][1], s8))
    assert (k, c, p) == (fx["K"][1], fx["cells"][1], fx["P"][1])
    assert open(outp, "rb").read() == (k + b"".join(c) + b"".join(p)) * 3
