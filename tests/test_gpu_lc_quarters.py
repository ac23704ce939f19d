"""-m gpu: the quarters form of the bucket linear combination (k_g1.hip: the subgroup test leaves Q = [|x|]P, every scalar is cut into four 64-bit
quarters on P, Q, -phi P, -phi Q, 6-bit windows) against the golden batch, the CPU oracle and the halves form it stands beside.

Every handle pins the bucket form (lincomb_form = 2: a launch set that validates its points takes the quarters; lincomb_form = 5 keeps the halves), once
with the chain threshold at 1 (k_lc_wsum + k_lc_hchain_quad) and once out of reach (k_lc_horner).  Shapes: n = 8 (the smallest the bucket form takes),
64, and 68 / 69 -- the last n whose lists fit the LDS and the first that takes the global slab (lc_forms.h: the busiest wave holds 7 windows of class 1
and 5 of class 0, 76 n + 28 <= 5200 entries)."""
import ctypes as C
import json
import os

import pytest

from synth import random_blob

pytestmark = pytest.mark.gpu

INF = bytes([0xC0]) + bytes(47)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CHAINS = pytest.mark.parametrize("chain_from", [1, 1 << 24], ids=["wsum+hchain_quad", "horner"])


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def fx64():
    fx = json.load(open(os.path.join(GOLDEN, "batch64.json")))
    blobs = [random_blob(fx["first_index"] + i) for i in range(fx["n"])]
    return fx, blobs, [bytes.fromhex(c) for c in fx["commitments"]], [bytes.fromhex(p) for p in fx["proofs"]]


@pytest.fixture(scope="module")
def fx512():
    """The first 207 blobs of the 512-blob fixture: three batches of up to 69."""
    fx = json.load(open(os.path.join(GOLDEN, "batch512.json")))
    k = 3 * 69
    return [random_blob(fx["first_index"] + i) for i in range(k)], [bytes.fromhex(c) for c in fx["commitments"][:k]], [bytes.fromhex(p) for p in fx["proofs"][:k]]


def _handle(kz, setup_bytes, **opts):
    g1, g2 = setup_bytes
    return kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], **opts)


def _dev(torch, s, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", s.device))


def _want(inter):
    return inter["r"], inter["proof_lincomb"], inter["rhs"], inter["ok"]


def _intermediates(L, s, t_rec, n, groups, want_status=None):
    out = C.create_string_buffer(128 * groups)
    ok = (C.c_bool * groups)(); st = (C.c_int * groups)()
    rc = L.kzg355_debug_batch_intermediates(out, ok, st, t_rec.data_ptr(), n, groups, s.handle)
    assert list(st) == (want_status or [0] * groups), (rc, list(st))
    d = out.raw
    return [(d[128 * g:128 * g + 32], d[128 * g + 32:128 * g + 80], d[128 * g + 80:128 * g + 128], bool(ok[g])) for g in range(groups)]


def _records(L, torch, s, batches, n, want_status=None):
    """Stage 1 of `batches` (lists of (blobs, commitments, proofs)) -> the device tensor of their records."""
    G = len(batches)
    tb = _dev(torch, s, b"".join(b"".join(b) for b, _, _ in batches))
    tc = _dev(torch, s, b"".join(b"".join(c) for _, c, _ in batches))
    tp = _dev(torch, s, b"".join(b"".join(p) for _, _, p in batches))
    rec = torch.zeros(160 * n * G, dtype=torch.uint8, device=tb.device)
    torch.cuda.synchronize()
    st = (C.c_int * G)()
    L.kzg355_verify_shard_records_device(rec.data_ptr(), st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle)
    assert list(st) == (want_status or [0] * G)
    return rec, (tb, tc, tp)


def _special_points(oracle):
    """An x off the curve and an x on the curve whose point lies outside the subgroup."""
    off = sub = None
    for x in range(1, 1000):
        b = bytearray(x.to_bytes(48, "big")); b[0] |= 0x80
        b = bytes(b)
        if off is None and oracle.g1_uncompress_only(b) != 0:
            off = b
        if sub is None and oracle.g1_uncompress_only(b) == 0 and oracle.g1_validate(b) != 0:
            sub = b
        if off and sub:
            return off, sub


@pytest.fixture(scope="module")
def shapes(oracle, oracle_settings, fx64, fx512):
    """n -> (three batches, expected intermediates of each or None where only the halves form is the reference)."""
    fx, blobs, cs, ps = fx64
    golden = (bytes.fromhex(fx["r"]), bytes.fromhex(fx["proof_lincomb"]), bytes.fromhex(fx["rhs"]), fx["expect"])
    rot = lambda v, k: v[k:] + v[:k]
    out = {64: ([(rot(blobs, k), rot(cs, k), rot(ps, k)) for k in (0, 1, 17)], [golden, None, None])}
    b5, c5, p5 = fx512
    for n in (8, 68, 69):
        bt = [(b5[n * j:n * j + n], c5[n * j:n * j + n], p5[n * j:n * j + n]) for j in range(3)]
        out[n] = (bt, [_want(oracle.verify_batch_intermediates(*bt[0], oracle_settings)), None, None])
    return out


@CHAINS
@pytest.mark.parametrize("n", [8, 64, 68, 69])
def test_intermediates_quarters_against_golden_oracle_and_halves(n, chain_from, kz, setup_bytes, shapes):
    import torch
    batches, want = shapes[n]
    L = kz.kzg.lib()
    sq = _handle(kz, setup_bytes, lincomb_form=2, lc_chain_from=chain_from)
    sh = _handle(kz, setup_bytes, lincomb_form=5, lc_chain_from=chain_from)
    try:
        rec, _ = _records(L, torch, sq, batches, n)
        quarters = _intermediates(L, sq, rec, n, 3)
        halves = _intermediates(L, sh, rec, n, 3)
        assert quarters == halves
        assert all(q[3] for q in quarters)
        for g, w in enumerate(want):
            if w is not None:
                assert quarters[g] == w, g
    finally:
        sq.free(); sh.free()


@CHAINS
def test_corner_batches(chain_from, kz, setup_bytes, oracle, oracle_settings, fx64):
    """n = 8: a commitment and a proof at infinity; every record the same with the proof equal to the commitment (equal and opposite points meet
    inside a bucket); a tampered proof.  Intermediates and verdicts as the oracle gives them, and the verdicts of the flagship call."""
    import torch
    _, blobs, cs, ps = fx64
    n = 8
    b, c, p = blobs[:n], cs[:n], ps[:n]
    inf = (b, [INF] + c[1:], p[:3] + [INF] + p[4:])
    same = ([b[0]] * n, [c[0]] * n, [c[0]] * n)
    sw = list(p); sw[2], sw[6] = sw[6], sw[2]
    tampered = (b, c, sw)
    batches = [(b, c, p), inf, same, tampered]
    want = [_want(oracle.verify_batch_intermediates(*bt, oracle_settings)) for bt in batches]
    assert [w[3] for w in want] == [True, False, False, False]
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes, lincomb_form=2, lc_chain_from=chain_from)
    try:
        rec, (tb, tc, tp) = _records(L, torch, s, batches, n)
        assert _intermediates(L, s, rec, n, len(batches)) == want
        G = len(batches)
        ok = (C.c_bool * G)(); st = (C.c_int * G)()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle) == 0
        assert [bool(x) for x in ok] == [w[3] for w in want] and not any(st)
    finally:
        s.free()


@CHAINS
def test_point_outside_the_subgroup_between_good_batches(chain_from, kz, setup_bytes, oracle, fx64):
    import torch
    _, blobs, cs, ps = fx64
    n = 8
    _, sub = _special_points(oracle)
    batches = [(blobs[:n], cs[:n], ps[:n]), (blobs[n:2 * n], cs[n:n + 3] + [sub] + cs[n + 4:2 * n], ps[n:2 * n]), (blobs[2 * n:3 * n], cs[2 * n:3 * n], ps[2 * n:3 * n])]
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes, lincomb_form=2, lc_chain_from=chain_from)
    try:
        rec, (tb, tc, tp) = _records(L, torch, s, batches, n, want_status=[0, 1, 0])
        ok = (C.c_bool * 3)(); st = (C.c_int * 3)()
        rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, 3, s.handle)
        assert rc == 1 and list(st) == [0, 1, 0] and bool(ok[0]) and bool(ok[2])
        # and through the records: the checked call validates again (quarters), the same statuses
        ok2 = (C.c_bool * 3)(); st2 = (C.c_int * 3)()
        rc = L.kzg355_verify_records_checked_device(ok2, st2, rec.data_ptr(), n, 3, s.handle)
        assert rc == 1 and list(st2) == [0, 1, 0] and bool(ok2[0]) and bool(ok2[2])
    finally:
        s.free()


def test_trusted_records_agree_with_the_checked_call(kz, setup_bytes, fx64):
    """kzg355_verify_records_device decodes trusted records without the subgroup test, so it has no Q's and keeps the halves form."""
    import torch
    _, blobs, cs, ps = fx64
    n = 8
    sw = list(ps[n:2 * n]); sw[1], sw[5] = sw[5], sw[1]
    batches = [(blobs[:n], cs[:n], ps[:n]), (blobs[n:2 * n], cs[n:2 * n], sw), (blobs[2 * n:3 * n], cs[2 * n:3 * n], ps[2 * n:3 * n])]
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes, lincomb_form=2, lc_chain_from=1)
    try:
        rec, _ = _records(L, torch, s, batches, n)
        got = []
        for fn in (L.kzg355_verify_records_device, L.kzg355_verify_records_checked_device):
            ok = (C.c_bool * 3)(); st = (C.c_int * 3)()
            assert fn(ok, st, rec.data_ptr(), n, 3, s.handle) == 0 and not any(st)
            got.append([bool(x) for x in ok])
        assert got[0] == got[1] == [True, False, True]
    finally:
        s.free()
