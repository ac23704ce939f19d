"""-m gpu: the kernels that run the lazy G1 chain arithmetic of g1.h (g1_dbl_lazy without C = B^2, the additions with Y3 under one reduction),
at the smallest shapes that reach them, against the CPU oracle:

  * k_validate_points (decompression + the two [|x|] ladders of 63 lazy doublings): one 64-blob batch of tests/golden/batch64.json and copies of it
    with ONE commitment or proof replaced by an encoding outside the subgroup, off the curve, or the point at infinity.  Verdicts and per-batch
    statuses as the oracle gives them, through the bench's entry point on a handle pinned to the bucket form (by size these few batches would take
    the pre-shifted form, which validates with other kernels) and through stage 1 alone; the decoded points are compared through what they feed --
    proof_lincomb and rhs, byte for byte (the ABI has no readback of the points themselves).
  * the tail of the bucket form: 64 batches of 8 blobs with the handle's chain threshold at 1 (k_lc_wsum: g1x_add_lazy2; k_lc_hchain_quad) and lifted
    out of reach (k_lc_horner: g1_dbl_lazy + g1_add_lazy): r, proof_lincomb and rhs byte for byte, one disturbed batch found at its position.
  * the reject branches of the latency forms of the validation, on one valid commitment and five spoiled encodings of it: lone compute_blob_kzg_proof
    calls (k_decompress_points; k_subgroup_ladder_from_x_quad + k_subgroup_finish) and lone verify_kzg_proof calls (entry_points.hip: the record's two
    points go through enqueue_points_beside -- k_decompress_points, then k_subgroup_points_quad since there are few points): statuses, and proofs /
    verdicts where there is no error, as the oracle gives them.  The same six checks in ONE verify_kzg_proof_many call take the other route
    (verify_records_impl with validate = 1: the fused k_validate_points on the fields of the records) and must give the same answers."""
import ctypes as C
import json
import os

import pytest

from synth import random_blob

pytestmark = pytest.mark.gpu

INF = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def fx64():
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "batch64.json")))
    blobs = [random_blob(fx["first_index"] + i) for i in range(fx["n"])]
    return blobs, [bytes.fromhex(c) for c in fx["commitments"]], [bytes.fromhex(p) for p in fx["proofs"]]


def _handle(kz, setup_bytes, **opts):
    g1, g2 = setup_bytes
    return kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], **opts)


def _dev(torch, s, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", s.device))


def _special_points(oracle):
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


def _oracle_batch(oracle, oracle_settings, blobs, cs, ps):
    """(status, (r, proof_lincomb, rhs, verdict) or None) of one batch by the oracle."""
    from oracle.oracle import OracleError
    try:
        return 0, _want(oracle.verify_batch_intermediates(blobs, cs, ps, oracle_settings))
    except OracleError as e:
        return e.code, None


def _intermediates(L, s, t_rec, n, groups):
    out = C.create_string_buffer(128 * groups)
    ok = (C.c_bool * groups)(); st = (C.c_int * groups)()
    rc = L.kzg355_debug_batch_intermediates(out, ok, st, t_rec.data_ptr(), n, groups, s.handle)
    assert rc == 0 and not any(st), (rc, list(st))
    d = out.raw
    return [(d[128 * g:128 * g + 32], d[128 * g + 32:128 * g + 80], d[128 * g + 80:128 * g + 128], bool(ok[g])) for g in range(groups)]


def _want(inter):
    return inter["r"], inter["proof_lincomb"], inter["rhs"], inter["ok"]


def test_validate_points_on_a_batch_and_its_spoiled_copies(kz, setup_bytes, oracle, oracle_settings, fx64):
    import torch
    blobs, cs, ps = fx64
    n = len(blobs)
    off, sub = _special_points(oracle)
    sub_neg = bytes([sub[0] ^ 0x20]) + sub[1:]                     # the other sign of y: the same x, still outside the subgroup
    batches = [(list(cs), list(ps)) for _ in range(6)]
    batches[1][0][5] = sub                                         # commitment outside the subgroup
    batches[2][1][63] = off                                        # proof off the curve
    batches[3][0][0] = INF                                         # infinity is a valid point (utils.rs:298-301): verdict false, no error
    batches[4][1][63] = INF
    batches[5][1][9] = sub_neg
    G = len(batches)
    want = [_oracle_batch(oracle, oracle_settings, blobs, c, p) for c, p in batches]
    assert [w[0] for w in want] == [0, 1, 1, 0, 0, 1] and [w[1][3] for w in want if w[0] == 0] == [True, False, False]      # (the cases are what they claim)
    L = kz.kzg.lib()
    # lincomb_form = 2 pins the bucket form.  By size, 6 batches of 64 would take the pre-shifted form, whose stage 1 decodes with k_decompress_points and
    # tests the subgroup with the DPP-quad ladder (verify_stages.hip: enqueue_points_beside) -- k_validate_points would never see the spoiled points.
    s = _handle(kz, setup_bytes, lincomb_form=2)
    try:
        tb = _dev(torch, s, b"".join(blobs) * G)
        tc = _dev(torch, s, b"".join(b"".join(c) for c, _ in batches))
        tp = _dev(torch, s, b"".join(b"".join(p) for _, p in batches))
        torch.cuda.synchronize()
        # 1. the entry point the benchmark times, all six batches: k_validate_points on every point, verdicts and statuses
        ok = (C.c_bool * G)(); st = (C.c_int * G)()
        rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle)
        print("many_device: rc", rc, "status", list(st), "ok", [bool(x) for x in ok], "oracle status", [w[0] for w in want])
        assert rc == 1
        assert [st[g] for g in range(G)] == [w[0] for w in want]
        assert [bool(ok[g]) for g in range(G) if want[g][0] == 0] == [w[1][3] for w in want if w[0] == 0]
        # 2. stage 1 alone on all six (never pre-shifted: k_validate_points again, on the packed inputs): the same status vector
        rec = torch.zeros(160 * n * G, dtype=torch.uint8, device=tb.device)
        torch.cuda.synchronize()
        st1 = (C.c_int * G)()
        rc = L.kzg355_verify_shard_records_device(rec.data_ptr(), st1, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle)
        print("shard_records: rc", rc, "status", list(st1))
        assert rc == 1 and [st1[g] for g in range(G)] == [w[0] for w in want]
        # 3. the decoded points, through the sums they enter: the records of the batches without an error go through stage 2, which runs
        #    k_validate_points once more on the points inside the records; r | proof_lincomb | rhs byte for byte
        good = [g for g in range(G) if want[g][0] == 0]
        good_rec = torch.cat([rec[160 * n * g:160 * n * (g + 1)] for g in good]).contiguous()
        torch.cuda.synchronize()
        got = _intermediates(L, s, good_rec, n, len(good))
        for g, have in zip(good, got):
            assert have == want[g][1], g
    finally:
        s.free()


@pytest.fixture(scope="module")
def small_batches(oracle, oracle_settings, fx64):
    """Eight different 8-blob batches cut from the 64-blob fixture and the oracle's intermediates of each, plus batch 3 with two proofs swapped."""
    blobs, cs, ps = fx64
    cut = [(blobs[8 * j:8 * j + 8], cs[8 * j:8 * j + 8], ps[8 * j:8 * j + 8]) for j in range(8)]
    want = [_want(oracle.verify_batch_intermediates(b, c, p, oracle_settings)) for b, c, p in cut]
    b, c, p = cut[3]
    sw = list(p); sw[2], sw[6] = sw[6], sw[2]
    want_sw = _want(oracle.verify_batch_intermediates(b, c, sw, oracle_settings))
    assert all(w[3] for w in want) and not want_sw[3]
    return cut, want, sw, want_sw


@pytest.mark.parametrize("chain_from", [1, 1 << 24], ids=["wsum+hchain_quad", "horner"])
def test_bucket_tail_on_64_batches_of_8(chain_from, kz, setup_bytes, small_batches):
    import torch
    cut, want, sw, want_sw = small_batches
    n, G, bad = 8, 64, 37                                          # batch g is cut[g % 8]; batch 37 (cut[5]) is replaced by the disturbed cut[3]
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes, lincomb_form=2, lc_chain_from=chain_from)
    try:
        order = [g % 8 for g in range(G)]
        order[bad] = 3
        tb = _dev(torch, s, b"".join(b"".join(cut[j][0]) for j in order))
        tc = _dev(torch, s, b"".join(b"".join(cut[j][1]) for j in order))
        tp = _dev(torch, s, b"".join(b"".join(sw if g == bad else cut[j][2]) for g, j in enumerate(order)))
        rec = torch.zeros(160 * n * G, dtype=torch.uint8, device=tb.device)
        torch.cuda.synchronize()
        st1 = (C.c_int * G)()
        assert L.kzg355_verify_shard_records_device(rec.data_ptr(), st1, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle) == 0 and not any(st1)
        got = _intermediates(L, s, rec, n, G)
        expect = [want_sw if g == bad else want[j] for g, j in enumerate(order)]
        assert [g for g in range(G) if got[g] != expect[g]] == []
        assert [g for g in range(G) if not got[g][3]] == [bad]
        # and the entry point the benchmark times: verdicts only
        ok = (C.c_bool * G)(); st = (C.c_int * G)()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle) == 0
        assert [g for g in range(G) if not ok[g]] == [bad] and not any(st)
    finally:
        s.free()


FP_MODULUS = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


@pytest.fixture(scope="module")
def six_encodings(oracle, fx64):
    """The fixture's first commitment and five spoiled encodings: infinity (valid), on the curve but outside the subgroup, x not on the curve, x >= p,
    no compression bit."""
    c = fx64[1][0]
    off, sub = _special_points(oracle)
    x_ge_p = bytearray(FP_MODULUS.to_bytes(48, "big")); x_ge_p[0] |= 0x80
    enc = [c, INF, sub, off, bytes(x_ge_p), bytes([c[0] & 0x7F]) + c[1:]]
    assert [oracle.g1_uncompress_only(e) == 0 for e in enc] == [True, True, True, False, False, False]      # (the cases are what they claim)
    assert [oracle.g1_validate(e) == 0 for e in enc] == [True, True, False, False, False, False]
    return enc


def test_lone_compute_blob_kzg_proof_on_spoiled_commitments(kz, setup_bytes, oracle, oracle_settings, fx64, six_encodings):
    from oracle.oracle import OracleError
    blob = fx64[0][0]
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes)
    try:
        got, want = [], []
        for c in six_encodings:
            out = C.create_string_buffer(48)
            rc = L.kzg355_compute_blob_kzg_proof(out, blob, c, s.handle)
            got.append((rc, out.raw if rc == 0 else None))
            try:
                want.append((0, oracle.compute_blob_kzg_proof(blob, c, oracle_settings)))
            except OracleError as e:
                want.append((e.code, None))
        print("compute_blob_kzg_proof: status", [g[0] for g in got], "oracle status", [w[0] for w in want])
        assert [w[0] for w in want] == [0, 0, 1, 1, 1, 1] and want[0][1] == fx64[2][0]
        assert got == want
    finally:
        s.free()


def test_verify_kzg_proof_lone_and_many_on_spoiled_commitments(kz, setup_bytes, oracle, oracle_settings, fx64, six_encodings):
    from oracle.oracle import OracleError
    blob = fx64[0][0]
    z = (0x1234567).to_bytes(32, "big")
    proof, y = oracle.compute_kzg_proof(blob, z, oracle_settings)
    want = []
    for c in six_encodings:
        try:
            want.append((0, oracle.verify_kzg_proof(c, z, y, proof, oracle_settings)))
        except OracleError as e:
            want.append((e.code, None))
    assert want == [(0, True), (0, False), (1, None), (1, None), (1, None), (1, None)]
    n = len(six_encodings)
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes)
    try:
        # lone calls: k_decompress_points + k_subgroup_points_quad
        lone = []
        for c in six_encodings:
            one = C.c_bool()
            rc = L.kzg355_verify_kzg_proof(C.byref(one), c, z, y, proof, s.handle)
            lone.append((rc, bool(one.value) if rc == 0 else None))
        print("verify_kzg_proof: (status, ok)", lone, "oracle", want)
        assert lone == want
        # one call of six: k_validate_points on the records
        ok = (C.c_bool * n)(); st = (C.c_int * n)()
        rc = L.kzg355_verify_kzg_proof_many(ok, st, b"".join(six_encodings), z * n, y * n, proof * n, n, s.handle)
        print("verify_kzg_proof_many: rc", rc, "status", list(st), "ok", [bool(x) for x in ok], "oracle", want)
        assert rc == 1
        assert [(st[i], bool(ok[i]) if st[i] == 0 else None) for i in range(n)] == want
    finally:
        s.free()
