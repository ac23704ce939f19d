"""-m gpu: the kernels that were built and measured with the column forms of field.h's lazy Montgomery products (the wrappers of its column body
mont_cols; the row forms are those of the bodies mont_mul and mont_sqr) -- k_eval (k_verify.hip: KZG_MONT_COLS_FR) and the bucket kernel (k_g1.hip:
g1x_add_mixed_lazy<true>) keep them, the point validation and the tails of the bucket form went back to the row forms (EXPERIMENTS.md) -- at the
smallest shapes that reach them, byte for byte against the CPU oracle:

  * k_eval: one batch of 4 blobs (one workgroup) and one of 5 (a second workgroup whose spare waves repeat the last blob): an all-zero blob, a blob of
    r - 1 throughout, random blobs -- z and y of the records as the oracle computes them -- and the same batches with ONE field element replaced by
    r (not canonical): the status the oracle gives.
  * k_validate_points: the 64-blob batch of tests/golden/batch64.json and six copies with one commitment or one proof replaced by an encoding off
    the curve, outside the subgroup, or the point at infinity: statuses and verdicts, and r | proof_lincomb | rhs of the batches without an error.
  * the bucket form and its tails: 64 batches of 8 blobs with the chain threshold at 1 (k_lc_wsum + k_lc_hchain_quad) and out of reach (k_lc_horner)."""
import ctypes as C

import pytest

from synth import random_blob
from test_gpu_lazy_chain import INF, _dev, _handle, _intermediates, _oracle_batch, _special_points, fx64, kz, small_batches  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


@pytest.fixture(scope="module")
def eval_blobs(oracle, oracle_settings):
    """Five canonical blobs with their commitments (the oracle's), and the same with element 1234 of blob 2 set to r."""
    blobs = [bytes(131072), (R_ORDER - 1).to_bytes(32, "big") * 4096] + [random_blob(7700 + i) for i in range(3)]
    cs = [oracle.blob_to_kzg_commitment(b, oracle_settings) for b in blobs]
    spoiled = list(blobs)
    spoiled[2] = blobs[2][:32 * 1234] + R_ORDER.to_bytes(32, "big") + blobs[2][32 * 1235:]
    return blobs, cs, spoiled


@pytest.mark.parametrize("n", [4, 5])
def test_eval_on_one_workgroup_and_on_a_tail_wave(n, kz, setup_bytes, oracle, oracle_settings, eval_blobs):
    import torch
    from oracle.oracle import OracleError
    blobs, cs, spoiled = (x[:n] for x in eval_blobs)
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes)
    try:
        tc = _dev(torch, s, b"".join(cs))
        for data, canonical in ((blobs, True), (spoiled, False)):
            tb = _dev(torch, s, b"".join(data))
            rec = torch.zeros(160 * n, dtype=torch.uint8, device=tb.device)
            torch.cuda.synchronize()
            st = (C.c_int * 1)(-1)
            rc = L.kzg355_verify_shard_records_device(rec.data_ptr(), st, tb.data_ptr(), tc.data_ptr(), tc.data_ptr(), n, 1, s.handle)
            if canonical:
                assert rc == 0 and st[0] == 0
                got = bytes(rec.cpu().numpy())
                for i in range(n):
                    z = oracle.compute_challenge(data[i], cs[i])
                    assert got[160 * i + 48:160 * i + 80] == z, f"z[{i}]"
                    assert got[160 * i + 80:160 * i + 112] == oracle.evaluate_polynomial(data[i], z, oracle_settings), f"y[{i}]"
            else:
                with pytest.raises(OracleError) as e:
                    oracle.verify_batch_intermediates(data, cs, cs, oracle_settings)
                print("non-canonical element: rc", rc, "status", st[0], "oracle", e.value.code)
                assert rc == 1 and st[0] == e.value.code
    finally:
        s.free()


def test_validate_points_on_spoiled_commitments_and_proofs(kz, setup_bytes, oracle, oracle_settings, fx64):
    import torch
    blobs, cs, ps = fx64
    n = len(blobs)
    off, sub = _special_points(oracle)
    batches = [(list(cs), list(ps)) for _ in range(7)]
    for g, (which, k, enc) in enumerate(((0, 17, off), (0, 63, sub), (0, 1, INF), (1, 0, off), (1, 31, sub), (1, 62, INF)), start=1):
        batches[g][which][k] = enc
    G = len(batches)
    want = [_oracle_batch(oracle, oracle_settings, blobs, c, p) for c, p in batches]
    assert [w[0] for w in want] == [0, 1, 1, 0, 1, 1, 0] and [w[1][3] for w in want if w[0] == 0] == [True, False, False]      # (the cases are what they claim)
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes, lincomb_form=2)                   # the bucket form: its stage 1 validates with k_validate_points
    try:
        tb = _dev(torch, s, b"".join(blobs) * G)
        tc = _dev(torch, s, b"".join(b"".join(c) for c, _ in batches))
        tp = _dev(torch, s, b"".join(b"".join(p) for _, p in batches))
        torch.cuda.synchronize()
        ok = (C.c_bool * G)(); st = (C.c_int * G)()
        rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle)
        print("many_device: rc", rc, "status", list(st), "ok", [bool(x) for x in ok])
        assert rc == 1 and [st[g] for g in range(G)] == [w[0] for w in want]
        assert [bool(ok[g]) for g in range(G) if want[g][0] == 0] == [w[1][3] for w in want if w[0] == 0]
        # the decoded points through the sums they enter: stage 1's records of the batches without an error, then stage 2's intermediates
        rec = torch.zeros(160 * n * G, dtype=torch.uint8, device=tb.device)
        torch.cuda.synchronize()
        st1 = (C.c_int * G)()
        rc = L.kzg355_verify_shard_records_device(rec.data_ptr(), st1, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle)
        assert rc == 1 and [st1[g] for g in range(G)] == [w[0] for w in want]
        good = [g for g in range(G) if want[g][0] == 0]
        good_rec = torch.cat([rec[160 * n * g:160 * n * (g + 1)] for g in good]).contiguous()
        torch.cuda.synchronize()
        for g, have in zip(good, _intermediates(L, s, good_rec, n, len(good))):
            assert have == want[g][1], g
    finally:
        s.free()


@pytest.mark.parametrize("chain_from", [1, 1 << 24], ids=["wsum+hchain_quad", "horner"])
def test_bucket_form_and_tails_on_64_batches_of_8(chain_from, kz, setup_bytes, small_batches):
    import torch
    cut, want, sw, want_sw = small_batches
    n, G, bad = 8, 64, 59                                          # batch g is cut[g % 8]; batch 59 (cut[3]) carries the two swapped proofs
    L = kz.kzg.lib()
    s = _handle(kz, setup_bytes, lincomb_form=2, lc_chain_from=chain_from)
    try:
        order = [g % 8 for g in range(G)]
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
    finally:
        s.free()
