"""-m gpu: the host-buffer entry points with the Fiat-Shamir challenges hashed on the HOST (kzg_rust_amd/csrc/host_sha256.cpp,
SURVEY 8f-4) and on the DEVICE (k_challenge*): every host-buffer parity check runs both ways.  The z_i (and y_i) of the stage-1
records are compared byte for byte with the oracle's in both modes; the reference's vectors for the three functions that hash a
blob (compute_blob_kzg_proof, verify_blob_kzg_proof, verify_blob_kzg_proof_batch; src/lib.rs:82-203) are replayed in both modes.
Transcript: reference src/kzg.rs:298-339; call shape of the bench: benches/kzg_benches.rs:113-120."""
import ctypes as C
import os
import threading

import pytest

from synth import random_blob
from vector_harness import run_function

pytestmark = pytest.mark.gpu

HASHING_FUNCTIONS = {"compute_blob_kzg_proof": 14, "verify_blob_kzg_proof": 24, "verify_blob_kzg_proof_batch": 22}
MODES = {"host": 1, "device": -1}


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
def backend():
    from gpu_backend import ProductBackend
    return ProductBackend()


@pytest.fixture(scope="module")
def batch(kz, settings):
    blobs = [random_blob(7000 + i) for i in range(67)]
    B = [kz.Blob(b) for b in blobs]
    settings.set_host_hash(-1)
    cs = kz.Kzg.blob_to_kzg_commitment_many(B, settings)
    ps = kz.Kzg.compute_blob_kzg_proof_many(B, cs, settings)
    settings.set_host_hash(0)
    return blobs, [c.to_bytes() for c in cs], [p.to_bytes() for p in ps]


def _records(kz, s, blobs, cs, ps, npg, groups):
    L = kz.kzg.lib()
    n = npg * groups
    out = C.create_string_buffer(160 * n)
    ok = (C.c_bool * groups)()
    st = (C.c_int * groups)()
    rc = L.kzg355_debug_verify_host_records(out, ok, st, b"".join(blobs[:n]), b"".join(cs[:n]), b"".join(ps[:n]), npg, groups, s.handle)
    return rc, list(ok), list(st), out.raw


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fn", list(HASHING_FUNCTIONS))
def test_reference_vectors_both_hash_routes(mode, fn, golden_vectors, golden_blobs, backend, settings):
    """The reference's test loop (src/lib.rs:82-203) for the functions that hash a blob, with the knob on and off."""
    settings.set_host_hash(MODES[mode])
    before = settings.host_hashed_calls
    try:
        n, failures = run_function(fn, golden_vectors, backend, settings, golden_blobs)
    finally:
        settings.set_host_hash(0)
    assert n == HASHING_FUNCTIONS[fn]
    assert not failures, "\n".join(failures)
    took_host = settings.host_hashed_calls - before
    assert (took_host > 0) == (mode == "host"), took_host


@pytest.mark.parametrize("mode", list(MODES))
def test_records_z_y_byte_exact_vs_oracle(mode, kz, settings, batch, oracle, oracle_settings):
    """z_i = hash_to_bls_field(SHA-256(transcript_i)) and y_i = p_i(z_i) of every blob, byte for byte against the oracle, through the
    host-buffer call; shapes: one batch of 64 (the bench call), 67 (a partial wave), 1 (the single-blob path), 4 batches of 16."""
    blobs, cs, ps = batch
    inter = oracle.verify_batch_intermediates(blobs, cs, ps, oracle_settings)
    settings.set_host_hash(MODES[mode])
    try:
        for npg, groups in ((64, 1), (67, 1), (1, 1), (16, 4), (3, 5)):
            before = settings.host_hashed_calls
            rc, ok, st, rec = _records(kz, settings, blobs, cs, ps, npg, groups)
            assert rc == 0 and ok == [True] * groups and st == [0] * groups, (npg, groups, rc, ok, st)
            assert (settings.host_hashed_calls - before == 1) == (mode == "host")
            for i in range(npg * groups):
                r = rec[160 * i:160 * i + 160]
                assert r[:48] == cs[i] and r[112:] == ps[i]
                assert r[48:80] == inter["z"][i], f"z[{i}] ({mode}, {npg} x {groups})"
                assert r[80:112] == inter["y"][i], f"y[{i}] ({mode}, {npg} x {groups})"
    finally:
        settings.set_host_hash(0)


@pytest.mark.parametrize("mode", list(MODES))
def test_verdicts_and_errors_both_hash_routes(mode, kz, settings, batch, oracle, oracle_settings):
    """Honest / swapped-proof / invalid-point / non-canonical-blob batches of odd sizes: same verdicts and same Errs either way
    (the host route changes the order of the work -- window shifts from x alone, validation beside them -- not the answers)."""
    blobs, cs, ps = batch
    B, Cm, Pr = [kz.Blob(b) for b in blobs], [kz.KzgCommitment(c) for c in cs], [kz.KzgProof(p) for p in ps]
    settings.set_host_hash(MODES[mode])
    try:
        for n in (2, 7, 33, 64, 65, 67):
            assert kz.Kzg.verify_blob_kzg_proof_batch(B[:n], Cm[:n], Pr[:n], settings) is True
            bad = list(Pr[:n]); bad[n - 1] = Pr[n - 2]
            assert kz.Kzg.verify_blob_kzg_proof_batch(B[:n], Cm[:n], bad, settings) is False
        n = 9
        assert oracle.verify_blob_kzg_proof_batch(blobs[:n], cs[:n], ps[:n], oracle_settings) is True
        # a proof that is on the curve but not in the subgroup, an x that is not on the curve, a bad flag byte, the point at infinity
        not_in_g1 = bytes.fromhex("8123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcde0")
        not_on_curve = bytes.fromhex("8123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef")
        for pos, badpt in ((0, not_in_g1), (n - 1, not_on_curve), (4, bytes(48)), (3, bytes([0x9a]) + b"\xff" * 47)):
            for which in ("proof", "commitment"):
                c2, p2 = list(Cm[:n]), list(Pr[:n])
                if which == "proof":
                    p2[pos] = kz.KzgProof(badpt)
                else:
                    c2[pos] = kz.KzgCommitment(badpt)
                with pytest.raises(kz.BadArgs):
                    kz.Kzg.verify_blob_kzg_proof_batch(B[:n], c2, p2, settings)
        inf = bytes([0xc0]) + bytes(47)
        p2 = list(Pr[:n]); p2[2] = kz.KzgProof(inf)
        assert kz.Kzg.verify_blob_kzg_proof_batch(B[:n], Cm[:n], p2, settings) is False      # infinity is a valid point (utils.rs:298-301), wrong proof
        noncanon = bytearray(blobs[1]); noncanon[32 * 77:32 * 78] = b"\xff" * 32
        b2 = list(B[:n]); b2[1] = kz.Blob(bytes(noncanon))
        with pytest.raises(kz.BadArgs):
            kz.Kzg.verify_blob_kzg_proof_batch(b2, Cm[:n], Pr[:n], settings)
        # the all-zero blob: commitment and proof at infinity, verdict true (the reference's 0xc0.. vectors)
        zero = kz.Blob(bytes(131072))
        assert kz.Kzg.verify_blob_kzg_proof_batch([zero, B[0]], [kz.KzgCommitment(inf), Cm[0]], [kz.KzgProof(inf), Pr[0]], settings) is True
        # blob proofs
        for i in (0, 5):
            assert kz.Kzg.compute_blob_kzg_proof(B[i], Cm[i], settings).to_bytes() == ps[i]
        got = kz.Kzg.compute_blob_kzg_proof_many(B[:5], Cm[:5], settings)
        assert [p.to_bytes() for p in got] == ps[:5]
    finally:
        settings.set_host_hash(0)


def test_auto_mode_crossover_and_portable_sha(kz, setup_bytes, batch):
    """mode 0 takes the host route up to the crossover only; KZG355_HOST_SHA=portable (CPUs without the SHA extensions) gives the same z."""
    blobs, cs, ps = batch
    g1, g2 = setup_bytes
    os.environ["KZG355_HOST_SHA"] = "portable"
    os.environ["KZG355_HOST_HASH_MAX"] = "8"
    try:
        s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    finally:
        del os.environ["KZG355_HOST_SHA"], os.environ["KZG355_HOST_HASH_MAX"]
    try:
        rc, ok, st, rec_host = _records(kz, s, blobs, cs, ps, 8, 1)
        assert rc == 0 and ok == [True] and s.host_hashed_calls == 1
        rc, ok, st, rec_dev = _records(kz, s, blobs, cs, ps, 9, 1)
        assert rc == 0 and ok == [True] and s.host_hashed_calls == 1          # above the crossover: device hash
        assert rec_host == rec_dev[:160 * 8]
    finally:
        s.free()


def test_concurrent_host_hashed_calls(kz, settings, batch):
    """Several threads on one handle, every call its own hashing job on the handle's shared host threads; verdicts hold."""
    blobs, cs, ps = batch
    B, Cm, Pr = [kz.Blob(b) for b in blobs], [kz.KzgCommitment(c) for c in cs], [kz.KzgProof(p) for p in ps]
    settings.set_host_hash(1)
    errors = []

    def work(k):
        try:
            for r in range(6):
                n = 5 + 7 * ((k + r) % 5)
                if kz.Kzg.verify_blob_kzg_proof_batch(B[:n], Cm[:n], Pr[:n], settings) is not True:
                    errors.append((k, r, "true expected"))
                bad = list(Pr[:n]); bad[0] = Pr[1]
                if kz.Kzg.verify_blob_kzg_proof_batch(B[:n], Cm[:n], bad, settings) is not False:
                    errors.append((k, r, "false expected"))
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    try:
        th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        settings.set_host_hash(0)
    assert not errors, errors


def test_four_threads_of_reference_shaped_calls_all_take_the_host_route(kz, settings, batch, oracle, oracle_settings):
    """no concurrency cliff on the small-call route.  Four threads x 20 verify_blob_kzg_proof_batch(n = 64) calls on host
    slices (the reference bench's call shape, benches/kzg_benches.rs:113-120) on ONE handle: every call has its challenges hashed on the host
    (round 3: one hashing slot per handle -- the second simultaneous caller took the 3.7 ms device hash and a 6 ms call), every verdict is true,
    and the calls do not queue behind each other beyond what the process's hardware queues impose.  Each call is a ~2.2 ms chain of small kernels on
    three streams of its own workspace, and the library gives a call its side streams only while the process's hardware queues (GPU_MAX_HW_QUEUES,
    set by whoever starts the process, csrc/engine.h) leave room for them.  With room for all four calls (3 x 4 queues or more) the median call of every
    thread stays below 3.5 ms; with fewer queues the runtime serialises the chains that share a queue, and the four threads together must still
    finish their 80 calls in at most 0.8 of the time one thread takes for the same calls back to back on the same handle.  z of a call made WHILE the other threads are
    hashing is byte-exact against the oracle."""
    import ctypes as C
    import time
    blobs, cs, ps = batch
    n = 64
    L = kz.kzg.lib()
    flat_b, flat_c, flat_p = b"".join(blobs[:n]), b"".join(cs[:n]), b"".join(ps[:n])
    for _ in range(3):                                   # warm the workspaces of one call
        ok = C.c_bool()
        assert L.kzg355_verify_blob_kzg_proof_batch(C.byref(ok), flat_b, n, flat_c, n, flat_p, n, settings.handle) == 0 and ok.value
    T, R = 4, 20
    one = []                                             # the same call back to back on one thread: the yardstick of the serialised case
    for _ in range(R):
        t0 = time.perf_counter()
        assert L.kzg355_verify_blob_kzg_proof_batch(C.byref(ok), flat_b, n, flat_c, n, flat_p, n, settings.handle) == 0 and ok.value
        one.append((time.perf_counter() - t0) * 1e3)
    before = settings.host_hashed_calls
    times = [[] for _ in range(T)]
    errors = []
    gate = threading.Barrier(T + 1)

    def work(k):
        ok = C.c_bool()
        gate.wait()
        for r in range(R):
            t0 = time.perf_counter()
            rc = L.kzg355_verify_blob_kzg_proof_batch(C.byref(ok), flat_b, n, flat_c, n, flat_p, n, settings.handle)
            times[k].append((time.perf_counter() - t0) * 1e3)
            if rc != 0 or not ok.value:
                errors.append((k, r, rc, ok.value))

    th = [threading.Thread(target=work, args=(k,)) for k in range(T)]
    for t in th:
        t.start()
    gate.wait()
    t0 = time.perf_counter()
    rc, okl, st, rec = _records(kz, settings, blobs, cs, ps, 8, 1)      # a fifth caller in the middle of it, records read back
    for t in th:
        t.join()
    wall_ms = (time.perf_counter() - t0) * 1e3
    assert not errors, errors
    assert settings.host_hashed_calls - before == T * R + 1, "a call fell back to the device hash"
    assert rc == 0 and okl == [True]
    want = oracle.shard_records(blobs[:8], cs[:8], ps[:8], oracle_settings)
    assert rec[:160 * 8] == want
    med = [sorted(t)[len(t) // 2] for t in times]
    allt = sorted(x for t in times for x in t)
    p80 = allt[int(0.8 * len(allt))]                     # (a few calls create workspaces: the first time four calls really overlap)
    one_med = sorted(one)[len(one) // 2]
    q = int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0)
    queues = q if 1 <= q <= 128 else 4                   # as the library reads it (csrc/options.hip)
    print(f"4 threads x 20 calls of n = 64 on {queues} hardware queues: median per thread {[round(m, 2) for m in med]} ms, 80th percentile of all calls "
          f"{p80:.2f} ms, {wall_ms:.1f} ms in all; one thread: {one_med:.2f} ms per call")
    if queues >= 3 * T:
        assert max(med) <= 3.5, med                       # measured 2.4-2.5 with 24 queues (profiles/r04/concurrent_small_calls.txt); round 3: 6.8
        assert p80 <= 4.5, p80
    else:
        # measured on 2 queues (MI355X): 158 ms for the 80 calls against 251 ms back to back (3.14 ms per call), 0.63 of it
        assert wall_ms <= 0.8 * T * R * one_med, (wall_ms, T * R * one_med, med)


def test_explicit_options_ignore_the_environment(kz, setup_bytes, batch, monkeypatch):
    """kzg355_load_trusted_setup_ex takes its knobs from the struct it is given: the KZG355_* variables (test overrides of the plain
    load functions) do not reach it.  Checked on two knobs with visible effects: the MSM form and the host hashing."""
    blobs, cs, ps = batch
    g1, g2 = setup_bytes
    monkeypatch.setenv("KZG355_HOST_HASH", "on")
    monkeypatch.setenv("KZG355_MSM_BITS", "13")
    s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)],
                                             msm_bits=8, host_hash=-1)
    try:
        assert s.msm_form == 8
        B, Cm, Pr = [kz.Blob(b) for b in blobs[:5]], [kz.KzgCommitment(c) for c in cs[:5]], [kz.KzgProof(p) for p in ps[:5]]
        assert kz.Kzg.verify_blob_kzg_proof_batch(B, Cm, Pr, s) is True and s.host_hashed_calls == 0
        assert kz.Kzg.blob_to_kzg_commitment(B[0], s).to_bytes() == cs[0]
    finally:
        s.free()
    s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)],
                                             host_hash=1, host_threads=3, lincomb_form=1, self_test=0)
    try:
        assert s.msm_form == 0 and s.msm_shape() == (0, 0, 0, 0)      # default: the MSM table is built by the first commitment / proof call, sized then
        assert kz.Kzg.verify_blob_kzg_proof_batch(B, Cm, Pr, s) is True and s.host_hashed_calls == 1
        assert s.msm_shape() == (0, 0, 0, 0)                          # verifying never builds it
        assert kz.Kzg.verify_blob_kzg_proof_batch(B, Cm, [Pr[1]] + Pr[1:], s) is False
    finally:
        s.free()


def _device_records(kz, s, blobs, cs, ps, npg, groups):
    """stage 1 of a DEVICE-RESIDENT call (kzg355_verify_shard_records_device on torch tensors): the 160-byte records, read back"""
    import torch
    L = kz.kzg.lib()
    dev = torch.device("cuda", s.device)
    n = npg * groups
    tb = torch.frombuffer(bytearray(b"".join(blobs[:n])), dtype=torch.uint8).to(dev)
    tc = torch.frombuffer(bytearray(b"".join(cs[:n])), dtype=torch.uint8).to(dev)
    tp = torch.frombuffer(bytearray(b"".join(ps[:n])), dtype=torch.uint8).to(dev)
    rec = torch.empty(160 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = (C.c_int * groups)()
    rc = L.kzg355_verify_shard_records_device(rec.data_ptr(), st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), npg, groups, s.handle)
    return rc, list(st), bytes(rec.cpu().numpy()), (tb, tc, tp)


@pytest.mark.parametrize("mode", list(MODES))
def test_device_resident_small_calls_take_the_host_route(mode, kz, settings, batch, oracle, oracle_settings):
    """a small call whose blobs are ALREADY in HBM copies them back in chunks and hashes on the host threads (5.3 -> ~2 ms for one
    64-blob batch) instead of the 3.7 ms device chain.  z_i and y_i of the records byte for byte against the oracle on that route and with it off
    (set_host_hash(-1)); verdicts / Errs of kzg355_verify_blob_kzg_proof_batch_many_device and blob proofs of the *_device call the same both ways."""
    import torch
    blobs, cs, ps = batch
    L = kz.kzg.lib()
    inter = oracle.verify_batch_intermediates(blobs, cs, ps, oracle_settings)
    settings.set_host_hash(0 if mode == "host" else -1)
    try:
        for npg, groups in ((64, 1), (67, 1), (1, 1), (16, 4), (3, 5), (2, 1)):
            before = settings.host_hashed_calls
            rc, st, rec, _ = _device_records(kz, settings, blobs, cs, ps, npg, groups)
            assert rc == 0 and st == [0] * groups, (npg, groups, rc, st)
            assert (settings.host_hashed_calls - before == 1) == (mode == "host"), (mode, npg, groups)
            for i in range(npg * groups):
                r = rec[160 * i:160 * i + 160]
                assert r[:48] == cs[i] and r[112:] == ps[i]
                assert r[48:80] == inter["z"][i], f"z[{i}] ({mode}, device-resident, {npg} x {groups})"
                assert r[80:112] == inter["y"][i], f"y[{i}] ({mode}, device-resident, {npg} x {groups})"
        # whole calls on device-resident inputs: honest, swapped proofs, an invalid point, a non-canonical element
        dev = torch.device("cuda", settings.device)
        n, G = 16, 4
        P = list(ps[:n * G]); P[16], P[17] = P[17], P[16]                      # batch 1: false
        Cm = list(cs[:n * G]); Cm[2 * 16 + 5] = bytes([0x9a]) + b"\xff" * 47    # batch 2: Err
        Bl = list(blobs[:n * G]); nc = bytearray(Bl[3 * 16 + 1]); nc[32 * 9:32 * 10] = b"\xff" * 32; Bl[3 * 16 + 1] = bytes(nc)   # batch 3: Err
        tb = torch.frombuffer(bytearray(b"".join(Bl)), dtype=torch.uint8).to(dev)
        tc = torch.frombuffer(bytearray(b"".join(Cm)), dtype=torch.uint8).to(dev)
        tp = torch.frombuffer(bytearray(b"".join(P)), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        ok = (C.c_bool * G)(); st = (C.c_int * G)()
        before = settings.host_hashed_calls
        rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, settings.handle)
        assert rc == 1 and list(st) == [0, 0, 1, 1] and bool(ok[0]) is True and bool(ok[1]) is False, (rc, list(st), list(ok))
        assert (settings.host_hashed_calls - before == 1) == (mode == "host")
        # blob proofs of device-resident blobs (the challenge hashes the blob: same route)
        out = C.create_string_buffer(48 * 5); st5 = (C.c_int * 5)()
        tb5 = torch.frombuffer(bytearray(b"".join(blobs[:5])), dtype=torch.uint8).to(dev)
        tc5 = torch.frombuffer(bytearray(b"".join(cs[:5])), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        before = settings.host_hashed_calls
        rc = L.kzg355_compute_blob_kzg_proof_many_device(out, st5, tb5.data_ptr(), tc5.data_ptr(), 5, settings.handle)
        assert rc == 0 and out.raw == b"".join(ps[:5])
        assert (settings.host_hashed_calls - before == 1) == (mode == "host")
    finally:
        settings.set_host_hash(0)


def test_device_resident_host_route_crossover(kz, setup_bytes, batch):
    """the route is taken up to host_hash_device_max_blobs only (default 1024; here 8), and never while submitted sets are in flight"""
    import torch
    blobs, cs, ps = batch
    g1, g2 = setup_bytes
    s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], host_hash_device_max_blobs=8)
    try:
        rc, st, rec8, _ = _device_records(kz, s, blobs, cs, ps, 8, 1)
        assert rc == 0 and s.host_hashed_calls == 1
        rc, st, rec9, _ = _device_records(kz, s, blobs, cs, ps, 9, 1)
        assert rc == 0 and s.host_hashed_calls == 1                            # above the crossover: device hash
        assert rec8 == rec9[:160 * 8]
        # with a submitted set out, a synchronous small device-resident call keeps the device hash
        L = kz.kzg.lib()
        dev = torch.device("cuda", s.device)
        tb = torch.frombuffer(bytearray(b"".join(blobs[:8])), dtype=torch.uint8).to(dev)
        tc = torch.frombuffer(bytearray(b"".join(cs[:8])), dtype=torch.uint8).to(dev)
        tp = torch.frombuffer(bytearray(b"".join(ps[:8])), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        tk = C.c_void_p()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device_submit(C.byref(tk), tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), 8, 1, s.handle) == 0
        ok = (C.c_bool * 1)(); st1 = (C.c_int * 1)()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st1, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), 8, 1, s.handle) == 0 and ok[0]
        assert s.host_hashed_calls == 1
        ok2 = (C.c_bool * 1)(); st2 = (C.c_int * 1)()
        assert L.kzg355_verify_collect(tk, ok2, st2) == 0 and ok2[0]
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st1, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), 8, 1, s.handle) == 0 and ok[0]
        assert s.host_hashed_calls == 2
    finally:
        s.free()


def test_device_resident_host_route_at_600_blobs_equals_the_device_hash(kz, setup_bytes, batch):
    """the route at a size that needs its eight chunks in earnest (600 blobs = 75 MiB back over PCIe, 10 batches of 60; host_hash_device_max_blobs = 1024):
    the records of the host-hashed and of the device-hashed run are the same bytes, and so are the verdicts of the whole call"""
    import torch
    blobs, cs, ps = batch
    g1, g2 = setup_bytes
    s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], host_hash_device_max_blobs=1024)
    try:
        npg, groups = 60, 10
        idx = [(7 * k) % 67 for k in range(npg * groups)]
        Bl, Cm, Pr = [blobs[i] for i in idx], [cs[i] for i in idx], [ps[i] for i in idx]
        rc, st, rec_host, (tb, tc, tp) = _device_records(kz, s, Bl, Cm, Pr, npg, groups)
        assert rc == 0 and st == [0] * groups and s.host_hashed_calls == 1
        s.set_host_hash(-1)
        rc, st, rec_dev, _ = _device_records(kz, s, Bl, Cm, Pr, npg, groups)
        assert rc == 0 and st == [0] * groups and s.host_hashed_calls == 1
        assert rec_host == rec_dev
        s.set_host_hash(0)
        L = kz.kzg.lib()
        ok = (C.c_bool * groups)(); stg = (C.c_int * groups)()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, stg, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), npg, groups, s.handle) == 0
        assert all(ok[i] for i in range(groups)) and s.host_hashed_calls == 2
    finally:
        s.free()


def test_handle_freed_with_a_ticket_out_is_released_by_the_last_collect(kz, setup_bytes, batch):
    """kzg355_free_trusted_setup with a submitted set not collected used to free what the ticket points into.  The free is deferred
    to the collect of the last ticket; the collect still returns the set's verdicts."""
    import torch
    blobs, cs, ps = batch
    g1, g2 = setup_bytes
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    L = kz.kzg.lib()
    dev = torch.device("cuda", s.device)
    n, G = 8, 3
    P = list(ps[:n * G]); P[8], P[9] = P[9], P[8]
    tb = torch.frombuffer(bytearray(b"".join(blobs[:n * G])), dtype=torch.uint8).to(dev)
    tc = torch.frombuffer(bytearray(b"".join(cs[:n * G])), dtype=torch.uint8).to(dev)
    tp = torch.frombuffer(bytearray(b"".join(P)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    tk = C.c_void_p()
    assert L.kzg355_verify_blob_kzg_proof_batch_many_device_submit(C.byref(tk), tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, G, s.handle) == 0
    s.free()                                                               # the caller's bug: a ticket is still out
    ok = (C.c_bool * G)(); st = (C.c_int * G)()
    assert L.kzg355_verify_collect(tk, ok, st) == 0
    assert [bool(x) for x in ok] == [True, False, True] and list(st) == [0, 0, 0]


def test_concurrent_device_resident_small_calls(kz, settings, batch):
    """Four threads making device-resident n = 64 calls on ONE handle at once: every call takes the host route on its own workspace (pinned slot, chunk
    events, hashing job on the shared host threads), honest batches are true and a batch with two proofs swapped is false -- no cross-talk between the calls."""
    import torch
    blobs, cs, ps = batch
    L = kz.kzg.lib()
    dev = torch.device("cuda", settings.device)
    n = 64
    tb = torch.frombuffer(bytearray(b"".join(blobs[:n])), dtype=torch.uint8).to(dev)
    tc = torch.frombuffer(bytearray(b"".join(cs[:n])), dtype=torch.uint8).to(dev)
    tp = torch.frombuffer(bytearray(b"".join(ps[:n])), dtype=torch.uint8).to(dev)
    sw = list(ps[:n]); sw[7], sw[40] = sw[40], sw[7]
    tsw = torch.frombuffer(bytearray(b"".join(sw)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    T, R = 4, 10
    errors = []
    before = settings.host_hashed_calls
    gate = threading.Barrier(T)

    def work(k):
        ok = (C.c_bool * 1)(); st = (C.c_int * 1)()
        gate.wait()
        for r in range(R):
            honest = (k + r) % 2 == 0
            rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), (tp if honest else tsw).data_ptr(), n, 1, settings.handle)
            if rc != 0 or st[0] != 0 or bool(ok[0]) is not honest:
                errors.append((k, r, rc, st[0], bool(ok[0]), honest))

    th = [threading.Thread(target=work, args=(k,)) for k in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert settings.host_hashed_calls - before == T * R


def test_load_free_cycles_release_device_memory(kz, setup_bytes, batch):
    """Thirty load -> a few calls (host-buffer, device-resident, submit / collect) -> free cycles: the device memory the process holds does not creep
    (workspaces, streams, the chunk events of the device-resident host route, tickets, the host threads all go with the handle)."""
    import torch
    blobs, cs, ps = batch
    g1, g2 = setup_bytes
    L = kz.kzg.lib()
    dev = torch.device("cuda", 0)
    n = 8
    tb = torch.frombuffer(bytearray(b"".join(blobs[:n])), dtype=torch.uint8).to(dev)
    tc = torch.frombuffer(bytearray(b"".join(cs[:n])), dtype=torch.uint8).to(dev)
    tp = torch.frombuffer(bytearray(b"".join(ps[:n])), dtype=torch.uint8).to(dev)
    B, Cm, Pr = [kz.Blob(b) for b in blobs[:n]], [kz.KzgCommitment(c) for c in cs[:n]], [kz.KzgProof(p) for p in ps[:n]]
    torch.cuda.synchronize()

    def cycle():
        s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], msm_bits=8, self_test=0)
        assert kz.Kzg.verify_blob_kzg_proof_batch(B, Cm, Pr, s) is True
        ok = (C.c_bool * 1)(); st = (C.c_int * 1)()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, 1, s.handle) == 0 and ok[0]
        tk = C.c_void_p()
        assert L.kzg355_verify_blob_kzg_proof_batch_many_device_submit(C.byref(tk), tb.data_ptr(), tc.data_ptr(), tp.data_ptr(), n, 1, s.handle) == 0
        assert L.kzg355_verify_collect(tk, ok, st) == 0 and ok[0]
        s.free()

    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(30):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 64 << 20, f"device memory crept by {(free0 - free1) >> 20} MiB over 30 load / free cycles"
