"""-m gpu: the EIP-4844 point-evaluation precompile, batched on the device (kzg355_point_evaluation_many, its device form, the single call and
kzg_to_versioned_hash on device memory) against the cases of tests/point_eval_cases.py, whose expectations tests/test_point_eval_cases.py pins
on the CPU with hashlib and the oracle.  The semantics under test: an input whose versioned hash is not that of its commitment is false /
KZG355_OK with match false and NOTHING else reported; an input whose hash matches is exactly what kzg355_verify_kzg_proof_many says about its
four fields; the return value is the first non-OK status after that merge."""
import ctypes as C
import hashlib
import os
import subprocess
import threading

import numpy as np
import pytest

import point_eval_cases as pc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 0x5A
SET = 1 << 17
NO_MEMORY = 7


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def L(kz):
    return kz.kzg.lib()


def _setup_lists(setup_bytes):
    g1, g2 = setup_bytes
    return [g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)]


@pytest.fixture(scope="module")
def settings(kz, setup_bytes):
    s = kz.Kzg.load_trusted_setup(*_setup_lists(setup_bytes))
    yield s
    s.free()


def run(L, s, data, n, device_ptr=None, with_status=True, with_match=True):
    """one call of the host form (data: bytes) or the device form (device_ptr) between guard bytes on all three arrays -> (rc, ok, status, match)"""
    ok = np.full(n + 16, GUARD, dtype=np.uint8)
    m = np.full(n + 16, GUARD, dtype=np.uint8)
    st = np.full(n + 4, 0x5A5A5A5A, dtype=np.int32)
    p_ok = ok[8:].ctypes.data_as(C.POINTER(C.c_bool))
    p_st = st[2:].ctypes.data_as(C.POINTER(C.c_int)) if with_status else None
    p_m = m[8:].ctypes.data_as(C.POINTER(C.c_bool)) if with_match else None
    if device_ptr is None:
        rc = L.kzg355_point_evaluation_many(p_ok, p_st, p_m, data, n, s.handle)
    else:
        rc = L.kzg355_point_evaluation_many_device(p_ok, p_st, p_m, device_ptr, n, s.handle)
    assert (ok[:8] == GUARD).all() and (ok[8 + n:] == GUARD).all(), "ok: written outside the array"
    assert (m[:8] == GUARD).all() and (m[8 + n:] == GUARD).all(), "hash_match: written outside the array"
    assert (st[:2] == 0x5A5A5A5A).all() and (st[2 + n:] == 0x5A5A5A5A).all(), "status: written outside the array"
    if not with_status:
        assert (st == 0x5A5A5A5A).all()
    if not with_match:
        assert (m == GUARD).all()
    assert set(np.unique(ok[8:8 + n])) <= {0, 1}
    return rc, ok[8:8 + n].astype(bool), st[2:2 + n].copy(), m[8:8 + n].astype(bool)


def check(got, cases):
    rc, ok, st, m = got
    e_ok, e_st, e_m, e_rc = pc.expected(cases)
    bad = [c.name for i, c in enumerate(cases) if (ok[i], st[i], m[i]) != (e_ok[i], e_st[i], e_m[i])]
    assert not bad, bad[:8]
    assert rc == e_rc


def test_all_cases_in_one_host_call(L, settings):
    cases = pc.CASES
    data, n = pc.pack(cases), len(cases)
    full = run(L, settings, data, n)
    check(full, cases)
    assert full[0] == pc.BADARGS                                  # (the invalid inputs behind matching hashes)
    rc, ok, _, m = run(L, settings, data, n, with_status=False)
    assert rc == full[0] and (ok == full[1]).all() and (m == full[3]).all()
    rc, ok, st, _ = run(L, settings, data, n, with_match=False)
    assert rc == full[0] and (ok == full[1]).all() and (st == full[2]).all()
    rc, ok, _, _ = run(L, settings, data, n, with_status=False, with_match=False)
    assert rc == full[0] and (ok == full[1]).all()
    # the return value is the first non-OK status AFTER the merge: a mismatch in front of an invalid input, placed first, reports nothing
    hidden = [c for c in pc.MISMATCH if c.name.rsplit("/", 1)[0] in {b.name for b in pc.BY_KIND["invalid"]}]
    assert len(hidden) >= 12
    quiet = hidden[:3] + pc.BY_KIND["true"][:3] + pc.BY_KIND["false"][:2] + hidden[3:]
    got = run(L, settings, pc.pack(quiet), len(quiet))
    check(got, quiet)
    assert got[0] == pc.OK
    for n_status in (True, False):
        assert run(L, settings, pc.pack(quiet), len(quiet), with_status=n_status)[0] == pc.OK
    loud = quiet + pc.BY_KIND["invalid"][:1]
    assert run(L, settings, pc.pack(loud), len(loud), with_status=False)[0] == pc.BADARGS


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes_at_the_wave_edge_and_the_single_lincomb_threshold(L, settings, n):
    """63 / 64 / 65: one wave of k_pe_unpack and the 64-check threshold from which the records chain takes k_lincomb_single; three orders, so that
    a mismatch, an invalid input and a false proof each sit first and last"""
    for first, last in (("mismatch", "invalid"), ("invalid", "false"), ("false", "mismatch")):
        cases = pc.select(n, first, last)
        full = run(L, settings, pc.pack(cases), n)
        check(full, cases)
        rc, ok, _, _ = run(L, settings, pc.pack(cases), n, with_status=False, with_match=False)
        assert rc == full[0] and (ok == full[1]).all()


def test_device_form_against_host_form(kz, L, settings):
    import torch
    cases = pc.CASES
    data, n = pc.pack(cases), len(cases)
    dev = torch.device("cuda", settings.device)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    host = run(L, settings, data, n)
    got = run(L, settings, None, n, device_ptr=t.data_ptr())
    assert got[0] == host[0] and all((a == b).all() for a, b in zip(got[1:], host[1:]))
    check(got, cases)
    torch.cuda.synchronize()
    assert bytes(t.cpu().numpy()) == data, "the caller's device buffer was written"
    # the Python mirror over the same tensor
    res, match = kz.Kzg.point_evaluation_many_device(t, n, settings)
    res_h, match_h = kz.Kzg.point_evaluation_many([c.data for c in cases], settings)
    for c, r, mm, rh, mh in zip(cases, res, match, res_h, match_h):
        assert mm == mh == c.match, c.name
        for x in (r, rh):
            assert isinstance(x, kz.BadArgs) if c.status else x is c.ok, c.name
    # a view offset by 8 bytes refuses the call as a whole
    big = torch.zeros(192 * n + 16, dtype=torch.uint8, device=dev)
    big[8:8 + 192 * n] = t
    torch.cuda.synchronize()
    view = big[8:8 + 192 * n]
    assert view.data_ptr() % 16 == 8
    rc, ok, st, m = run(L, settings, None, n, device_ptr=view.data_ptr())
    assert rc == pc.BADARGS and not ok.any() and not m.any() and (st == pc.BADARGS).all()


def pe_unpack_launches(L, s):
    total, launches = C.c_double(), C.c_long()
    assert L.kzg355_kernel_ms_stats(s.handle, b"pe_unpack", C.byref(total), C.byref(launches)) == 0
    return launches.value


@pytest.mark.parametrize("n,launches", [(SET - 1, 1), (SET, 1), (SET + 1, 2)])
def test_set_border(L, settings, n, launches):
    """launch sets of at most 2^17 inputs: expectations by position across the border, both forms, one pe_unpack launch per set"""
    import torch
    dev = torch.device("cuda", settings.device)
    for pins in ({SET - 1: "mismatch", SET: "invalid", 0: "false", SET - 2: "true"}, {SET - 1: "invalid", SET: "mismatch", 0: "mismatch", SET - 2: "false"}):
        idx = pc.tiled(n, pins)
        data, e_ok, e_st, e_m = pc.arrays_of(idx)
        bad = e_st[e_st != pc.OK]
        e_rc = int(bad[0]) if len(bad) else pc.OK
        t = torch.from_numpy(data).to(dev)
        torch.cuda.synchronize()
        for ptr in (None, t.data_ptr()):
            L.kzg355_set_kernel_timing(settings.handle, 1)
            L.kzg355_reset_kernel_stats(settings.handle)
            rc, ok, st, m = run(L, settings, data.ctypes.data_as(C.c_char_p) if ptr is None else None, n, device_ptr=ptr)
            got_launches = pe_unpack_launches(L, settings)
            L.kzg355_set_kernel_timing(settings.handle, 0)
            assert rc != NO_MEMORY and rc == e_rc
            assert (ok == e_ok).all() and (st == e_st).all() and (m == e_m).all(), np.nonzero((ok != e_ok) | (st != e_st) | (m != e_m))[0][:8]
            assert got_launches == launches
        for pos, kind in pins.items():
            if pos < n:
                assert (e_m[pos], e_st[pos]) == {"mismatch": (False, pc.OK), "invalid": (True, pc.BADARGS), "false": (True, pc.OK), "true": (True, pc.OK)}[kind]


def test_against_the_existing_engine(kz, settings):
    """wherever the hash matches, ok / status are what kzg355_verify_kzg_proof_many returns on the four fields"""
    cases = pc.CASES
    f = [pc.fields(c.data) for c in cases]
    ref = kz.Kzg.verify_kzg_proof_many([x[3] for x in f], [x[1] for x in f], [x[2] for x in f], [x[4] for x in f], settings)
    res, match = kz.Kzg.point_evaluation_many([c.data for c in cases], settings)
    seen = 0
    for c, r, x, m in zip(cases, ref, res, match):
        if m:
            seen += 1
            assert type(r) is type(x) and (isinstance(r, Exception) or r is x), c.name
        else:
            assert x is False, c.name
    assert seen == len(pc.BASE)


def test_the_single_call(kz, L, settings):
    want = (4096).to_bytes(32, "big") + pc.BLS_MODULUS.to_bytes(32, "big")
    sentinel = bytes([GUARD]) * 80

    def call(data):
        out = C.create_string_buffer(sentinel, 80)
        rc = L.kzg355_point_evaluation(C.cast(C.addressof(out) + 8, C.c_char_p), data, len(data), settings.handle)
        assert out.raw[:8] == sentinel[:8] and out.raw[72:] == sentinel[72:]
        return rc, out.raw[8:72]

    for c in pc.BY_KIND["true"][:4]:
        assert call(c.data) == (pc.OK, want), c.name
        assert kz.Kzg.point_evaluation(c.data, settings) == want
    failing = pc.BY_KIND["mismatch"][:5] + pc.MISMATCH[-3:] + pc.BY_KIND["false"][:3] + pc.BY_KIND["invalid"][:3]
    for c in failing:
        assert call(c.data) == (pc.BADARGS, sentinel[:64]), c.name
    with pytest.raises(kz.BadArgs):
        kz.Kzg.point_evaluation(failing[0].data, settings)
    assert len(pc.LENGTHS) == 8
    for name, data in pc.LENGTHS:
        assert call(data) == (pc.BADARGS, sentinel[:64]), name


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_versioned_hash_on_the_device_against_hashlib(kz, settings, n):
    import torch
    dev = torch.device("cuda", settings.device)
    cs = [pc.fields(pc.BASE[i % len(pc.BASE)].data)[3] if i % 3 else hashlib.sha256(b"c%d" % i).digest() + bytes([i & 255] * 16) for i in range(n)]
    t_in = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).to(dev)
    t_out = torch.full((32 * n + 64,), GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    kz.Kzg.kzg_to_versioned_hash_many_device(t_out[:32 * n], t_in, n, settings)
    torch.cuda.synchronize()
    got = bytes(t_out.cpu().numpy())
    assert got[32 * n:] == bytes([GUARD]) * 64
    assert got[:32 * n] == b"".join(pc.vh(c) for c in cs)
    assert bytes(t_in.cpu().numpy()) == b"".join(cs)
    with pytest.raises(kz.BadArgs):                               # d_out off 16 bytes
        kz.Kzg.kzg_to_versioned_hash_many_device(t_out[8:8 + 32 * n], t_in, n, settings)


def test_a_handle_over_three_replicas_of_one_card(kz, L, setup_bytes, settings):
    old = os.environ.get("KZG355_MSM")
    os.environ["KZG355_MSM"] = "bucket"                            # no MSM table per replica: this test only verifies
    try:
        s3 = kz.Kzg.load_trusted_setup(*_setup_lists(setup_bytes), devices=[settings.device] * 3)
    finally:
        if old is None:
            del os.environ["KZG355_MSM"]
        else:
            os.environ["KZG355_MSM"] = old
    try:
        assert s3.device_count == 3
        for n in (2, 7):                                          # fewer inputs than replicas: one device; 7: ranges of 2, 2 and 3
            for first, last in (("mismatch", "invalid"), ("invalid", "false")):
                cases = pc.select(n, first, last)
                plain = run(L, settings, pc.pack(cases), n)
                multi = run(L, s3, pc.pack(cases), n)
                assert multi[0] == plain[0] and all((a == b).all() for a, b in zip(multi[1:], plain[1:]))
                check(multi, cases)
        check(run(L, s3, pc.pack(pc.CASES), len(pc.CASES)), pc.CASES)
    finally:
        s3.free()


def test_two_host_threads_on_one_handle(L, settings):
    sets = [pc.select(65, "mismatch", "invalid"), pc.select(64, "false", "mismatch")]
    results, errors = [None, None], []

    def work(k):
        try:
            for _ in range(3):
                results[k] = run(L, settings, pc.pack(sets[k]), len(sets[k]))
                check(results[k], sets[k])
        except BaseException as e:                                # noqa: BLE001 -- reported below, in the test's own thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results[0] is not None and results[1] is not None


def test_minimal_preset_handle(kz, L, setup_bytes):
    """verify_kzg_proof does not depend on the blob size: a FIELD_ELEMENTS_PER_BLOB = 4 handle serves the precompile, and the single call's first
    word reads that handle's FIELD_ELEMENTS_PER_BLOB"""
    import json
    from kzg_rust_amd import kzg_minimal as km
    fx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    s = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in fx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        case = fx["compute_kzg_proof"][0]
        c = bytes.fromhex(fx["commitments"][case["blob"]])
        z, y, p = (bytes.fromhex(case[k]) for k in ("z", "y", "proof"))
        good = pc.vh(c) + z + y + c + p
        y2 = ((int.from_bytes(y, "big") + 1) % pc.BLS_MODULUS).to_bytes(32, "big")
        wrong_y = pc.vh(c) + z + y2 + c + p
        wrong_h = bytes([good[0]]) + bytes([good[1] ^ 4]) + good[2:]
        rc, ok, st, m = run(L, s, good + wrong_y + wrong_h, 3)
        assert rc == pc.OK and list(ok) == [True, False, False] and list(st) == [0, 0, 0] and list(m) == [True, True, False]
        out = km.Kzg.point_evaluation(good, s)
        assert out == (4).to_bytes(32, "big") + pc.BLS_MODULUS.to_bytes(32, "big")
        for data in (wrong_y, wrong_h):
            with pytest.raises(kz.BadArgs):
                km.Kzg.point_evaluation(data, s)
    finally:
        s.free()


def test_cpp_mirror(tmp_path):
    native = os.path.join(HERE, "native")
    exe, src, hdr = os.path.join(native, "cpp_point_eval_runner"), os.path.join(native, "cpp_point_eval_runner.cpp"), os.path.join(ROOT, "include", "kzg355.hpp")
    if not os.path.exists(exe) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, src, "-L" + os.path.join(ROOT, "kzg_rust_amd"), "-lkzg355",
                        "-Wl,-rpath," + os.path.join(ROOT, "kzg_rust_amd")], check=True)
    cases = pc.BY_KIND["true"][:3] + pc.BY_KIND["false"][:3] + pc.BY_KIND["invalid"][:3] + pc.BY_KIND["mismatch"][:4] + pc.MISMATCH[-3:]
    inp = tmp_path / "cases.bin"
    inp.write_bytes(pc.pack(cases))
    out = subprocess.run([exe, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), str(inp)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    want_out = ((4096).to_bytes(32, "big") + pc.BLS_MODULUS.to_bytes(32, "big")).hex()
    assert len(lines) == len(cases) + 2
    for c, ln in zip(cases, lines):
        verdict = "err 1" if c.status else "true" if c.ok else "false"
        single = want_out if c.ok else "single_err 1"
        assert ln == f"{verdict} {'match' if c.match else 'nomatch'} {single}", (c.name, ln)
    assert lines[-2] == "short 1"
    assert lines[-1] == "vh " + pc.vh(pc.fields(cases[0].data)[3]).hex()
