"""-m gpu: verify_blob_kzg_proof_batch_many_sets -- verify_blob_kzg_proof_batch on batches of different blob counts in one call -- against the CPU
(tests/blob_sets_cases.py, pinned without a GPU by tests/test_blob_sets_cases.py).  Every call runs through the debug forms on host arrays and
on device arrays; the verdict, the status and all 128 bytes r | proof_lincomb | rhs of every group are compared byte for byte with the CPU's
answer for that group ALONE.  A valid group verifies under any r, so no test asks for True alone: a group that read its neighbour's records,
its neighbour's r powers or lincomb items from across a border has other bytes.  No tolerance anywhere.  Every output array lies between guard
bytes, and the guards are checked after every call.

  1 borders     counts [0, 1, 2, 0, 0, 10, 11, 1, 6, 0] and the same reversed: a wave of lincomb items straddles groups, a group spans two waves,
                empty groups first, last and adjacent
  2 many        130 groups, 78 of them hashed: more than one wave of the lanes form, more than one workgroup of the wave form; on a default
                handle, on one with KZG355_RHASH_LANES_FROM=1, on one with KZG355_HOST_RHASH=off and on one with both
  3 large       [64, 1, 447] (stride loops beyond 64 lanes) and [512] against tests/golden/batch512.json
  4 spoils      swapped proofs, the modulus as a blob element, a commitment with x >= p and one off the subgroup, each in its own group
  5 launch sets the set limit lowered (kzg355_settings_set_blob_sets_max_blobs): the same bytes, the predicted number of sets
  6 replicas    three replicas of device 0: the same bytes, the blobs per device the cut rule predicts
  7 minimal     [1, 3, 0, 2] on an N = 4 handle against the oracle's minimal preset
  8 mirrors     the Python and C++ mirrors"""
import ctypes as C
import json
import os
import subprocess

import pytest

import blob_sets_cases as bs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BADARGS = 1
GUARD = 16


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, devices=None, **more):
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer", **more)      # no wide table per handle
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


@pytest.fixture(scope="module")
def s1(kz, setup_bytes):
    s = _load(kz, setup_bytes)
    yield s
    s.free()


class Guarded:
    """`size` bytes of output between two runs of guard bytes"""

    def __init__(self, size):
        self.size = size
        self.buf = C.create_string_buffer(b"\xa5" * (2 * GUARD + size), 2 * GUARD + size)

    def ptr(self, ctype):
        return C.cast(C.addressof(self.buf) + GUARD, C.POINTER(ctype))

    def data(self):
        raw = self.buf.raw
        assert raw[:GUARD] == b"\xa5" * GUARD and raw[GUARD + self.size:] == b"\xa5" * GUARD, "guard bytes overwritten"
        return raw[GUARD:GUARD + self.size]


def run(kz, s, call, device):
    """the debug form on host or device arrays -> (return value, per group "BadArgs" | (verdict, 128 bytes))"""
    from kzg_rust_amd.kzg import lib
    G = len(call.counts)
    ok, st, out = Guarded(G), Guarded(4 * G), Guarded(128 * G)
    cnt = (C.c_size_t * max(G, 1))(*call.counts)
    blobs, cs, ps = call.flat()
    if device:
        import torch
        keep = [torch.frombuffer(bytearray(x), dtype=torch.uint8).to("cuda:0") if x else None for x in (blobs, cs, ps)]
        ptrs = [C.c_void_p(t.data_ptr()) if t is not None else None for t in keep]
        rc = lib().kzg355_debug_batch_intermediates_sets_device(C.cast(out.ptr(C.c_char), C.c_char_p), ok.ptr(C.c_bool), st.ptr(C.c_int), cnt, *ptrs, G,
                                                                s.handle)
    else:
        rc = lib().kzg355_debug_batch_intermediates_sets(C.cast(out.ptr(C.c_char), C.c_char_p), ok.ptr(C.c_bool), st.ptr(C.c_int), cnt, blobs, cs, ps, G,
                                                         s.handle)
    okb, stb, outb = ok.data(), st.data(), out.data()
    res = []
    for g in range(G):
        status = int.from_bytes(stb[4 * g:4 * g + 4], "little")
        assert okb[g] in (0, 1) and status in (0, BADARGS), (call.name, g, okb[g], status)
        if status == BADARGS:
            assert okb[g] == 0, (call.name, g)
            res.append("BadArgs")
        else:
            res.append((bool(okb[g]), outb[128 * g:128 * g + 128]))
    return rc, res


def check(kz, s, oracle, oracle_settings, call, forms=(False, True)):
    want = bs.answers(oracle, oracle_settings, call)
    first = BADARGS if "BadArgs" in want else 0
    for device in forms:
        rc, got = run(kz, s, call, device)
        for g, (a, b) in enumerate(zip(got, want)):
            assert a == b, (call.name, "device" if device else "host", g, call.counts[g])
        assert rc == first, (call.name, device, rc)
    return want


def test_borders_of_the_item_numbering(kz, s1, oracle, oracle_settings):
    call = bs.borders()
    want = check(kz, s1, oracle, oracle_settings, call)
    assert [w[0] for w in want] == [True] * 10 and [w[1] == bs.ZERO128 for w in want] == [c == 0 for c in call.counts]
    check(kz, s1, oracle, oracle_settings, call.reversed())


# (a lone call of at most 1024 records hashes its transcripts on the host unless the handle says KZG355_HOST_RHASH=off: the default handle takes that
# route, "host-rhash-off" the wave form of the device hash -- 78 hashed groups in 130 one-wave workgroups --, and the last handle the lanes form)
HASH_HANDLES = [{}, {"KZG355_RHASH_LANES_FROM": "1"}, {"KZG355_HOST_RHASH": "off"}, {"KZG355_RHASH_LANES_FROM": "1", "KZG355_HOST_RHASH": "off"}]


@pytest.mark.parametrize("env", HASH_HANDLES, ids=["default", "lanes-from-1", "host-rhash-off", "lanes-from-1-host-rhash-off"])
def test_many_groups_both_hash_forms(kz, s1, setup_bytes, oracle, oracle_settings, env):
    s = _load(kz, setup_bytes, **env) if env else s1
    try:
        check(kz, s, oracle, oracle_settings, bs.many())
    finally:
        if env:
            s.free()


def test_large_beside_small(kz, s1, oracle, oracle_settings):
    check(kz, s1, oracle, oracle_settings, bs.large())
    call = bs.whole512()
    (ok, dump), = check(kz, s1, oracle, oracle_settings, call)
    raw = call.fx.raw
    assert ok is True and (dump[:32].hex(), dump[32:80].hex(), dump[80:].hex()) == (raw["r"], raw["proof_lincomb"], raw["rhs"])


def test_spoils_stay_in_their_groups(kz, s1, oracle, oracle_settings, golden_vectors):
    clean = bs.answers(oracle, oracle_settings, bs.borders())
    for name, (call, changed) in bs.spoil_calls(golden_vectors, oracle).items():
        want = check(kz, s1, oracle, oracle_settings, call)
        for g in range(len(call.counts)):
            if g in changed:
                assert (want[g] if want[g] == "BadArgs" else want[g][0]) == changed[g], (name, g)
            else:
                assert want[g] == clean[g], (name, g)      # the neighbours are intact, byte for byte (check() compared the device with `want`)


def _sets_run(kz, s, call, device):
    """the call with kernel timing on -> (results, launch sets it took: one err_fold launch each)"""
    from kzg_rust_amd.kzg import lib
    lib().kzg355_set_kernel_timing(s.handle, 1)
    lib().kzg355_reset_kernel_stats(s.handle)
    rc, got = run(kz, s, call, device)
    total, launches = C.c_double(), C.c_long()
    assert lib().kzg355_kernel_ms_stats(s.handle, b"err_fold", C.byref(total), C.byref(launches)) == 0
    lib().kzg355_set_kernel_timing(s.handle, 0)
    return rc, got, launches.value


def test_launch_sets(kz, s1, setup_bytes, oracle, oracle_settings):
    many, borders = bs.many(), bs.borders()
    one_set = {c.name: [run(kz, s1, c, d)[1] for d in (False, True)] for c in (many, borders)}
    for c in (many, borders):
        assert one_set[c.name][0] == one_set[c.name][1] == bs.answers(oracle, oracle_settings, c)
    assert _sets_run(kz, s1, many, True)[2] == 1
    # limits 1 and 5 together break between every pair of neighbouring groups of `many` (test_blob_sets_cases); with 5, the 10- and 11-blob groups
    # of `borders` are larger than the limit and run as sets of their own
    from kzg_rust_amd.kzg import lib
    assert lib().kzg355_settings_set_blob_sets_max_blobs(s1.handle, (1 << 24) + 1) == BADARGS
    try:
        for limit in (1, 5):
            s1.set_blob_sets_max_blobs(limit)
            for c in (many, borders):
                for d, device in enumerate((False, True)):
                    rc, got, sets = _sets_run(kz, s1, c, device)
                    assert rc == 0 and got == one_set[c.name][d], (limit, c.name, device)
                    assert sets == len(bs.set_breaks(c.counts, limit)), (limit, c.name, device, sets)
    finally:
        s1.set_blob_sets_max_blobs(0)                             # the default again
    assert _sets_run(kz, s1, many, False)[2] == 1


def test_three_replicas_cut_by_blobs(kz, setup_bytes, oracle, oracle_settings):
    s = _load(kz, setup_bytes, devices=[0, 0, 0])
    try:
        assert s.device_count == 3
        call = bs.many()
        before = s.blob_sets_blobs_per_device()
        check(kz, s, oracle, oracle_settings, call, forms=(False,))
        after = s.blob_sets_blobs_per_device()
        assert [a - b for a, b in zip(after, before)] == bs.device_cuts(call.counts, 3) == [94, 98, 94]
        # the device form stays on the first device
        check(kz, s, oracle, oracle_settings, call, forms=(True,))
        assert [a - b for a, b in zip(s.blob_sets_blobs_per_device(), after)] == [286, 0, 0]
    finally:
        s.free()


def test_minimal_preset(kz, setup_bytes):
    from oracle.oracle import Oracle
    fx = json.load(open(os.path.join(HERE, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    lagrange = [bytes.fromhex(x) for x in fx["setup_g1_lagrange"]]
    o = Oracle(preset="minimal")
    os_ = o.load_trusted_setup(b"".join(lagrange), g2)
    s = kz.Kzg.load_trusted_setup(lagrange, [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        assert s.field_elements_per_blob == 4
        call = bs.minimal(fx)
        want = check(kz, s, o, os_, call)
        assert [w[0] for w in want] == [True] * 4
        spoiled = bs.Call("minimal-swapped", call.fx, bs.MINIMAL, {1: [("proof", call.fx.proofs[2])], 2: [("proof", call.fx.proofs[1])]})
        assert [w[0] for w in check(kz, s, o, os_, spoiled)] == [True, False, True, True]
    finally:
        s.free()
        o.free_trusted_setup(os_)


def test_python_and_cpp_mirrors(kz, s1, oracle, oracle_settings, golden_vectors, tmp_path):
    import torch
    clean, (swapped, _) = bs.borders(), bs.spoil_calls(golden_vectors, oracle)["swapped-proofs"]
    for call in (clean, swapped):
        want = [w[0] for w in bs.answers(oracle, oracle_settings, call)]
        assert kz.Kzg.verify_blob_kzg_proof_batch_many_sets(call.groups(), s1) == want
        res, dumps = kz.Kzg.debug_batch_intermediates_sets(call.groups(), s1)
        assert res == want and dumps == [w[1] for w in bs.answers(oracle, oracle_settings, call)]
        dev = [torch.frombuffer(bytearray(x), dtype=torch.uint8).to("cuda:0") for x in call.flat()]
        assert kz.Kzg.verify_blob_kzg_proof_batch_many_sets_device(*dev, call.counts, s1) == want
        assert kz.Kzg.debug_batch_intermediates_sets_device(*dev, call.counts, s1)[0] == want
    assert want == [True, True, True, True, True, False, True, True, False, True]
    assert kz.Kzg.verify_blob_kzg_proof_batch_many_sets([], s1) == [] and kz.Kzg.verify_blob_kzg_proof_batch_many_sets([([], [], [])], s1) == [True]
    runner = os.path.join(HERE, "native", "cpp_blob_sets_runner")
    inp = str(tmp_path / "groups_in.bin")
    with open(inp, "wb") as f:
        for b, c, p in swapped.groups():
            f.write(len(b).to_bytes(4, "little") + b"".join(b) + b"".join(c) + b"".join(p))
    out = subprocess.run([runner, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), inp],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[:-1] == ["true" if w else "false" for w in want]
    assert lines[-1] == "mismatch 1"                              # Error::BadArgs: the mirror's own length check, a proof dropped from one group
