"""-m gpu: verify_blob_cell_proofs_batch_many_sets -- groups of whole blobs, every group its own blob count, in one set of launches -- against the
CPU (tests/blob_cell_sets_cases.py, whose calls and answers tests/test_blob_cell_sets_cases.py pins to tests/cell_spec.py without a GPU).  Every
call runs through the host form with interp_form 0, 1 and 2, the device form with interp_form 1, 2 times prep_form 1, 2, and the two plain entry
points; the verdict, the status and all 176 bytes r | [I(tau)]_1 | LL | RL of every group are compared byte for byte with the CPU's answer for
that group ALONE.  A valid group verifies under any r, so no test asks for True alone: a group that read its neighbour's offsets, its
neighbour's r powers or commitments deduplicated across the border has other bytes.  No tolerance anywhere.

What the calls cross (listed in blob_cell_sets_cases): offsets behind an empty group; 6 | 7 blobs in the launch set (columns | coefficients);
the largest group first and last (k_blob_coef's per-group loop, k_cell_sum's second pass at 384 cells next to a one-pass group); commitments
shared by the groups of one call; statuses by position; k_cell_rhash_wave_sets | k_cell_rhash_lanes_sets on 2 | 3 groups of different lengths;
equal counts against the uniform call; 2050 blobs in two launch sets with a group that would straddle blob 2048; three replicas; a shrinking and
a growing call on one workspace; empty calls.

MEASURED (one run, MI355X; the lines this module prints): the 2050-blob call (281 MB of host bytes, 898 groups) takes 0.22 - 0.26 s per route
from host memory and 0.10 - 0.19 s from device memory, building its arguments 0.41 s; every other call 0.010 - 0.012 s, 0.03 - 0.06 s with
prep_form 1 (the device hashes); the CPU answer of a group 0.12 - 0.25 s; the module 13.4 s."""
import ctypes as C
import os
import time

import pytest

import blob_cell_sets_cases as ss
import blob_cell_shape_cases as sc

pytestmark = pytest.mark.gpu

BADARGS = 1
HOST_FORMS = (0, 1, 2)
DEVICE_FORMS = tuple((i, p) for i in (1, 2) for p in (1, 2))


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, devices, **more):
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer", **more)      # no wide table per replica
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
    s = _load(kz, setup_bytes, None)
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def named(oracle, fx):
    return ss.named_groups(sc.Pools(oracle, fx))


@pytest.fixture(scope="module")
def want(oracle, fx):
    """the CPU's answer per group name, computed once and shared by the tests of this module"""
    known = {}

    def get(g):
        sc.check_claims(g)
        if g.name not in known:
            t0 = time.perf_counter()
            known[g.name] = g.args, ss.answer(oracle, fx, g)
            print(f"CPU, {g.name} ({g.n} blobs): {time.perf_counter() - t0:.3f} s")
        args, answer = known[g.name]
        assert args == g.args, f"two different groups are called {g.name}"
        assert (answer == "BadArgs") == (g.kind == "malformed") and (answer == "BadArgs" or answer[1] is (g.kind == "valid")), (g.name, g.kind)
        return answer
    return get


def u8(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")


def to_device(groups):
    blobs, c, p, _ = ss.flat(groups)
    if not blobs:
        return None, None, None
    return u8(b"".join(blobs)), u8(b"".join(c)), u8(b"".join(p))


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def host_call(kz, s, groups, interp_form=0):
    res, out = kz.Kzg.debug_blob_cell_batch_intermediates_sets([g.args for g in groups], s, interp_form)
    return norm(res), out


def run_routes(kz, s, groups, host_forms=HOST_FORMS, device_forms=DEVICE_FORMS, plain=True):
    """{route: (verdicts, [176 bytes per group] or None)} of one `_sets` call per route"""
    out, cnts = {}, ss.counts(groups)

    def timed(route, f):
        t0 = time.perf_counter()
        out[route] = f()
        print(f"counts {cnts if len(cnts) < 10 else str(len(cnts)) + ' groups'}, {route}: {time.perf_counter() - t0:.3f} s")
    for f in host_forms:
        timed(f"host call, interp_form {f}", lambda: host_call(kz, s, groups, f))
    d = to_device(groups) if device_forms or plain else None
    for i, p in device_forms:
        def dev():
            res, o = kz.Kzg.debug_blob_cell_batch_intermediates_sets_device(*d, cnts, s, i, p)
            return norm(res), o
        timed(f"device call, interp_form {i}, prep_form {p}", dev)
    if plain:
        timed("verify_blob_cell_proofs_batch_many_sets", lambda: (norm(kz.Kzg.verify_blob_cell_proofs_batch_many_sets([g.args for g in groups], s)), None))
        timed("verify_blob_cell_proofs_batch_many_sets_device", lambda: (norm(kz.Kzg.verify_blob_cell_proofs_batch_many_sets_device(*d, cnts, s)), None))
    return out


def parts(o):
    return {"r": o[:32].hex(), "itau": o[32:80].hex(), "ll": o[80:128].hex(), "rl": o[128:176].hex()}


def same_as_cpu(route, groups, cpu, res, outs):
    """the verdict and all 176 bytes of every group are the CPU's for that group alone; a group the CPU refuses is BadArgs (bytes unspecified)"""
    assert len(res) == len(groups)
    for t, (g, w) in enumerate(zip(groups, cpu)):
        if w == "BadArgs":
            assert res[t] == "BadArgs", (route, t, g.name, res[t])
            continue
        if outs is not None:
            assert parts(outs[t]) == parts(w[0]), (route, t, g.name)
        assert res[t] is w[1], (route, t, g.name, res[t])


def check_exact(kz, s, want, groups, **routes):
    cpu = [want(g) for g in groups]
    got = run_routes(kz, s, groups, **routes)
    for route, (res, outs) in got.items():
        same_as_cpu(route, groups, cpu, res, outs)
    return got, cpu


def moved(s, before):
    return [a - b for a, b in zip(s.cell_calls_per_device(), before)]


# ---- 1. offsets and an empty group; 6 | 7 blobs in the launch set
@pytest.mark.parametrize("name", ["offsets-7", "offsets-3", "route-6", "route-7"])
def test_offsets_and_route_choice(kz, s1, named, want, name):
    gs = ss.call(named, name)
    before = s1.cell_calls_per_device()
    got, cpu = check_exact(kz, s1, want, gs)
    assert len(got) == 9 and moved(s1, before) == [9]             # one launch set per call, whatever the counts
    assert len({w[0] for w in cpu}) == len(gs)                    # every group has its own bytes (the empty one zeros)
    for g, w, o in zip(gs, cpu, got["host call, interp_form 0"][1]):
        assert (g.n == 0) == (o == bytes(176))


# ---- 2. the largest group first, and last
@pytest.mark.parametrize("name", ["largest-first", "largest-last"])
def test_largest_group_placement(kz, s1, named, want, name):
    gs = ss.call(named, name)
    assert max(ss.counts(gs)) == 4 and sorted(ss.counts(gs)) == [1, 1, 4]
    check_exact(kz, s1, want, gs)


# ---- 3. deduplication stops at the border
@pytest.mark.parametrize("name", ["shared", "shared-zero"])
def test_commitments_shared_across_groups(kz, s1, named, want, name):
    gs = ss.call(named, name)
    assert [g.distinct for g in gs] == [2, 1, 2] and gs[0].first == gs[2].first[::-1] and gs[1].first == gs[0].first[:1]
    if name == "shared-zero":
        assert gs[0].c[1] == sc.INF and gs[2].c[0] == sc.INF
    got, cpu = check_exact(kz, s1, want, gs)
    assert len({w[0][:32] for w in cpu}) == 3                     # each group its own r


# ---- 4. statuses by position
def test_statuses_by_position(kz, s1, named, want):
    gs = ss.call(named, "statuses")
    expect = [False, "BadArgs", True, True, "BadArgs"]
    got, cpu = check_exact(kz, s1, want, gs)
    for route, (res, _) in got.items():
        assert res == expect, route
    blobs, c, p, cnts = ss.flat(gs)
    G = len(gs)
    ok, st, cnt = (C.c_bool * G)(), (C.c_int * G)(*([7] * G)), (C.c_size_t * G)(*cnts)
    rc = kz.kzg.lib().kzg355_verify_blob_cell_proofs_batch_many_sets(ok, st, cnt, b"".join(blobs), b"".join(c), b"".join(p), G, s1.handle)
    assert rc == BADARGS and list(st) == [0, BADARGS, 0, 0, BADARGS]       # the return value is the first non-OK status
    assert [bool(x) for x in ok] == [False, False, True, True, False]
    # the off-curve proof alone: the first non-OK status is the last group's
    tail = gs[2:]
    res, out = host_call(kz, s1, tail)
    same_as_cpu("the last group malformed", tail, cpu[2:], res, out)


# ---- 5. both device hash kernels on ragged lengths
def test_both_device_hash_kernels_on_ragged_lengths(kz, setup_bytes, named, want):
    s = _load(kz, setup_bytes, None, KZG355_RHASH_LANES_FROM="3")
    try:
        for name in ("hash-2", "hash-3"):                         # k_cell_rhash_wave_sets, k_cell_rhash_lanes_sets
            gs = ss.call(named, name)
            assert len(set(ss.counts(gs))) == len(gs)
            d, cpu = to_device(gs), [want(g) for g in gs]
            for interp_form in HOST_FORMS:
                res, out = kz.Kzg.debug_blob_cell_batch_intermediates_sets_device(*d, ss.counts(gs), s, interp_form, 1)
                same_as_cpu(f"{name}, interp_form {interp_form}", gs, cpu, norm(res), out)
    finally:
        s.free()


# ---- 6. uniform and ragged calls agree
def test_equal_counts_agree_with_the_uniform_call(kz, s1, named, want):
    gs = ss.call(named, "uniform")
    got, cpu = check_exact(kz, s1, want, gs)
    for form in HOST_FORMS:
        res, out = kz.Kzg.debug_blob_cell_batch_intermediates([g.args for g in gs], s1, form)
        assert (norm(res), out) == got[f"host call, interp_form {form}"]
        assert out == [w[0] for w in cpu]


# ---- 7. more blobs than one launch set takes
def test_chunks_of_whole_groups(kz, s1, named, want):
    gs = ss.chunked(named)
    t0 = time.perf_counter()
    cpu = [want(g) for g in gs]
    args = [g.args for g in gs]
    d = to_device(gs)
    print(f"2050 blobs in {len(gs)} groups: arguments built in {time.perf_counter() - t0:.3f} s")
    cnts = ss.counts(gs)
    before = s1.cell_calls_per_device()

    def timed(route, f):
        t0 = time.perf_counter()
        res, out = f()
        print(f"2050 blobs, {route}: {time.perf_counter() - t0:.3f} s")
        same_as_cpu(route, gs, cpu, norm(res), out)
    for form in HOST_FORMS:
        timed(f"host call, interp_form {form}", lambda: kz.Kzg.debug_blob_cell_batch_intermediates_sets(args, s1, form))
    for i, p in DEVICE_FORMS:
        timed(f"device call, interp_form {i}, prep_form {p}", lambda: kz.Kzg.debug_blob_cell_batch_intermediates_sets_device(*d, cnts, s1, i, p))
    timed("verify_blob_cell_proofs_batch_many_sets", lambda: (kz.Kzg.verify_blob_cell_proofs_batch_many_sets(args, s1), None))
    timed("verify_blob_cell_proofs_batch_many_sets_device", lambda: (kz.Kzg.verify_blob_cell_proofs_batch_many_sets_device(*d, cnts, s1), None))
    assert moved(s1, before) == [18]                              # nine calls of two launch sets


# ---- 8. a handle over three replicas
def test_several_replicas(kz, setup_bytes, s1, named, want):
    s3 = _load(kz, setup_bytes, [0, 0, 0])
    try:
        assert s3.device_count == 3
        for name, per_call in (("replicas-5", [1, 1, 1]), ("replicas-2", [1, 1, 0])):
            gs = ss.call(named, name)
            cpu = [want(g) for g in gs]
            before = s3.cell_calls_per_device()
            for form in HOST_FORMS:
                res, out = host_call(kz, s3, gs, form)
                same_as_cpu(f"three replicas, {name}, interp_form {form}", gs, cpu, res, out)
                assert (res, out) == host_call(kz, s1, gs, form)
            assert norm(kz.Kzg.verify_blob_cell_proofs_batch_many_sets([g.args for g in gs], s3)) == [w[1] for w in cpu]
            assert moved(s3, before) == [4 * x for x in per_call]     # four calls, one launch set on every replica that got a group
    finally:
        s3.free()


# ---- 9. workspace reuse and empty calls
def test_shrinking_and_growing_calls_and_empty_ones(kz, s1, named, want):
    for name in ("grow", "shrink", "grow"):
        gs = ss.call(named, name)
        for form in (1, 2):
            res, out = host_call(kz, s1, gs, form)
            same_as_cpu(f"{name}, interp_form {form}", gs, [want(g) for g in gs], res, out)
    before = s1.cell_calls_per_device()
    gs = ss.call(named, "all-empty")
    for form in HOST_FORMS:
        assert host_call(kz, s1, gs, form) == ([True] * 3, [bytes(176)] * 3)
    assert norm(kz.Kzg.verify_blob_cell_proofs_batch_many_sets([g.args for g in gs], s1)) == [True] * 3
    assert norm(kz.Kzg.verify_blob_cell_proofs_batch_many_sets_device(None, None, None, [0, 0, 0], s1)) == [True] * 3
    assert kz.Kzg.debug_blob_cell_batch_intermediates_sets_device(None, None, None, [0, 0, 0], s1, 1, 1) == ([True] * 3, [bytes(176)] * 3)
    assert kz.Kzg.verify_blob_cell_proofs_batch_many_sets([], s1) == [] and kz.Kzg.debug_blob_cell_batch_intermediates_sets([], s1) == ([], [])
    assert kz.Kzg.verify_blob_cell_proofs_batch_many_sets_device(None, None, None, [], s1) == []
    assert moved(s1, before) == [0]                               # no launch set counted


# ---- refusals that need a live handle
def test_refusals_as_a_whole_on_a_live_handle(kz, s1, named):
    lib = kz.kzg.lib()
    gs = ss.call(named, "offsets-3")
    blobs, c, p, cnts = (b"".join(x) if i < 3 else x for i, x in enumerate(ss.flat(gs)))
    G = len(gs)
    before = s1.cell_calls_per_device()

    def refused(f):
        ok, st = (C.c_bool * G)(*([True] * G)), (C.c_int * G)()
        rc = f(ok, st)
        assert rc == BADARGS and list(st) == [BADARGS] * G and [bool(x) for x in ok] == [False] * G
    cnt = (C.c_size_t * G)(*cnts)
    out = C.create_string_buffer(176 * G)
    refused(lambda ok, st: lib.kzg355_verify_blob_cell_proofs_batch_many_sets(ok, st, (C.c_size_t * G)(2, 2049, 1), blobs, c, p, G, s1.handle))
    refused(lambda ok, st: lib.kzg355_verify_blob_cell_proofs_batch_many_sets(ok, st, None, blobs, c, p, G, s1.handle))
    refused(lambda ok, st: lib.kzg355_verify_blob_cell_proofs_batch_many_sets(ok, st, cnt, None, c, p, G, s1.handle))
    refused(lambda ok, st: lib.kzg355_debug_blob_cell_batch_intermediates_sets(out, ok, st, cnt, blobs, c, p, G, 3, s1.handle))
    refused(lambda ok, st: lib.kzg355_debug_blob_cell_batch_intermediates_sets(None, ok, st, cnt, blobs, c, p, G, 0, s1.handle))
    d = to_device(gs)
    ptr = [x.data_ptr() for x in d]
    refused(lambda ok, st: lib.kzg355_debug_blob_cell_batch_intermediates_sets_device(out, ok, st, cnt, ptr[0], ptr[1], ptr[2], G, 0, 3, s1.handle))
    refused(lambda ok, st: lib.kzg355_verify_blob_cell_proofs_batch_many_sets_device(ok, st, cnt, ptr[0] + 8, ptr[1], ptr[2], G, s1.handle))
    assert moved(s1, before) == [0]
