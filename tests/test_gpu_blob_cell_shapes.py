"""-m gpu: verify_blob_cell_proofs_batch at the sizes where its own code takes another path, against the CPU (tests/blob_cell_shape_cases.py, whose
groups and answers tests/test_blob_cell_shape_cases.py pins to tests/cell_spec.py without a GPU).  Every group runs through the host call with
interp_form 0, 1 and 2, the device call with interp_form 1, 2 times prep_form 1, 2 and the two plain entry points; r, [I(tau)]_1, LL, RL -- all 176
bytes -- and the verdict are compared with the CPU byte for byte on every route.  A valid group verifies under any weights, so a wrong r^(128 b), a
blob stride that matters only when blobs differ, a dropped tail of blobs or a wrong position of a commitment all answer True on copies of one blob:
here the blobs of a group differ, the bytes are the CPU's, and what is spoiled sits in the last blob and must be refused.  No tolerance anywhere.

The boundaries (the groups are listed in blob_cell_shape_cases): positions of repeated commitments (k_blob_meta), 6 | 7 blobs per launch set
(blob_interp_form), 256 | 384 cells per group (k_cell_sum's stride, n = 2 | 3), 128 | 129 blobs = 16384 | 16512 cells per group (the last group the
device hashes | the first the host must), 2 | 3 groups per call on a handle with KZG355_RHASH_LANES_FROM=3 (k_cell_rhash_wave | k_cell_rhash_lanes
over the index array k_blob_meta writes).  The blob call does not move settings.cell_device_prep_calls (blob_set never touches the counter), so
which side hashed the 128 and 129 groups is not asserted through it: above CELL_PREP_MAX_CELLS cell_device_call_prepares_on_host answers before it
looks at prep_form, and what is asserted is that every prep_form gives the CPU's r.

The CPU's answer for the 128- and 129-blob groups is blob_cell_shape_cases.BigReference (r from cell_spec.challenge, [I(tau)]_1 from the blobs'
coefficients, LL and RL from cell_spec.lincomb, the verdict from the oracle's pairings); every other group has cell_spec.verify_cell_kzg_proof_batch
over its 128 n cells.  MEASURED (one run, MI355X box; the lines this module prints):
  CPU, the `big` fixture: 129 mixture blobs built in 14.9 s; the references of the 128 / 129 / 129-swapped groups 4.9 / 1.7 / 1.7 s (the first
       validates the 16.6 thousand distinct points the three share); every other group 0.1 - 0.5 s, 24 of them
  GPU, one call of one group of 129 blobs: 0.040 - 0.044 s from host memory, 0.037 s from device memory, on every form
  GPU, one call of one group of 128 blobs: the same, but 0.95 - 1.2 s with prep_form 1 (one wave hashes 33.9 MB): the one place where the device's
       hash shows, and it does not show at 129
  GPU, one call of one group of 7 blobs: 0.010 - 0.011 s, 0.079 s with prep_form 1
  the module as a whole: 46 s, 23 s of them the `big` fixture"""
import ctypes as C
import os
import threading
import time

import pytest

import blob_cell_shape_cases as sc
import cell_device_cases as dcases
import cell_spec as cs

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
def pools(oracle, fx):
    return sc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def want(oracle, fx):
    """the CPU's answer per group -- (176 bytes, verdict) or "BadArgs" -- computed once per group name and shared by the tests of this module"""
    known, big = {}, sc.BigReference(oracle, fx)

    def get(g):
        sc.check_claims(g)
        if g.name not in known:
            t0 = time.perf_counter()
            try:
                known[g.name] = g.args, (big(g) if g.n >= sc.BIG - 1 else sc.expected(oracle, fx, g))
            except cs.BadArgs:
                known[g.name] = g.args, "BadArgs"
            print(f"CPU, {g.name} ({g.n} blobs): {time.perf_counter() - t0:.3f} s")
        args, answer = known[g.name]
        assert args == g.args, f"two different groups are called {g.name}"
        assert (answer == "BadArgs") == (g.kind == "malformed") and (answer == "BadArgs" or answer[1] is (g.kind == "valid")), (g.name, g.kind)
        return answer
    return get


@pytest.fixture(scope="module")
def big(pools, want):
    """the 128 and 129 groups of distinct mixtures and the 129 group with two proofs of its last blob exchanged, with their CPU answers"""
    t0 = time.perf_counter()
    out = {"128": sc.big_group(pools, 128), "129": sc.big_group(pools, 129), "129-swapped": sc.big_swapped(pools)}
    print(f"CPU, {sc.BIG} mixture blobs built: {time.perf_counter() - t0:.3f} s")
    assert [g.distinct for g in out.values()] == [128, 129, 129] and [g.kind for g in out.values()] == ["valid", "valid", "spoiled"]
    for g in out.values():
        want(g)
    return out


def u8(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")


def to_device(groups):
    return (u8(b"".join(b"".join(g.blobs) for g in groups)), u8(b"".join(b"".join(g.c) for g in groups)), u8(b"".join(b"".join(g.p) for g in groups)))


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def host_call(kz, s, groups, interp_form=0):
    res, out = kz.Kzg.debug_blob_cell_batch_intermediates([g.args for g in groups], s, interp_form)
    return norm(res), out


def run_routes(kz, s, groups, host_forms=HOST_FORMS, device_forms=DEVICE_FORMS, plain=True):
    """{route: (verdicts, [176 bytes per group] or None)} of one _many call per route"""
    n, G = groups[0].n, len(groups)
    assert all(g.n == n for g in groups)
    out = {}

    def timed(route, f):
        t0 = time.perf_counter()
        out[route] = f()
        print(f"{G} x {n} blobs, {route}: {time.perf_counter() - t0:.3f} s")
    for f in host_forms:
        timed(f"host call, interp_form {f}", lambda: host_call(kz, s, groups, f))
    d = to_device(groups) if device_forms or plain else None
    for i, p in device_forms:
        def dev():
            res, o = kz.Kzg.debug_blob_cell_batch_intermediates_device(*d, n, G, s, i, p)
            return norm(res), o
        timed(f"device call, interp_form {i}, prep_form {p}", dev)
    if plain:
        timed("verify_blob_cell_proofs_batch_many", lambda: (norm(kz.Kzg.verify_blob_cell_proofs_batch_many([g.args for g in groups], s)), None))
        timed("verify_blob_cell_proofs_batch_many_device", lambda: (norm(kz.Kzg.verify_blob_cell_proofs_batch_many_device(*d, n, G, s)), None))
    return out


def parts(o):
    return {"r": o[:32].hex(), "itau": o[32:80].hex(), "ll": o[80:128].hex(), "rl": o[128:176].hex()}


def same_as_cpu(route, groups, cpu, res, outs):
    """the verdict and all 176 bytes of every group are the CPU's; a group the CPU refuses is BadArgs and its bytes are unspecified"""
    assert len(res) == len(groups)
    for t, (g, w) in enumerate(zip(groups, cpu)):
        if w == "BadArgs":
            assert res[t] == "BadArgs", (route, g.name, res[t])
            continue
        if outs is not None:
            assert parts(outs[t]) == parts(w[0]), (route, g.name)
        assert res[t] is w[1], (route, g.name, res[t])


def check_exact(kz, s, want, groups, **routes):
    cpu = [want(g) for g in groups]
    got = run_routes(kz, s, groups, **routes)
    for route, (res, outs) in got.items():
        same_as_cpu(route, groups, cpu, res, outs)
    return got, cpu


# ---- 1. where a commitment sits among its group's unique ones
@pytest.mark.parametrize("which", sc.DEDUP)
def test_dedup_positions(kz, s1, pools, want, which):
    g = sc.dedup_group(pools, which)
    got, cpu = check_exact(kz, s1, want, [g])
    assert cpu[0][1] is True and len(got) == 9
    if which == "kinds":                                          # infinity among the commitments; the zero blob adds nothing to any sum
        assert g.c[1] == sc.INF and sc.INF not in (cpu[0][0][32:80], cpu[0][0][80:128], cpu[0][0][128:176])


# ---- 2. 6 | 7 blobs per launch set, and 256 | 384 cells per group (n = 2 | 3)
@pytest.mark.parametrize("n,groups", sc.LAUNCH_SETS)
def test_blobs_per_launch_set(kz, s1, pools, want, n, groups):
    gs = sc.launch_set_groups(pools, n, groups)
    assert len(gs) == groups and {g.kind for g in gs} == {"valid"}
    got, cpu = check_exact(kz, s1, want, gs)
    assert got["host call, interp_form 0"][0] == [True] * groups
    assert len({w[0] for w in cpu}) == groups                     # no two groups of the call are alike


# ---- 3. the last of seven distinct blobs spoiled: an ignored tail would answer True
@pytest.mark.parametrize("what", sc.SPOILS7)
def test_spoils_in_the_last_of_seven_blobs(kz, s1, pools, want, what):
    base, g = sc.distinct_group(pools, 7), sc.spoils_at_seven(pools)[what]
    got, cpu = check_exact(kz, s1, want, [g])
    if g.kind == "spoiled":
        assert cpu[0][1] is False and cpu[0][0] != want(base)[0]
        if what == "proofs":                                      # r changes with the transcript; [I(tau)]_1 with r alone
            assert cpu[0][0][:32] != want(base)[0][:32]
    else:
        assert cpu[0] == "BadArgs" and all(res == ["BadArgs"] for res, _ in got.values())


# ---- 4. 128 | 129 distinct blobs in one group
BIG_ROUTES = dict(host_forms=HOST_FORMS, device_forms=((0, 0), (0, 1)) + DEVICE_FORMS)


def test_128_blobs_the_last_group_the_device_hashes(kz, s1, big, want):
    g = big["128"]
    assert 128 * g.n == 16384
    got, cpu = check_exact(kz, s1, want, [g], host_forms=HOST_FORMS, device_forms=((0, 0), (0, 1), (0, 2)) + DEVICE_FORMS)
    assert cpu[0][1] is True and len(got) == 12


def test_129_blobs_the_first_group_the_host_must_hash(kz, s1, big, want):
    g = big["129"]
    assert 128 * g.n == 16512
    got, cpu = check_exact(kz, s1, want, [g], **BIG_ROUTES)
    assert cpu[0][1] is True and len(got) == 11


def test_129_blobs_with_two_proofs_of_the_last_exchanged(kz, s1, big, want):
    g, base = big["129-swapped"], big["129"]
    assert g.blobs == base.blobs and g.c == base.c and [t for t in range(len(g.p)) if g.p[t] != base.p[t]] == [128 * 128 + 126, 128 * 128 + 127]
    got, cpu = check_exact(kz, s1, want, [g], **BIG_ROUTES)
    assert cpu[0][1] is False and all(res == [False] for res, _ in got.values())
    assert cpu[0][0][:32] != want(base)[0][:32]


# ---- 5. a smaller call after the largest, on the same workspace: no buffer's stale tail is read
def test_shrinking_sizes_on_one_workspace(kz, s1, fx, oracle, pools, big, want):
    g129 = big["129"]
    for form in (1, 2):                                           # both interpolations leave their largest buffers behind
        res, out = host_call(kz, s1, [g129], form)
        same_as_cpu(f"129 blobs, interp_form {form}", [g129], [want(g129)], res, out)
    one, abac = sc.distinct_group(pools, 1, 14), sc.dedup_group(pools, "ABAC")
    for g in (one, abac):
        for form in HOST_FORMS:
            res, out = host_call(kz, s1, [g], form)
            same_as_cpu(f"after 129 blobs, interp_form {form}", [g], [want(g)], res, out)
    d = to_device([abac])
    for i, p in DEVICE_FORMS:
        res, out = kz.Kzg.debug_blob_cell_batch_intermediates_device(*d, 4, 1, s1, i, p)
        same_as_cpu(f"after 129 blobs, device call {i} {p}", [abac], [want(abac)], norm(res), out)
    # the calls that share the workspace
    cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(fx["blobs"][1], s1)
    assert [x.to_bytes() for x in cells] == fx["cells"][1] and [x.to_bytes() for x in proofs] == fx["P"][1]
    batch = dcases.batch(fx, [(0, 5), (1, 127), (1, 5), (2, 64), (0, 0)])
    ok, d = cs.verify_cell_kzg_proof_batch(oracle, *batch, mono=fx["mono"], g2=fx["g2"], intermediates=True)
    res, out = kz.Kzg.debug_cell_batch_intermediates([batch], s1)
    assert ok is True and norm(res) == [True] and out[0] == d["r"] + d["itau"] + d["ll"] + d["rl"]
    # and one route after the other on one group
    seven = sc.distinct_group(pools, 7)
    for form in (1, 2, 1):
        res, out = host_call(kz, s1, [seven], form)
        same_as_cpu(f"interp_form 1, 2, 1: {form}", [seven], [want(seven)], res, out)


# ---- 6. the device hash over the index array k_blob_meta writes, in both of its forms
def test_both_device_hash_kernels_over_the_written_index_array(kz, setup_bytes, pools, want):
    two = sc.launch_set_groups(pools, 2, 4)
    by_name = {g.name: g for g in two}
    repeat = by_name["two-AA"]
    assert repeat.distinct == 1 and repeat.c[0] == repeat.c[1]
    s = _load(kz, setup_bytes, None, KZG355_RHASH_LANES_FROM="3")
    try:
        for groups in ([repeat, by_name["distinct2@9"]], [by_name["two-mix-zero"], repeat, by_name["two-x64-mix"]]):      # k_cell_rhash_wave, _lanes
            d = to_device(groups)
            cpu = [want(g) for g in groups]
            for interp_form in HOST_FORMS:
                res, out = kz.Kzg.debug_blob_cell_batch_intermediates_device(*d, 2, len(groups), s, interp_form, 1)
                same_as_cpu(f"{len(groups)} groups, interp_form {interp_form}", groups, cpu, norm(res), out)
                assert norm(res) == [True] * len(groups)
    finally:
        s.free()


# ---- 7. one call of every kind: verdicts, statuses and bytes land on their own groups
def test_neighbours_in_one_call_of_seven_blob_groups(kz, s1, pools, want):
    spoils = sc.spoils_at_seven(pools)
    valid = [sc.distinct_group(pools, 7), sc.distinct_group(pools, 7, 7), sc.planned("seven-repeats", [pools.mix(t) for t in (3, 9, 1, 12, 0)],
                                                                                     [0, 0, 1, 2, 0, 3, 4])]
    groups = [valid[0], spoils["element"], spoils["element=r"], valid[1], spoils["proofs"], valid[2]]
    expect = [True, False, "BadArgs", True, False, True]
    got, cpu = check_exact(kz, s1, want, groups)
    for route, (res, _) in got.items():
        assert res == expect, route
    alone = [host_call(kz, s1, [g])[1][0] for g in valid]
    assert alone == [got["host call, interp_form 0"][1][t] for t in (0, 3, 5)] == [cpu[t][0] for t in (0, 3, 5)]
    G = len(groups)
    ok, st = (C.c_bool * G)(), (C.c_int * G)(*([7] * G))
    rc = kz.kzg.lib().kzg355_verify_blob_cell_proofs_batch_many(ok, st, b"".join(b"".join(g.blobs) for g in groups), b"".join(b"".join(g.c) for g in groups),
                                                                b"".join(b"".join(g.p) for g in groups), 7, G, s1.handle)
    assert rc == BADARGS and list(st) == [BADARGS if e == "BadArgs" else 0 for e in expect]
    assert [bool(x) for x in ok] == [e is True for e in expect]


# ---- 8. a handle over three replicas: uneven ranges of groups
def test_uneven_ranges_over_three_replicas(kz, setup_bytes, s1, pools, want):
    two = {g.name: g for g in sc.launch_set_groups(pools, 2, 4)}
    base = two["distinct2@9"]
    groups = [base, sc.malformed_element(base, 1, 4095), sc.spoil_swap_proofs(two["two-AA"], 1, 127, 126), two["two-x64-mix"], two["two-mix-zero"]]
    expect = [True, "BadArgs", False, True, True]
    cpu = [want(g) for g in groups]
    s3 = _load(kz, setup_bytes, [0, 0, 0])
    try:
        assert s3.device_count == 3
        for count in (5, 4):
            before = s3.cell_calls_per_device()
            for form in HOST_FORMS:
                res, out = host_call(kz, s3, groups[:count], form)
                assert res == expect[:count]
                same_as_cpu(f"three replicas, {count} groups, interp_form {form}", groups[:count], cpu[:count], res, out)
                single = host_call(kz, s1, groups[:count], form)
                assert res == single[0] and [o for o, e in zip(out, expect) if e != "BadArgs"] == [o for o, e in zip(single[1], expect) if e != "BadArgs"]
            assert norm(kz.Kzg.verify_blob_cell_proofs_batch_many([g.args for g in groups[:count]], s3)) == expect[:count]
            moved = [a - b for a, b in zip(s3.cell_calls_per_device(), before)]
            assert moved == [4, 4, 4], moved                              # four calls, one launch set on every replica in each
    finally:
        s3.free()


# ---- 9. four different first calls on a fresh handle at once: ensure_cc_consts and ensure_cell_setup under contention (one run, no loop)
def test_concurrent_first_calls_on_a_fresh_handle(kz, setup_bytes, fx, oracle, pools, want):
    g = sc.distinct_group(pools, 2, 9)
    cpu = want(g)
    batch = dcases.batch(fx, [(0, 5), (1, 127), (1, 5), (2, 64), (0, 0)])
    ix = list(range(0, 128, 2))
    s = _load(kz, setup_bytes, None)
    gate, got = threading.Barrier(4), {}

    def run(name, f):
        try:
            gate.wait()
            got[name] = f()
        except Exception as e:                                   # reported below, in the main thread
            got[name] = e
    work = {"blob": lambda: host_call(kz, s, [g]), "compute": lambda: kz.Kzg.compute_cells_and_kzg_proofs(fx["blobs"][2], s),
            "verify": lambda: kz.Kzg.verify_cell_kzg_proof_batch(*batch, s), "recover": lambda: kz.Kzg.recover_cells_and_kzg_proofs(
                ix, [fx["cells"][0][k] for k in ix], s)}
    try:
        threads = [threading.Thread(target=run, args=item) for item in work.items()]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert set(got) == set(work) and not [v for v in got.values() if isinstance(v, Exception)], got
        assert got["blob"][0] == [True] and got["blob"][1][0] == cpu[0] and cpu[1] is True
        assert [x.to_bytes() for x in got["compute"][0]] == fx["cells"][2] and [x.to_bytes() for x in got["compute"][1]] == fx["P"][2]
        assert got["verify"] is True
        assert [x.to_bytes() for x in got["recover"][0]] == fx["cells"][0] and [x.to_bytes() for x in got["recover"][1]] == fx["P"][0]
    finally:
        s.free()
