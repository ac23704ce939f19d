"""-m gpu: verify_cell_kzg_proof_batch_many_sets -- groups of different sizes in one set of launches -- against the CPU (tests/cell_sets_cases.py,
whose calls and answers tests/test_cell_sets_cases.py pins to tests/cell_spec.py without a GPU).  The contract is that group g's result is exactly
that of verify_cell_kzg_proof_batch on its slice, so every comparison is of the debug form's 176 bytes r | [I(tau)]_1 | LL | RL and the verdict,
per group, byte for byte, with the CPU's for that group alone: a dedup that crosses a border, a group's offset, its term base or its error word
taken from a neighbour changes r or lands a status on the wrong group, and a changed r still verifies a valid batch, so no test asks for True
alone.  There is no tolerance anywhere."""
import ctypes as C
import json
import os

import pytest

import cell_batch_cases as bc
import cell_device_cases as dcases
import cell_sets_cases as sets

pytestmark = pytest.mark.gpu

BADARGS = 1


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, devices, **env):
    g1, g2 = setup_bytes
    env = dict(env, KZG355_MSM="bucket", KZG355_EXCHANGE="peer")          # no wide table per replica
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
def s3(kz, setup_bytes):
    s = _load(kz, setup_bytes, [0, 0, 0])
    assert s.device_count == 3
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    return bc.fixture()


@pytest.fixture(scope="module")
def pools(oracle, fx):
    return bc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def want(oracle, fx):
    """the CPU's answer per group (verdict or "BadArgs", 176 bytes or None), computed once per group name and shared by the tests of this module"""
    reference, known = bc.Reference(oracle, fx), {}

    def get(g):
        if g.name not in known:
            known[g.name] = g.args, sets.cpu_answer(reference, g)
        args, answer = known[g.name]
        assert args == g.args, f"two different groups are called {g.name}"
        return answer
    return get


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def parts(o):
    return {"r": o[:32].hex(), "itau": o[32:80].hex(), "ll": o[80:128].hex(), "rl": o[128:176].hex()}


def moved(s, before):
    return [a - b for a, b in zip(s.cell_calls_per_device(), before)]


def raw_sets(kz, s, groups, debug=False):
    """the _sets call through ctypes: (return value, verdicts, statuses[, 176 bytes per group])"""
    G = len(groups)
    ok, st = (C.c_bool * max(G, 1))(), (C.c_int * max(G, 1))(*([7] * max(G, 1)))
    counts = (C.c_size_t * max(G, 1))(*[g.n for g in groups])
    flat = [int(i) for g in groups for i in g.i]
    idx = (C.c_size_t * max(len(flat), 1))(*flat)
    args = (ok, st, counts, b"".join(b"".join(g.c) for g in groups), idx, b"".join(b"".join(g.cells) for g in groups),
            b"".join(b"".join(g.p) for g in groups), G, s.handle)
    if not debug:
        return kz.kzg.lib().kzg355_verify_cell_kzg_proof_batch_many_sets(*args), [bool(x) for x in ok][:G], list(st)[:G]
    out = C.create_string_buffer(b"\x55" * (176 * max(G, 1)))
    rc = kz.kzg.lib().kzg355_debug_cell_batch_intermediates_sets(out, *args)
    return rc, [bool(x) for x in ok][:G], list(st)[:G], [out.raw[176 * t:176 * t + 176] for t in range(G)]


def check_call(kz, s, want, call):
    """one debug _sets call: every group's verdict and 176 bytes are the CPU's for that group; a group the CPU refuses is BadArgs, alone"""
    sets.check_call(call)
    cpu = [want(g) for g in call.groups]
    res, outs = kz.Kzg.debug_cell_batch_intermediates_sets([g.args for g in call.groups], s)
    res = norm(res)
    for t, (g, (verdict, raw)) in enumerate(zip(call.groups, cpu)):
        assert res[t] == verdict if verdict == "BadArgs" else res[t] is verdict, (call.name, t, g.name, res[t], verdict)
        if raw is not None:
            assert parts(outs[t]) == parts(raw), (call.name, t, g.name)
    assert [v for v, _ in cpu] == [{"malformed": "BadArgs", "spoiled": False}.get(call.spoiled.get(t), True) for t in range(len(cpu))], call.name
    # the verify form: the same verdicts and statuses, and the return value is the first non-OK status in group order
    rc, ok, st = raw_sets(kz, s, call.groups)
    assert st == [BADARGS if v == "BadArgs" else 0 for v in res] and ok == [v is True for v in res], call.name
    assert rc == next((x for x in st if x), 0), call.name
    return res, outs


# ---- 1. sizes side by side
def test_sizes_side_by_side(kz, s1, pools, want):
    call = sets.side_by_side(pools)
    before = s1.cell_calls_per_device()
    res, outs = check_call(kz, s1, want, call)
    assert moved(s1, before) == [2], "one launch set per call, the debug and the verify one"
    assert res == [True] * 9
    assert outs[2] == outs[6] == outs[7] == sets.ZERO_DEBUG
    # every non-empty group alone through the uniform call: the same bytes
    for t, g in enumerate(call.groups):
        if g.n:
            alone, o = kz.Kzg.debug_cell_batch_intermediates([g.args], s1)
            assert (alone, o) == ([True], [outs[t]]), (t, g.name)


# ---- 2. empty at the ends, nothing but empty groups, no groups
def test_empty_at_the_ends(kz, s1, pools, want):
    res, outs = check_call(kz, s1, want, sets.empty_ends(pools))
    assert res == [True] * 3 and outs[0] == outs[2] == sets.ZERO_DEBUG and outs[1] != sets.ZERO_DEBUG
    before = s1.cell_calls_per_device()
    empty = sets.all_empty()
    assert raw_sets(kz, s1, empty.groups, debug=True) == (0, [True] * 3, [0] * 3, [sets.ZERO_DEBUG] * 3)
    assert raw_sets(kz, s1, empty.groups) == (0, [True] * 3, [0] * 3)
    assert raw_sets(kz, s1, []) == (0, [], []) and raw_sets(kz, s1, [], debug=True) == (0, [], [], [])
    assert kz.Kzg.debug_cell_batch_intermediates_sets([], s1) == ([], [])
    assert kz.Kzg.verify_cell_kzg_proof_batch_many_sets([g.args for g in empty.groups], s1) == [True] * 3
    assert moved(s1, before) == [0], "a call without a cell launches nothing"


# ---- 3. borders
def test_borders(kz, s1, pools, want):
    res, _ = check_call(kz, s1, want, sets.borders(pools))
    assert res == [True] * 6


# ---- 4. statuses by position, error words at a border
def test_statuses_by_position(kz, s1, pools, want, oracle):
    calls = sets.status_calls(pools, dcases.not_in_subgroup(oracle), dcases.off_curve(oracle))
    assert len(calls) == 10
    n_false = 0
    for call in calls:
        res, _ = check_call(kz, s1, want, call)
        at = [t for t, how in call.spoiled.items() if how == "malformed"]
        assert len(at) == 1 and [t for t, v in enumerate(res) if v == "BadArgs"] == at, call.name
        n_false += res.count(False)
        assert [v for t, v in enumerate(res) if t not in call.spoiled] == [True] * (5 - len(call.spoiled)), call.name
    assert n_false == 2                                           # the well-formed False groups between True ones


# ---- 5. uniform through the new call
def test_uniform_through_the_new_call(kz, s1, pools, want):
    call = sets.uniform(pools)
    res, outs = check_call(kz, s1, want, call)
    assert (res, outs) == kz.Kzg.debug_cell_batch_intermediates([g.args for g in call.groups], s1)
    assert res == [True] * 4


# ---- 6. more groups than one block of the per-group kernels
def test_many_small_groups(kz, s1, pools, want):
    call = sets.many_small(pools)
    assert len(call.groups) == 70 and call.counts.count(0) == 17
    res, outs = check_call(kz, s1, want, call)
    assert res == [True] * 70
    assert [o == sets.ZERO_DEBUG for o in outs] == [n == 0 for n in call.counts]


# ---- 7. several replicas
def test_several_replicas(kz, s1, s3, pools, want):
    call = sets.side_by_side(pools)
    args = [g.args for g in call.groups]
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()
    got3 = kz.Kzg.debug_cell_batch_intermediates_sets(args, s3)
    assert moved(s3, before) == [1, 1, 1], "six non-empty groups in three ranges: every replica runs one launch set"
    assert got3 == kz.Kzg.debug_cell_batch_intermediates_sets(args, s1)
    assert got3[0] == [True] * 9 and got3[1] == [want(g)[1] for g in call.groups]
    assert raw_sets(kz, s3, call.groups) == raw_sets(kz, s1, call.groups) == (0, [True] * 9, [0] * 9)
    # two non-empty groups use two replicas, wherever the empty ones stand
    pair = sets.two_groups(pools)
    padded = [sets.empty("p0"), pair.groups[0], sets.empty("p1"), sets.empty("p2"), pair.groups[1], sets.empty("p3")]
    before = s3.cell_calls_per_device()
    rc, ok, st, outs = raw_sets(kz, s3, padded, debug=True)
    assert moved(s3, before) == [1, 1, 0]
    assert (rc, ok, st) == (0, [True] * 6, [0] * 6) and outs == [want(g)[1] for g in padded]
    # a status keeps its place over the replicas
    bad = [pair.groups[0], sets.empty("p4"), bc.malformed_index(pair.groups[1], 3), call.groups[8]]
    assert raw_sets(kz, s3, bad) == raw_sets(kz, s1, bad) == (BADARGS, [True, True, False, True], [0, 0, BADARGS, 0])
    assert s3.exchange_stats() == ex, "nothing is cut, nothing is exchanged"


# ---- 8. refusals on a live handle
def test_refusals_on_a_live_handle(kz, s1, setup_bytes):
    lib = kz.kzg.lib()
    few = bytes(16)                                               # never read: the counts alone refuse the call
    idx = (C.c_size_t * 2)(0, 1)
    before = s1.cell_calls_per_device()
    for counts in ([1 << 18, 1], [1 << 63, 1 << 63], [(1 << 64) - 1, 2], [0, (1 << 18) + 1]):
        ok, st = (C.c_bool * 2)(True, True), (C.c_int * 2)(7, 7)
        cnt = (C.c_size_t * 2)(*counts)
        assert lib.kzg355_verify_cell_kzg_proof_batch_many_sets(ok, st, cnt, few, idx, few, few, 2, s1.handle) == BADARGS, counts
        assert list(st) == [BADARGS] * 2 and list(ok) == [False] * 2, counts
        out = C.create_string_buffer(2 * 176)
        st = (C.c_int * 2)(7, 7)
        assert lib.kzg355_debug_cell_batch_intermediates_sets(out, ok, st, cnt, few, idx, few, few, 2, s1.handle) == BADARGS and list(st) == [BADARGS] * 2
    # a NULL array while there are cells, NULL counts
    ok, st, cnt = (C.c_bool * 2)(True, True), (C.c_int * 2)(7, 7), (C.c_size_t * 2)(1, 1)
    assert lib.kzg355_verify_cell_kzg_proof_batch_many_sets(ok, st, cnt, few, idx, None, few, 2, s1.handle) == BADARGS and list(st) == [BADARGS] * 2
    st = (C.c_int * 2)(7, 7)
    assert lib.kzg355_verify_cell_kzg_proof_batch_many_sets(ok, st, None, few, idx, few, few, 2, s1.handle) == BADARGS and list(st) == [BADARGS] * 2
    assert moved(s1, before) == [0]
    # a handle of the minimal preset
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        ok, st = (C.c_bool * 2)(True, True), (C.c_int * 2)(7, 7)
        assert lib.kzg355_verify_cell_kzg_proof_batch_many_sets(ok, st, cnt, few, idx, few, few, 2, sm.handle) == BADARGS
        assert list(st) == [BADARGS] * 2 and list(ok) == [False] * 2
    finally:
        sm.free()
