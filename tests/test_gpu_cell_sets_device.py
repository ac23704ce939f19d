"""-m gpu: verify_cell_kzg_proof_batch_many_sets_device -- groups of different sizes whose four arrays lie in HBM -- against the CPU
(tests/cell_sets_cases.py and tests/cell_sets_device_cases.py).  Every call runs with the preparation pinned to the device (prep_form 1:
k_cell_prep_sets, k_cell_rhash_*_sets) and to the host (prep_form 2: the arrays copied back), and the counter of device preparations must move by 1
and by 0.  Every comparison is of the debug form's 176 bytes r | [I(tau)]_1 | LL | RL and the verdict, per group, byte for byte, with the CPU's
for that group alone, and with the host `_sets` call on the same handle: a dedup that crosses a border, a table, an offset or a segment slot
taken from a neighbour changes r or [I(tau)]_1, and a changed r still verifies a valid batch, so no test asks for True alone.  Groups above 4096
cells are compared with the CPU in r and [I(tau)]_1 and with the host call in all 176 bytes.  There is no tolerance anywhere."""
import ctypes as C
import json
import os

import pytest

import cell_batch_cases as bc
import cell_device_cases as dcases
import cell_sets_cases as sets
import cell_sets_device_cases as sd

pytestmark = pytest.mark.gpu

BADARGS = 1
VERIFY, DEBUG = "kzg355_verify_cell_kzg_proof_batch_many_sets_device", "kzg355_debug_cell_batch_intermediates_sets_device"


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


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
def fx():
    return bc.fixture()


@pytest.fixture(scope="module")
def pools(oracle, fx):
    return bc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def want(oracle, fx):
    """the CPU's answer per group (cell_sets_device_cases.cpu_answer), computed once per group name and shared by the tests of this module"""
    reference, known = bc.Reference(oracle, fx), {}

    def get(g):
        if g.name not in known:
            known[g.name] = g.args, sd.cpu_answer(reference, g)
        args, answer = known[g.name]
        assert args == g.args, f"two different groups are called {g.name}"
        return answer
    return get


@pytest.fixture(scope="module")
def status_calls(pools, oracle):
    calls = sets.status_calls(pools, dcases.not_in_subgroup(oracle), dcases.off_curve(oracle))
    assert len(calls) == 10
    return calls


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def parts(o):
    return {"r": o[:32].hex(), "itau": o[32:80].hex(), "ll": o[80:128].hex(), "rl": o[128:176].hex()}


def counters(s):
    return s.cell_calls_per_device(), s.cell_device_prep_calls


def device_call(kz, s, d, counts, form):
    """one debug call on device arrays: (verdicts, 176 bytes per group, device preparations counted)"""
    before = s.cell_device_prep_calls
    res, outs = kz.Kzg.debug_cell_batch_intermediates_sets_device(*d, counts, s, prep_form=form)
    return norm(res), outs, s.cell_device_prep_calls - before


def check_call(kz, torch, s, want, call, device_prepares=True):
    """prep_form 1 and 2: every group's verdict and bytes are the CPU's for that group alone and the host `_sets` call's on the same handle; the
    device preparation is counted once under prep_form 1 (not at all when the call has a group above its cap) and never under prep_form 2"""
    sets.check_call(call)
    cpu = [want(g) for g in call.groups]
    host_res, host_outs = kz.Kzg.debug_cell_batch_intermediates_sets([g.args for g in call.groups], s)
    host_res = norm(host_res)
    d = sd.to_device(torch, call.groups)
    kept = [x.clone() for x in d]
    for form in (1, 2):
        res, outs, prepared = device_call(kz, s, d, call.counts, form)
        assert prepared == (1 if form == 1 and device_prepares else 0), (call.name, form)
        for t, (g, (verdict, raw, upto)) in enumerate(zip(call.groups, cpu)):
            if verdict == "BadArgs":
                assert res[t] == "BadArgs", (call.name, form, t, g.name, res[t])
                continue
            assert res[t] is verdict if verdict is not None else res[t] in (True, False), (call.name, form, t, g.name, res[t], verdict)
            assert parts(outs[t][:upto]) == parts(raw[:upto]), (call.name, form, t, g.name)
        assert (res, outs) == (host_res, host_outs), (call.name, form)
    assert all(torch.equal(a, b) for a, b in zip(d, kept)), "a device-resident input was written"
    # the verify form: the same verdicts, whatever route it chose
    assert norm(kz.Kzg.verify_cell_kzg_proof_batch_many_sets_device(*d, call.counts, s)) == host_res, call.name
    return host_res, host_outs, d


def raw_call(kz, s, d, counts, form=None, G=None):
    """through ctypes, with a debug buffer pre-filled with 0x55, verdicts with True and statuses with 7: (return value, verdicts, statuses[, 176 bytes
    per group]); counts None (with G): a NULL count array"""
    G = len(counts) if counts is not None else G
    ok, st = (C.c_bool * max(G, 1))(*([True] * max(G, 1))), (C.c_int * max(G, 1))(*([7] * max(G, 1)))
    cnt = (C.c_size_t * max(G, 1))(*counts) if counts is not None else None
    ptrs = [x if isinstance(x, int) or x is None else x.data_ptr() for x in d]
    lib = kz.kzg.lib()
    if form is None:
        return getattr(lib, VERIFY)(ok, st, cnt, *ptrs, G, s.handle), [bool(x) for x in ok][:G], list(st)[:G]
    out = C.create_string_buffer(b"\x55" * (176 * max(G, 1)))
    rc = getattr(lib, DEBUG)(out, ok, st, cnt, *ptrs, G, form, s.handle)
    return rc, [bool(x) for x in ok][:G], list(st)[:G], [out.raw[176 * t:176 * t + 176] for t in range(G)]


# ---- 1. sizes side by side: empties inside, the 256-thread stride, offsets behind empty groups; outputs fully written; prep_form 0
def test_sizes_side_by_side(kz, torch, s1, pools, want):
    call = sets.side_by_side(pools)
    before = s1.cell_calls_per_device()
    res, outs, d = check_call(kz, torch, s1, want, call)
    assert [a - b for a, b in zip(s1.cell_calls_per_device(), before)] == [4], "one launch set per call: the host one and three device ones"
    assert res == [True] * 9 and outs[2] == outs[6] == outs[7] == sets.ZERO_DEBUG
    # the route chosen by shape gives the same bytes
    res0, outs0, _ = device_call(kz, s1, d, call.counts, 0)
    assert (res0, outs0) == (res, outs)
    # every output byte and every status is written, on both routes and in both forms
    for form in (1, 2):
        assert raw_call(kz, s1, d, call.counts, form) == (0, [True] * 9, [0] * 9, outs), form
    assert raw_call(kz, s1, d, call.counts) == (0, [True] * 9, [0] * 9)


# ---- 2. empty at the ends, nothing but empty groups, no groups
def test_empty_at_the_ends_and_calls_without_a_cell(kz, torch, s1, pools, want):
    res, outs, _ = check_call(kz, torch, s1, want, sets.empty_ends(pools))
    assert res == [True] * 3 and outs[0] == outs[2] == sets.ZERO_DEBUG and outs[1] != sets.ZERO_DEBUG
    before = counters(s1)
    none = (None,) * 4
    for form in (0, 1, 2):
        assert kz.Kzg.debug_cell_batch_intermediates_sets_device(*none, [0, 0, 0], s1, prep_form=form) == ([True] * 3, [sets.ZERO_DEBUG] * 3)
        assert raw_call(kz, s1, none, [0, 0, 0], form) == (0, [True] * 3, [0] * 3, [sets.ZERO_DEBUG] * 3)
        assert raw_call(kz, s1, none, [], form) == (0, [], [], [])
    assert kz.Kzg.verify_cell_kzg_proof_batch_many_sets_device(*none, [0, 0, 0], s1) == [True] * 3
    assert kz.Kzg.verify_cell_kzg_proof_batch_many_sets_device(*none, [], s1) == []
    assert kz.Kzg.debug_cell_batch_intermediates_sets_device(*none, [], s1) == ([], [])
    assert counters(s1) == before, "a call without a cell launches nothing"


# ---- 3. borders: a commitment or a column shared across a group border must not merge
def test_borders(kz, torch, s1, pools, want):
    res, _, _ = check_call(kz, torch, s1, want, sets.borders(pools))
    assert res == [True] * 6


# ---- 4. more workgroups than one block of the per-group kernels
def test_many_small_groups(kz, torch, s1, pools, want):
    call = sets.many_small(pools)
    assert len(call.groups) == 70 and call.counts.count(0) == 17
    res, outs, _ = check_call(kz, torch, s1, want, call)
    assert res == [True] * 70
    assert [o == sets.ZERO_DEBUG for o in outs] == [n == 0 for n in call.counts]


# ---- 5. statuses by position: on the device route the index error is the kernel's error word, at the group's number after renumbering
@pytest.mark.parametrize("k", range(10))
def test_statuses_by_position(kz, torch, s1, want, status_calls, k):
    call = status_calls[k]
    res, _, d = check_call(kz, torch, s1, want, call)
    at = [t for t, how in call.spoiled.items() if how == "malformed"]
    assert len(at) == 1 and [t for t, v in enumerate(res) if v == "BadArgs"] == at, call.name
    assert [v for t, v in enumerate(res) if t not in call.spoiled] == [True] * (5 - len(call.spoiled)), call.name
    assert res.count(False) == sum(how == "spoiled" for how in call.spoiled.values()), call.name
    st = [BADARGS if v == "BadArgs" else 0 for v in res]
    for form in (1, 2):
        rc, ok, got, _ = raw_call(kz, s1, d, call.counts, form)
        assert (rc, ok, got) == (BADARGS, [v is True for v in res], st), (call.name, form)


def test_an_index_error_behind_empty_groups(kz, torch, s1, pools, want):
    """the malformed group is number 1 of the launch set and number 4 of the call"""
    pair = sets.two_groups(pools)
    groups = [sets.empty("q0"), pair.groups[0], sets.empty("q1"), sets.empty("q2"), bc.malformed_index(pair.groups[1], 6), sets.empty("q3")]
    call = sets.Call("index-behind-empties", groups, [0, 4, 0, 0, 7, 0], spoiled={4: "malformed"})
    res, _, _ = check_call(kz, torch, s1, want, call)
    assert res == [True, True, True, True, "BadArgs", True]


# ---- 6. sizes only the preparation kernel sees
def test_the_second_sort_tile(kz, torch, s1, pools, want):
    res, _, _ = check_call(kz, torch, s1, want, sd.sized(pools, "sort-tiles", sd.SORT_TILES))
    assert res == [False, False, True]


def test_an_lds_table_an_hbm_table_and_a_tiny_group(kz, torch, s1, pools, want):
    res, _, _ = check_call(kz, torch, s1, want, sd.sized(pools, "tables", sd.TABLES))
    assert res == [False, False, True]


def test_a_group_above_the_cap_sends_the_call_to_the_host_preparation(kz, torch, s1, pools, want):
    res, _, _ = check_call(kz, torch, s1, want, sd.sized(pools, "over-the-cap", sd.OVER_THE_CAP), device_prepares=False)
    assert res == [False, True]


# ---- 7. both transcript kernels on groups of different lengths
def test_both_hash_kernels(kz, torch, setup_bytes, pools, want):
    s = _load(kz, setup_bytes, None, KZG355_RHASH_LANES_FROM="3")
    try:
        for call in sd.hash_calls(pools):                         # k_cell_rhash_wave_sets, then k_cell_rhash_lanes_sets
            assert len(set(call.counts)) == len(call.counts) in (2, 3)
            res, _, _ = check_call(kz, torch, s, want, call)
            assert res == [True] * len(call.counts)
    finally:
        s.free()


# ---- 8. refusals of the call as a whole
def test_refusals_on_a_live_handle(kz, torch, s1, pools, setup_bytes):
    call = sets.two_groups(pools)
    good = sd.to_device(torch, call.groups)
    before = counters(s1)

    def refused(s, d, counts):
        for form in (None, 0, 1, 2):
            got = raw_call(kz, s, d, counts, form, G=2)
            assert got[:3] == (BADARGS, [False] * 2, [BADARGS] * 2), (counts, form, got[:3])
    # a bulk pointer 8 bytes off a 16-byte boundary; an index pointer 4 bytes off an 8-byte one
    shifted = sd.to_device(torch, call.groups, shift=8)
    assert shifted[0].data_ptr() % 16 == 8 and torch.equal(shifted[0], good[0])
    refused(s1, shifted, call.counts)
    refused(s1, (good[0], good[1].data_ptr() + 4, good[2], good[3]), call.counts)
    assert norm(kz.Kzg.verify_cell_kzg_proof_batch_many_sets_device(*shifted, call.counts, s1)) == ["BadArgs"] * 2       # every status is marked
    # counts that sum above 2^18 or overflow (the arrays are never read), NULL counts
    for counts in ([1 << 18, 1], [1 << 63, 1 << 63], [(1 << 64) - 1, 2], [0, (1 << 18) + 1]):
        refused(s1, good, counts)
    refused(s1, good, None)
    assert counters(s1) == before, "a refused call counts nowhere"
    # a handle of the minimal preset
    from kzg_rust_amd import kzg_minimal as km
    mfx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        refused(sm, good, call.counts)
    finally:
        sm.free()
    # and the arrays still verify
    assert raw_call(kz, s1, good, call.counts) == (0, [True, True], [0, 0])


# ---- 9. a handle over several replicas: the call runs on the first device alone
def test_several_replicas(kz, torch, s1, setup_bytes, pools, want):
    s3 = _load(kz, setup_bytes, [0, 0, 0])
    try:
        assert s3.device_count == 3
        call = sets.side_by_side(pools)
        d = sd.to_device(torch, call.groups)
        for form in (1, 2):
            before = s3.cell_calls_per_device()
            got = device_call(kz, s3, d, call.counts, form)
            assert [a - b for a, b in zip(s3.cell_calls_per_device(), before)] == [1, 0, 0], form
            assert got == device_call(kz, s1, d, call.counts, form)
            assert got[0] == [True] * 9 and got[1] == [want(g)[1] for g in call.groups]
        before = s3.cell_calls_per_device()
        assert raw_call(kz, s3, d, call.counts) == (0, [True] * 9, [0] * 9)
        assert [a - b for a, b in zip(s3.cell_calls_per_device(), before)] == [1, 0, 0]
    finally:
        s3.free()
