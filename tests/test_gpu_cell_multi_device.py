"""-m gpu: the EIP-7594 cell calls on a handle over several devices (include/kzg355.h, "EIP-7594 cell proofs"; DESIGN.md sections 8 and 11).  A GPU
box has one card, so the replicas share it, as in tests/test_gpu_multi_device.py: what is exercised is the orchestration -- ranges of groups and
blobs per replica, statuses by position, the cut of a group into blocks of cells with ragged blocks, the first exponent of a block, the
per-block dedup and column sort, the exchange of the three sums, k_cell_merge and the status merge.  Every comparison is byte for byte: against
the same call on a single-device handle and, where the fixtures have it, against the CPU (cell_batch_cases.Reference, tests/golden/cells.json).
kzg355_settings_cell_calls_per_device and the exchange counter say which route a call took."""
import ctypes as C
import os
import random

import pytest

import cell_batch_cases as bc
import cell_device_cases as dcases
import cell_shard_cases as sc
import cell_spec as cs

pytestmark = pytest.mark.gpu

BADARGS = 1
ROW = 128 * 2048


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
    assert s.device_count == 3 and s.exchange_stats()[0] == 0
    yield s
    s.free()


@pytest.fixture(scope="module")
def s2(kz, setup_bytes):
    """two replicas: everything that needs the proof setup (384 MiB per replica)"""
    s = _load(kz, setup_bytes, [0, 0])
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    return bc.fixture()


@pytest.fixture(scope="module")
def pools(oracle, fx):
    return bc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def reference(oracle, fx):
    return bc.Reference(oracle, fx)


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def raw_verify(kz, s, groups):
    """kzg355_verify_cell_kzg_proof_batch_many through ctypes: (return value, verdicts, statuses)"""
    G, npg = len(groups), groups[0].n
    ok, st = (C.c_bool * G)(), (C.c_int * G)(*([7] * G))
    idx = (C.c_size_t * (G * npg))(*[int(i) for g in groups for i in g.i])
    rc = kz.kzg.lib().kzg355_verify_cell_kzg_proof_batch_many(ok, st, b"".join(b"".join(g.c) for g in groups), idx, b"".join(b"".join(g.cells) for g in groups),
                                                              b"".join(b"".join(g.p) for g in groups), npg, G, s.handle)
    return rc, [bool(x) for x in ok], list(st)


def moved(s, before):
    return [a - b for a, b in zip(s.cell_calls_per_device(), before)]


def cpu_parts(reference, g):
    r, itau, ll, rl, ok = reference(*g.args)
    return r + itau + ll + rl, ok


def triple(pools, first, name):
    return bc.planned(name, pools.mixed, [first, first + 1, first + 2])


# ------------------------------------------------------------------------------------------------ 1, 2: ranges of groups
def test_groups_fan_out_over_three_replicas(kz, s1, s3, pools, reference):
    groups = [triple(pools, 3 * t, f"fan{t}") for t in range(5)]
    groups[1] = sc.swap_proofs(groups[1], 0, 1)
    groups[3] = bc.malformed_index(groups[3], 1)
    groups[4] = sc.with_item(groups[4], 2, "malformed", cell=sc.noncanonical(groups[4].cells[2]))
    assert len(s1.cell_calls_per_device()) == 1 and s1.device_count == 1
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()[1:]
    rc, ok, st = raw_verify(kz, s3, groups)
    assert moved(s3, before) == [1, 1, 1], "ranges of 1, 2 and 2 groups: every replica runs one launch set"
    assert s3.exchange_stats()[1:] == ex
    assert st == [0, 0, 0, BADARGS, BADARGS] and ok == [True, False, True, False, False]
    assert rc == st[3], "the return value is the first non-OK status in group order"
    assert (rc, ok, st) == raw_verify(kz, s1, groups)
    for g, verdict in zip(groups[:3], ok[:3]):                     # the CPU's verdicts
        assert cpu_parts(reference, g)[1] is verdict, g.name
    # the debug form takes the same route and keeps its positions
    res3, out3 = kz.Kzg.debug_cell_batch_intermediates([g.args for g in groups], s3)
    res1, out1 = kz.Kzg.debug_cell_batch_intermediates([g.args for g in groups], s1)
    assert norm(res3) == norm(res1) == [True, False, True, "BadArgs", "BadArgs"]
    assert out3[:3] == out1[:3] == [cpu_parts(reference, g)[0] for g in groups[:3]]


def test_fewer_groups_than_replicas_too_small_to_cut(kz, s1, s3, pools):
    groups = [triple(pools, 20, "few0"), sc.swap_proofs(triple(pools, 23, "few1"), 0, 2)]
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()
    assert raw_verify(kz, s3, groups) == raw_verify(kz, s1, groups) == (0, [True, False], [0, 0])
    assert moved(s3, before) == [1, 1, 0], "a call uses as many replicas as it has groups"
    g = groups[0]
    assert kz.Kzg.verify_cell_kzg_proof_batch(*g.args, s3) is True and kz.Kzg.verify_cell_kzg_proof_batch(*groups[1].args, s3) is False
    assert moved(s3, before) == [3, 1, 0]
    empty = ([], [], [], [])
    assert kz.Kzg.verify_cell_kzg_proof_batch_many([empty, empty], s3) == [True, True]
    assert kz.Kzg.verify_cell_kzg_proof_batch(*empty, s3) is True
    L = kz.kzg.lib()
    ok, st = (C.c_bool * 1)(), (C.c_int * 1)(7)
    idx = (C.c_size_t * 3)(*g.i)
    assert L.kzg355_verify_cell_kzg_proof_batch_many(ok, st, b"".join(g.c), idx, b"".join(g.cells), b"".join(g.p), 3, 0, s3.handle) == 0 and st[0] == 7
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_cell_kzg_proof_batch(g.c, g.i[:2], g.cells, g.p, s3)
    assert moved(s3, before) == [3, 1, 0] and s3.exchange_stats() == ex


# ------------------------------------------------------------------------------------------------ 3, 4: one group over all replicas
def sharded_equals_single(kz, s1, sN, groups, reference=None):
    """one debug call per handle: the cut call makes exactly one exchange and returns the single-device handle's verdicts and 176 bytes"""
    before, ex = sN.cell_calls_per_device(), sN.exchange_stats()[2]
    resN, outN = kz.Kzg.debug_cell_batch_intermediates([g.args for g in groups], sN)
    assert sN.exchange_stats()[2] == ex + 1, "the call was not cut over the replicas"
    assert moved(sN, before) == [1] * sN.device_count, "every replica runs one block"
    res1, out1 = kz.Kzg.debug_cell_batch_intermediates([g.args for g in groups], s1)
    assert norm(resN) == norm(res1)
    for t, g in enumerate(groups):
        if res1[t] in (True, False):
            assert outN[t] == out1[t], g.name
            if reference is not None:
                assert (outN[t], resN[t]) == cpu_parts(reference, g), g.name
    return norm(resN), outN


@pytest.mark.parametrize("shape", ["7", "6", "8+8"])
def test_a_group_cut_over_three_replicas(kz, oracle, fx, s1, s3, reference, shape):
    groups = [sc.cut_group(oracle, fx, int(n), v) for v, n in enumerate(shape.split("+"))]
    for g in groups:
        bc.check_claims(g)
        sc.check_cut(g, 3)
    res, _ = sharded_equals_single(kz, s1, s3, groups, reference)
    assert res == [True] * len(groups)
    ex = s3.exchange_stats()[2]
    assert raw_verify(kz, s3, groups) == (0, [True] * len(groups), [0] * len(groups)) and s3.exchange_stats()[2] == ex + 1


def test_a_cut_group_that_is_wrong(kz, oracle, fx, s1, s3, reference):
    g = sc.cut_group(oracle, fx, 7)                               # blocks: cells 0-1, 2-3, 4-6
    res, _ = sharded_equals_single(kz, s1, s3, [sc.swap_proofs(g, 0, 6)], reference)
    assert res == [False]
    bad_point = dcases.not_in_subgroup(oracle)
    assert oracle.g1_uncompress_only(bad_point) == 0 and oracle.g1_validate(bad_point) != 0
    for bad in (bc.malformed_index(g, 3),                                                        # block 1
                sc.with_item(g, 6, "malformed", proof=bad_point),                                # the last block
                sc.with_item(g, 0, "malformed", cell=sc.noncanonical(g.cells[0]))):              # block 0
        ex = s3.exchange_stats()[2]
        assert raw_verify(kz, s3, [bad]) == raw_verify(kz, s1, [bad]) == (BADARGS, [False], [BADARGS]), bad.name
        assert s3.exchange_stats()[2] == ex + 1, bad.name
    # an Err in one group of a cut call leaves the other group's answer alone
    pair = [bc.malformed_index(sc.cut_group(oracle, fx, 8, 0), 7), sc.cut_group(oracle, fx, 8, 1)]
    assert raw_verify(kz, s3, pair) == raw_verify(kz, s1, pair) == (BADARGS, [False, True], [BADARGS, 0])


def test_every_sum_at_infinity(kz, s1, s3, pools, reference):
    g = bc.zero_group(pools, 6)
    res, out = sharded_equals_single(kz, s1, s3, [g], reference)
    assert res == [True] and out[0][32:] == bc.INF * 3


def test_force_sharded_cuts_below_two_cells_per_replica(kz, setup_bytes, oracle, fx, s1, s2, reference):
    g = sc.cut_group(oracle, fx, 3)                               # two replicas: blocks of 1 and 2 cells, n >= D but < 2 D
    sc.check_cut(g, 2)
    sf = _load(kz, setup_bytes, [0, 0], KZG355_FORCE_SHARDED="1")
    try:
        assert sharded_equals_single(kz, s1, sf, [g], reference)[0] == [True]
        assert sharded_equals_single(kz, s1, sf, [sc.swap_proofs(g, 0, 1)], reference)[0] == [False]
    finally:
        sf.free()
    before, ex = s2.cell_calls_per_device(), s2.exchange_stats()
    res2, out2 = kz.Kzg.debug_cell_batch_intermediates([g.args], s2)
    assert moved(s2, before) == [1, 0] and s2.exchange_stats() == ex, "without the option the same call goes to one replica"
    assert (out2[0], res2[0]) == cpu_parts(reference, g)


def test_a_block_shaped_group(kz, fx, s1, s3, reference):
    """two blobs x 128 columns = 256 cells in a seeded shuffle, blocks of 85, 85 and 86: both commitments are in every block, every column
    sits twice in the group and most of them in two different blocks, and the exponents pass 2^7 from the second block on"""
    order = [(b, k) for b in (0, 1) for k in range(128)]
    random.Random(0x7594F).shuffle(order)
    c, i, cl, p = dcases.batch(fx, order)
    g = bc.Group("block256", list(zip(c, i, cl, p)), "valid", distinct=2, first=list(dict.fromkeys(c)), columns={k: 2 for k in range(128)})
    bc.check_claims(g)
    sc.check_cut(g, 3)
    assert [cnt for _, cnt in sc.blocks_of(256, 3)] == [85, 85, 86]
    assert sharded_equals_single(kz, s1, s3, [g], reference)[0] == [True]
    assert sharded_equals_single(kz, s1, s3, [sc.swap_proofs(g, 3, 250)])[0] == [False]


# ------------------------------------------------------------------------------------------------ 5: compute
def bad_blob(blob):
    return blob[:32 * 77] + cs.R.to_bytes(32, "big") + blob[32 * 78:]


def test_compute_cells_over_three_replicas(kz, fx, s1, s3):
    blobs = [fx["blobs"][0], fx["blobs"][1], bad_blob(fx["blobs"][0]), fx["blobs"][2]]
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()
    got = kz.Kzg._compute_cells(blobs, s3, True, False)
    assert moved(s3, before) == [1, 1, 1] and s3.exchange_stats() == ex          # ranges of 1, 1 and 2 blobs
    one = kz.Kzg._compute_cells(blobs, s1, True, False)
    assert isinstance(got[2], kz.BadArgs) and isinstance(one[2], kz.BadArgs)
    for t, b in ((0, 0), (1, 1), (3, 2)):
        cells = [x.to_bytes() for x in got[t][0]]
        assert cells == [x.to_bytes() for x in one[t][0]] == fx["cells"][b] and got[t][1] is None
    L = kz.kzg.lib()
    st = (C.c_int * 4)(7, 7, 7, 7)
    out = C.create_string_buffer(ROW * 4)
    assert L.kzg355_compute_cells_and_kzg_proofs_many(out, None, st, b"".join(blobs), 4, s3.handle) == BADARGS and list(st) == [0, 0, BADARGS, 0]


def test_compute_proofs_over_two_replicas(kz, fx, s1, s2):
    blobs = fx["blobs"][:3]
    before = s2.cell_calls_per_device()
    got, one = kz.Kzg.compute_cells_and_kzg_proofs_many(blobs, s2), kz.Kzg.compute_cells_and_kzg_proofs_many(blobs, s1)
    assert moved(s2, before) == [1, 1]
    for b in range(3):
        assert [x.to_bytes() for x in got[b][0]] == [x.to_bytes() for x in one[b][0]] == fx["cells"][b]
        assert [x.to_bytes() for x in got[b][1]] == [x.to_bytes() for x in one[b][1]] == fx["P"][b]
    assert kz.Kzg.debug_cell_compute_h(blobs, s2) == kz.Kzg.debug_cell_compute_h(blobs, s1)
    cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(blobs[1], s2)
    assert [x.to_bytes() for x in cells] == fx["cells"][1] and [x.to_bytes() for x in proofs] == fx["P"][1]
    assert moved(s2, before) == [3, 2], "h: two more ranges; the single blob: the first replica"


# ------------------------------------------------------------------------------------------------ 6: recover
def test_recover_shared_set_over_two_replicas(kz, fx, s1, s2):
    ix = list(range(1, 128, 2))
    rows = [[fx["cells"][b][k] for k in ix] for b in range(3)]
    before = s2.cell_calls_per_device()
    got, one = kz.Kzg.recover_cells_and_kzg_proofs_many(ix, rows, s2), kz.Kzg.recover_cells_and_kzg_proofs_many(ix, rows, s1)
    assert moved(s2, before) == [1, 1]
    for b in range(3):
        assert [x.to_bytes() for x in got[b][0]] == [x.to_bytes() for x in one[b][0]] == fx["cells"][b]
        assert [x.to_bytes() for x in got[b][1]] == [x.to_bytes() for x in one[b][1]] == fx["P"][b]
    cells, proofs = kz.Kzg.recover_cells_and_kzg_proofs(ix, rows[2], s2)
    assert [x.to_bytes() for x in cells] == fx["cells"][2] and [x.to_bytes() for x in proofs] == fx["P"][2]


def sets_call(kz, s, units, cells=True, counts=True):
    m = len(units)
    flat = [i for ix, _ in units for i in ix]
    cnt, idx = (C.c_size_t * m)(*[len(ix) for ix, _ in units]), (C.c_size_t * len(flat))(*flat)
    out = C.create_string_buffer(ROW * m) if cells else None
    st = (C.c_int * m)(*([7] * m))
    rc = kz.kzg.lib().kzg355_recover_cells_and_kzg_proofs_many_sets(out, None, st, cnt if counts else None, idx, b"".join(b"".join(row) for _, row in units), m,
                                                                    s.handle)
    return rc, list(st), out.raw if cells else None


def test_recover_own_sets_over_three_replicas(kz, fx, s1, s3):
    rng = random.Random(7594)
    first64, all128, rand100 = list(range(64)), list(range(128)), sorted(rng.sample(range(128), 100))
    unsorted = list(rand100); unsorted[10], unsorted[11] = unsorted[11], unsorted[10]
    plan = [(0, first64), (1, first64[:63]), (2, all128), (0, unsorted), (1, rand100)]          # ranges of 1, 2 and 2 blobs
    units = [(ix, [fx["cells"][b][k] for k in ix]) for b, ix in plan]
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()
    rc, st, out = sets_call(kz, s3, units)
    assert moved(s3, before) == [1, 1, 1] and s3.exchange_stats() == ex
    assert st == [0, BADARGS, 0, BADARGS, 0] and rc == st[1]
    rc1, st1, out1 = sets_call(kz, s1, units)
    assert (rc1, st1) == (rc, st)
    for t in (0, 2, 4):
        assert out[ROW * t:ROW * (t + 1)] == out1[ROW * t:ROW * (t + 1)] == b"".join(fx["cells"][plan[t][0]]), t
    # what refuses the call as a whole marks every blob and reaches no replica
    before = s3.cell_calls_per_device()
    assert sets_call(kz, s3, units, cells=False)[:2] == (BADARGS, [BADARGS] * 5)
    assert sets_call(kz, s3, units, counts=False)[:2] == (BADARGS, [BADARGS] * 5)
    assert moved(s3, before) == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 7: device-resident calls
def test_device_resident_calls_stay_on_the_first_replica(kz, s3, pools):
    import torch
    groups = [triple(pools, 40, "dev0"), sc.swap_proofs(triple(pools, 43, "dev1"), 0, 1)]

    def u8(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    d = (u8(b"".join(b"".join(g.c) for g in groups)), torch.tensor([int(i) for g in groups for i in g.i], dtype=torch.int64).to("cuda:0"),
         u8(b"".join(b"".join(g.cells) for g in groups)), u8(b"".join(b"".join(g.p) for g in groups)))
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()
    assert kz.Kzg.verify_cell_kzg_proof_batch_many_device(*d, 3, 2, s3) == [True, False]
    assert moved(s3, before) == [1, 0, 0] and s3.exchange_stats() == ex
