"""-m gpu: verify_cell_kzg_proof_batch at the shapes it exists for -- a column sidecar (one cell index, one distinct commitment per cell) and a
block as one batch (up to 128 x 128 cells) -- against the CPU (tests/cell_batch_cases.py, whose inputs and answers tests/test_cell_batch_cases.py
pins to tests/cell_spec.py without a GPU).  Every group runs three ways: the host call (debug_cell_batch_intermediates), the device call prepared
by the device kernels (prep_form 1: k_cell_prep, k_cell_rhash_*) and the device call prepared by the host (prep_form 2).  r, [I(tau)]_1, LL, RL --
all 176 bytes -- and the verdict are compared with the CPU byte for byte: a dedup, numbering or transcript-offset mistake changes r, and a changed
r still verifies a valid batch, so a test that asks for True alone would not see it.  There is no tolerance anywhere.

The sizes are the first on each side of a boundary in the code:
  128 | 129    k_cell_sum's 256-thread stride takes a second pass on side 0 (2 n terms) from 129 cells
  256 | 257    the same on side 2 (n terms); k_cell_prep's insert and its numbering scan take a second pass of their CP_THREADS stride
  2048 | 2049  a second CP_SORT_TILE of the column placement
  4096 | 4097  the fullest dedup table in LDS | the first in HBM (CELL_PREP_LDS_SLOTS = 8192 slots = 2 x 4096)
  16384 | 16385  CELL_PREP_MAX_CELLS: the last call the device prepares | the first that cells.hip hands to the host preparation
  rhash_lanes_from - 1 | rhash_lanes_from groups: k_cell_rhash_wave | k_cell_rhash_lanes
At 16384 / 16385 the CPU gives r and [I(tau)]_1 only (the sums of 16384 points are pinned at the sizes below); LL, RL and the verdict are then
compared between the three routes."""
import os
import re
import time
from collections import Counter

import pytest

import cell_batch_cases as bc
import cell_spec as cs

pytestmark = pytest.mark.gpu

ROUTES = (("host call", None), ("device call, device preparation", 1), ("device call, host preparation", 2))


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def settings(kz, setup_bytes):
    g1, g2 = setup_bytes
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
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
    """the CPU's answer per group, computed once per group name and shared by the tests of this module"""
    reference, known = bc.Reference(oracle, fx), {}

    def get(g, sums=True):
        bc.check_claims(g)
        if (g.name, sums) not in known:
            try:
                known[g.name, sums] = g.args, reference(*g.args, sums=sums)
            except cs.BadArgs:
                known[g.name, sums] = g.args, "BadArgs"
        args, answer = known[g.name, sums]
        assert args == g.args, f"two different groups are called {g.name}"
        return answer
    return get


def u8(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def to_device(torch, groups):
    return (u8(torch, b"".join(b"".join(g.c) for g in groups)), torch.tensor([int(i) for g in groups for i in g.i], dtype=torch.int64).cuda(),
            u8(torch, b"".join(b"".join(g.cells) for g in groups)), u8(torch, b"".join(b"".join(g.p) for g in groups)))


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def three_routes(kz, torch, settings, groups):
    """{route: (verdicts, [176 bytes per group], device preparations counted)} of one _many call per route"""
    npg, G = groups[0].n, len(groups)
    assert all(g.n == npg for g in groups)
    d = to_device(torch, groups)
    out = {}
    for name, form in ROUTES:
        before, t0 = settings.cell_device_prep_calls, time.perf_counter()
        if form is None:
            res, o = kz.Kzg.debug_cell_batch_intermediates([g.args for g in groups], settings)
        else:
            res, o = kz.Kzg.debug_cell_batch_intermediates_device(*d, npg, G, settings, prep_form=form)
        print(f"{G} x {npg} cells, {name}: {time.perf_counter() - t0:.3f} s")
        out[name] = (norm(res), o, settings.cell_device_prep_calls - before)
    return out


def parts(o):
    return {"r": o[:32].hex(), "itau": o[32:80].hex(), "ll": o[80:128].hex(), "rl": o[128:176].hex()}


def check_exact(kz, torch, settings, want, groups):
    """every route, every group: the verdict and all 176 bytes are the CPU's; a group the CPU refuses is BadArgs on every route"""
    t0 = time.perf_counter()
    cpu = [want(g) for g in groups]
    print(f"{len(groups)} x {groups[0].n} cells, CPU: {time.perf_counter() - t0:.3f} s")
    for g, w in zip(groups, cpu):                                 # the CPU itself tells valid from spoiled
        assert (w == "BadArgs") == (g.kind == "malformed") and (w == "BadArgs" or w[4] is (g.kind == "valid")), (g.name, g.kind)
    got = three_routes(kz, torch, settings, groups)
    for route, (res, outs, prepared) in got.items():
        assert prepared == (1 if route == ROUTES[1][0] else 0), route
        for t, (g, w) in enumerate(zip(groups, cpu)):
            if w == "BadArgs":
                assert res[t] == "BadArgs", (route, g.name)
                continue
            assert parts(outs[t]) == {"r": w[0].hex(), "itau": w[1].hex(), "ll": w[2].hex(), "rl": w[3].hex()}, (route, g.name)
            assert res[t] is w[4], (route, g.name, res[t])
    return got


# ---- 1. every commitment distinct: mixtures at the first size on each side of k_cell_sum's and k_cell_prep's 256-thread strides
@pytest.mark.parametrize("n", [128, 129, 256, 257])
def test_distinct_commitments_sidecar_columns_and_spoilings(kz, torch, settings, pools, want, n):
    base = bc.distinct_group(pools, n, "mixed")
    groups = [base, bc.distinct_group(pools, n, "sidecar"), bc.distinct_group(pools, n, "columns")]
    groups += [bc.spoil(base, what, n - 1, pools.spare[0]) for what in bc.SPOILINGS]      # the last cell: the one past the stride at 129 / 257
    assert [g.distinct for g in groups] == [n] * 7 and [g.kind for g in groups] == ["valid"] * 3 + ["spoiled"] * 4
    got = check_exact(kz, torch, settings, want, groups)
    assert got["host call"][0] == [True] * 3 + [False] * 4


# ---- 2. orders of first appearance and of repeats, valid by construction
@pytest.mark.parametrize("order", bc.DEDUP_ORDERS)
@pytest.mark.parametrize("n", [257, 2049])
def test_dedup_orders(kz, torch, settings, pools, want, n, order):
    g = bc.dedup_group(pools, n, order)
    got = check_exact(kz, torch, settings, want, [g])
    assert got["host call"][0] == [True]


# ---- 3. up to 4097 distinct commitments: the column placement's second tile, the fullest LDS table, the first HBM table
@pytest.mark.parametrize("n", [2048, 2049, 4096, 4097])
def test_thousands_of_distinct_commitments(kz, torch, settings, pools, want, n):
    g = bc.setup_group(pools, n)
    assert g.distinct == n
    got = check_exact(kz, torch, settings, want, [g])
    assert got["host call"][0] == [False]


def test_one_commitment_4097_times(kz, torch, settings, pools, want):
    """a single key under atomicMin from every wave of every pass, in the HBM table"""
    g = bc.dedup_group(pools, 4097, "one")
    got = check_exact(kz, torch, settings, want, [g])
    assert got["host call"][0] == [True]


# ---- 4. a block as one batch: the device preparation's cap and the first size above it
@pytest.mark.parametrize("n", [16384, 16385])
def test_the_device_preparations_cap(kz, torch, settings, pools, want, n):
    g = bc.setup_group(pools, n, every=2)
    assert g.distinct == 8192
    w = want(g, sums=False)
    got = three_routes(kz, torch, settings, [g])
    for route, (res, outs, prepared) in got.items():
        assert res in ([True], [False]), (route, res)             # status OK: the group is well-formed (the CPU has not validated its points)
        p = parts(outs[0])
        assert (p["r"], p["itau"]) == (w[0].hex(), w[1].hex()), route
    host = got["host call"]
    for route in (ROUTES[1][0], ROUTES[2][0]):                    # LL, RL and the verdict by route parity
        assert got[route][1] == host[1] and got[route][0] == host[0], route
    assert host[0] == [False]
    # 16384 cells with prep_form 1 are prepared on the device, 16385 are not (cells.hip hands them to the host preparation); prep_form 2 never is
    assert got[ROUTES[1][0]][2] == (1 if n <= 16384 else 0) and got[ROUTES[2][0]][2] == 0 and host[2] == 0


# ---- 5. both transcript kernels with 8 distinct commitments in every group
def rhash_lanes_from(torch, settings):
    """the number of groups from which the one-lane-per-group transcript kernel runs, read from options.hip: a multiple of the device's CU count"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kzg_rust_amd", "csrc", "options.hip")).read()
    m = re.search(r"s->rhash_lanes_from = opt\.rhash_lanes_from > 0 \? opt\.rhash_lanes_from : (\d+) \* cus;", src)
    assert m, "options.hip no longer sets rhash_lanes_from the way this test reads it"
    return int(m.group(1)) * torch.cuda.get_device_properties(settings.device).multi_processor_count


def test_both_transcript_kernels_with_distinct_commitments(kz, torch, settings, pools, want):
    lanes = rhash_lanes_from(torch, settings)
    assert 64 < lanes <= 1024                                     # 8 x lanes distinct setup points exist
    big = bc.setup_group(pools, 8 * lanes)
    assert big.distinct == 8 * lanes
    items = big.items()
    groups = []
    for t in range(lanes):
        sl = items[8 * t:8 * t + 8]
        groups.append(bc.Group(f"eight{t}", sl, "spoiled", distinct=8, first=[x[0] for x in sl], columns=dict(Counter(x[1] for x in sl))))
    d = to_device(torch, groups)
    seen = {}
    for G in (lanes, lanes - 1):                                  # k_cell_rhash_lanes, then k_cell_rhash_wave on all but the last group
        before = settings.cell_device_prep_calls
        res, outs = kz.Kzg.debug_cell_batch_intermediates_device(d[0][:48 * 8 * G], d[1][:8 * G], d[2][:2048 * 8 * G], d[3][:48 * 8 * G], 8, G, settings,
                                                                 prep_form=1)
        assert settings.cell_device_prep_calls - before == 1
        assert norm(res) == [False] * G
        for t in range(G):
            bc.check_claims(groups[t])
            assert outs[t][:32] == cs._be(bc.challenge(*groups[t].args)[0]), (G, t)
        seen[G] = outs
    assert seen[lanes][:lanes - 1] == seen[lanes - 1]             # and the two kernels' calls agree in all 176 bytes
    for t in (0, lanes - 2):                                      # two groups in full against the CPU
        w = want(groups[t])
        assert seen[lanes - 1][t] == w[0] + w[1] + w[2] + w[3] and w[4] is False


# ---- 6. sums at infinity
def test_all_three_sums_at_infinity(kz, torch, settings, pools, want):
    g = bc.zero_group(pools, 129)
    w = want(g)
    assert (w[1], w[2], w[3], w[4]) == (bc.INF, bc.INF, bc.INF, True)
    check_exact(kz, torch, settings, want, [g])


def test_ll_and_rl_at_infinity_and_the_spoiled_neighbour(kz, torch, settings, pools, want):
    g = bc.constlin_group(pools, 129)
    w = want(g)
    assert w[1] != bc.INF and (w[2], w[3], w[4]) == (bc.INF, bc.INF, True)
    s = bc.spoil(g, "cell", 128)
    w = want(s)
    assert w[2] == bc.INF and w[3] != bc.INF and w[4] is False    # LL at infinity, RL finite
    check_exact(kz, torch, settings, want, [g])
    check_exact(kz, torch, settings, want, [s])
    check_exact(kz, torch, settings, want, [g, s])


def test_infinity_among_129_distinct_commitments(kz, torch, settings, pools, want):
    g = bc.mixed_group(pools, 129)
    assert g.distinct == 129 and g.c.count(bc.INF) == 1 and g.p.count(bc.INF) >= 21 and g.p.count(pools.fx["mono"][0]) == 1
    got = check_exact(kz, torch, settings, want, [g])
    assert got["host call"][0] == [True]


# ---- 7. one _many call of 129-cell groups of every kind: statuses and verdicts land on their own groups
def test_mixed_many_call(kz, torch, settings, pools, want):
    base = bc.distinct_group(pools, 129, "mixed")
    cl = bc.constlin_group(pools, 129)
    groups = [base, bc.spoil(base, "cell", 128), bc.zero_group(pools, 129), bc.malformed_index(base, 64), bc.distinct_group(pools, 129, "sidecar"),
              bc.spoil(base, "commitment", 128, pools.spare[0]), cl, bc.spoil(cl, "cell", 128), bc.mixed_group(pools, 129), bc.setup_group(pools, 129),
              bc.malformed_index(cl, 128), bc.distinct_group(pools, 129, "columns")]
    got = check_exact(kz, torch, settings, want, groups)
    expect = [True, False, True, "BadArgs", True, False, True, False, True, False, "BadArgs", True]
    for route, (res, _, _) in got.items():
        assert res == expect, route
