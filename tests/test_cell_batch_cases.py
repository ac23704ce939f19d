"""CPU only: the inputs and the CPU answer of tests/test_gpu_cell_batch_shapes.py (tests/cell_batch_cases.py) are what they say.  The builders'
groups at 129 cells get the same r, [I(tau)]_1, LL, RL and verdict from cell_batch_cases.Reference as from cell_spec.verify_cell_kzg_proof_batch, every
valid group is True and every spoiled group False under the spec, a sample of the items passes the single-cell check, every builder's claims
(distinct commitments, first-appearance order, cells per column) hold at the sizes the GPU test runs, and a spoiling that changes nothing is an
error.  So a machine without a GPU proves that the reference alone tells valid from spoiled."""
import random

import pytest

import cell_batch_cases as bc
import cell_spec as cs

R = cs.R


@pytest.fixture(scope="module")
def fx():
    return bc.fixture()


@pytest.fixture(scope="module")
def pools(oracle, fx):
    return bc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def reference(oracle, fx):
    return bc.Reference(oracle, fx)


def small_groups(pools, n=129):
    out = []
    for layout in ("mixed", "sidecar", "columns"):
        out.append(bc.distinct_group(pools, n, layout))
    base = out[0]
    donor = pools.spare[0]
    out += [bc.spoil(base, what, n - 1, donor) for what in bc.SPOILINGS]
    out += [bc.dedup_group(pools, n, order) for order in bc.DEDUP_ORDERS]
    out.append(bc.setup_group(pools, n))
    out.append(bc.setup_group(pools, n, every=2))
    out.append(bc.zero_group(pools, n))
    cl = bc.constlin_group(pools, n)
    out += [cl, bc.spoil(cl, "cell", 77), bc.mixed_group(pools, n)]
    return out


def test_dictionary_challenge_is_the_specs(pools):
    for g in (bc.distinct_group(pools, 40, "mixed"), bc.dedup_group(pools, 41, "two"), bc.dedup_group(pools, 41, "half"), bc.setup_group(pools, 33, 2)):
        assert bc.challenge(*g.args) == cs.challenge(*g.args), g.name


def test_reference_is_the_spec_at_129_cells(oracle, fx, pools, reference):
    groups = small_groups(pools)
    assert len({g.name for g in groups}) == len(groups) >= 17
    seen = set()
    for g in groups:
        bc.check_claims(g)
        ok, d = cs.verify_cell_kzg_proof_batch(oracle, *g.args, mono=fx["mono"][:64], g2=fx["g2"], intermediates=True)
        assert reference(*g.args) == (d["r"], d["itau"], d["ll"], d["rl"], ok), g.name
        assert ok is (g.kind == "valid"), (g.name, g.kind, ok)
        assert reference(*g.args, sums=False)[:2] == (d["r"], d["itau"]), g.name
        seen.add((d["itau"] == bc.INF, d["ll"] == bc.INF, d["rl"] == bc.INF, ok))
    # the corners at infinity are really there: all three at infinity (True), LL and RL only (True), LL only (False)
    assert {(True, True, True, True), (False, True, True, True), (False, True, False, False), (False, False, False, True)} <= seen
    bad = bc.malformed_index(groups[0], 5)
    for call in (lambda: reference(*bad.args), lambda: cs.verify_cell_kzg_proof_batch(oracle, *bad.args, mono=fx["mono"][:64], g2=fx["g2"])):
        with pytest.raises(cs.BadArgs):
            call()


def test_items_pass_the_single_cell_check(oracle, fx, pools):
    rng = random.Random(5)
    items = rng.sample(pools.mixed, 4) + [pools.sidecar[200], pools.columns[256], pools.spare[1], pools.many(bc.POOL + 3)[-1]]
    items += bc.mixed_group(pools).items()[1:12:2] + bc.constlin_group(pools, 4).items() + bc.zero_group(pools, 2).items()
    assert len(items) >= 20
    for c, k, cell, p in items:
        assert oracle.g1_validate(c) == 0 and oracle.g1_validate(p) == 0
        assert cs.single_cell_check(oracle, c, k, cell, p, mono=fx["mono"][:64], g2=fx["g2"])
    c, k, cell, p = items[0]
    assert not cs.single_cell_check(oracle, c, (k + 1) % 128, cell, p, mono=fx["mono"][:64], g2=fx["g2"])


def test_setup_points_are_8192_distinct_valid_points(oracle, pools):
    pts = pools.setup
    assert len(pts) == len(set(pts)) == 8192 and bc.INF not in pts
    assert all(oracle.g1_validate(p) == 0 for p in pts)


def test_builders_claim_what_they_build_at_the_gpu_sizes(pools):
    n_groups = 0
    for n in (128, 129, 256, 257):
        for layout in ("mixed", "sidecar", "columns"):
            g = bc.distinct_group(pools, n, layout)
            bc.check_claims(g)
            assert g.distinct == n == g.n
            assert len(g.columns) == {"sidecar": 1, "columns": 128}.get(layout, len(g.columns))
            n_groups += 1
        base = bc.distinct_group(pools, n, "mixed")
        for what in bc.SPOILINGS:
            s = bc.spoil(base, what, n - 1, pools.spare[0])
            bc.check_claims(s)
            changed = [t for t in range(4) if s.args[t] != base.args[t]]
            assert changed == [{"commitment": 0, "index": 1, "cell": 2, "proof": 3}[what]] and s.distinct == n
            assert [a == b for a, b in zip(s.items(), base.items())].count(False) == 1
    for n in (257, 2049):
        for order, u in (("one", 1), ("two", 2), ("half", n // 2), ("descending", min(n, bc.POOL))):
            g = bc.dedup_group(pools, n, order)
            bc.check_claims(g)
            assert (g.n, g.distinct) == (n, u)
        h = bc.dedup_group(pools, n, "half")
        second = [h.c.index(c, h.c.index(c) + 1) - h.c.index(c) for c in h.first[:50]]
        assert min(second) >= n // 2 - 100                       # every second appearance is far from the first
        d = bc.dedup_group(pools, n, "descending")
        assert d.first == sorted(d.first, reverse=True)
    for n in (2048, 2049, 4096, 4097):
        g = bc.setup_group(pools, n)
        bc.check_claims(g)
        assert g.distinct == g.n == n
    for n in (16384, 16385):
        g = bc.setup_group(pools, n, every=2)
        bc.check_claims(g)
        assert (g.n, g.distinct) == (n, 8192) and len(g.columns) == 128
    g = bc.dedup_group(pools, 4097, "one")
    bc.check_claims(g)
    assert g.distinct == 1
    for g in (bc.zero_group(pools, 129), bc.constlin_group(pools, 129), bc.mixed_group(pools, 129)):
        bc.check_claims(g)
    assert bc.zero_group(pools, 129).distinct == 1 and bc.constlin_group(pools, 129).distinct == 129 and bc.mixed_group(pools, 129).distinct == 129
    assert n_groups == 12


def test_a_spoiling_that_changes_nothing_is_an_error(pools):
    g = bc.distinct_group(pools, 8, "mixed")
    same = g.items()[3]
    for what in ("proof", "commitment"):
        with pytest.raises(AssertionError):
            bc.spoil(g, what, 3, same)
    with pytest.raises(AssertionError):                          # a commitment the group holds already would collapse two into one
        bc.spoil(g, "commitment", 3, g.items()[4])
    with pytest.raises(AssertionError):                          # a claim that does not hold is found out
        h = bc.distinct_group(pools, 8, "mixed")
        h.c[2] = h.c[1]
        bc.check_claims(h)
