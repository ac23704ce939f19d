"""CPU only: the calls of tests/test_gpu_cell_sets.py (tests/cell_sets_cases.py) are what they say.  Every call's counts, its groups' claims
(distinct commitments, first-appearance order, cells per column), which neighbours share a commitment or a column and which group is spoiled are
recomputed from the bytes, and the CPU answer the GPU test compares with -- cell_batch_cases.Reference, one group at a time -- is pinned to
cell_spec.verify_cell_kzg_proof_batch for every non-empty group of every call.  So a machine without a GPU proves that the expected bytes of the
_sets call are the spec's, group by group."""
import pytest

import cell_batch_cases as bc
import cell_device_cases as dcases
import cell_sets_cases as sets
import cell_spec as cs


@pytest.fixture(scope="module")
def fx():
    return bc.fixture()


@pytest.fixture(scope="module")
def pools(oracle, fx):
    return bc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def reference(oracle, fx):
    return bc.Reference(oracle, fx)


@pytest.fixture(scope="module")
def calls(oracle, pools):
    out = [sets.side_by_side(pools), sets.empty_ends(pools), sets.all_empty(), sets.borders(pools), sets.uniform(pools), sets.many_small(pools),
           sets.two_groups(pools)]
    return out + sets.status_calls(pools, dcases.not_in_subgroup(oracle), dcases.off_curve(oracle))


def test_every_call_claims_what_it_holds(calls):
    assert len({c.name for c in calls}) == len(calls) == 17
    for call in calls:
        sets.check_call(call)
    by = {c.name: c for c in calls}
    assert by["side-by-side"].counts == [1, 129, 0, 2, 257, 128, 0, 0, 3] and by["empty-ends"].counts == [0, 5, 0] and by["all-empty"].counts == [0, 0, 0]
    assert by["many-small"].counts == [1, 2, 3, 0] * 17 + [1, 2] and by["uniform"].counts == [5] * 4
    assert sum(by["proof-first-of-2-large"].counts) * 2 > 1024    # past the four-lanes-per-point form of the subgroup test
    # the border: the same commitment on the same column ends one group and begins the next, which repeats it
    a, b = by["borders"].groups[:2]
    assert (a.c[-1], a.i[-1]) == (b.c[0], b.i[0]) and b.c[2] == b.c[4] == b.c[0]
    # a dedup across that border would give group 1 a transcript with another first-appearance list: its own starts with X
    assert b.first[0] == a.c[-1] and a.first[-1] == a.c[-1]


def test_the_spoiled_groups_are_where_the_names_say(calls, oracle):
    bad_pts = {dcases.not_in_subgroup(oracle), dcases.off_curve(oracle)}
    assert all(oracle.g1_validate(p) != 0 for p in bad_pts)
    for call in calls:
        if "-of-" not in call.name:
            continue
        at = 1 if "last-of-1" in call.name else 2
        assert call.spoiled[at] == "malformed" and list(call.spoiled.values()).count("malformed") == 1, call.name
        g = call.groups[at]
        j = g.n - 1 if at == 1 else 0
        if call.name.startswith("proof"):
            assert g.p[j] in bad_pts and not (set(g.p[:j] + g.p[j + 1:] + g.c) & bad_pts), call.name
        elif call.name.startswith("commitment"):
            assert g.c[j] in bad_pts and not (set(g.c[:j] + g.c[j + 1:] + g.p) & bad_pts), call.name
        elif call.name.startswith("element"):
            assert [cs.R.to_bytes(32, "big") in (c[32 * e:32 * e + 32] for e in range(64)) for c in g.cells] == [t == j for t in range(g.n)], call.name
        else:
            assert [int(i) for i in g.i].index(128) == j and list(g.i).count(128) == 1, call.name
        for t, other in enumerate(call.groups):                   # nothing else in the call is malformed
            if t != at:
                assert max([int(i) for i in other.i], default=0) < 128 and not (set(other.c + other.p) & bad_pts), (call.name, t)


def test_the_cpu_answer_of_every_group_is_the_specs(calls, oracle, fx, reference):
    seen, verdicts = set(), {}
    for call in calls:
        for t, g in enumerate(call.groups):
            if g.n == 0:
                assert sets.cpu_answer(reference, g) == (True, sets.ZERO_DEBUG)
                continue
            want_kind = call.spoiled.get(t, "valid")
            if g.name in seen:                                    # a group that stands in several calls is pinned once
                assert verdicts[g.name] == (want_kind, g.args), f"two different groups are called {g.name}"
                continue
            seen.add(g.name)
            verdicts[g.name] = want_kind, g.args
            got = sets.cpu_answer(reference, g)
            try:
                ok, d = cs.verify_cell_kzg_proof_batch(oracle, *g.args, mono=fx["mono"][:64], g2=fx["g2"], intermediates=True)
            except cs.BadArgs:
                assert got == ("BadArgs", None) and want_kind == "malformed", (call.name, g.name)
                continue
            assert got == (ok, d["r"] + d["itau"] + d["ll"] + d["rl"]), (call.name, g.name)
            assert ok is (want_kind == "valid"), (call.name, g.name, ok)
    assert len(seen) > 80
