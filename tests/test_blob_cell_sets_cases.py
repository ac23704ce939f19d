"""CPU only: the calls of tests/blob_cell_sets_cases.py (the inputs of tests/test_gpu_blob_cell_sets.py) are what they say.  Every group's claims
hold on its bytes, the CPU's answer of every group is cell_spec.verify_cell_kzg_proof_batch over the group's own 128 n cells and says what the
group's kind says, the flat arrays cut by the counts give each group back, blobs within a group and across the groups of a call differ (but for
the calls that share commitments on purpose), and every spoil sits in the last blob of its group."""
import pytest

import blob_cell_cases as bcc
import blob_cell_sets_cases as ss
import blob_cell_shape_cases as sc
import cell_spec as cs

N = sc.N


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def named(oracle, fx):
    return ss.named_groups(sc.Pools(oracle, fx))


def test_every_group_claims_what_it_holds(named):
    assert len(named) == 21
    for name, g in named.items():
        assert g.name == name
        sc.check_claims(g)
    assert named["empty"].n == 0 and named["empty"].args == ([], [], [])
    assert [named[k].distinct for k in ("share-AB", "share-A", "share-BAA", "two-AA", "three-ABA", "dedup-ABAC")] == [2, 1, 2, 1, 2, 3]
    assert named["zshare-AB"].c[1] == sc.INF and named["zshare-BAA"].c[0] == sc.INF and named["dedup-kinds"].c[1] == sc.INF
    # the shared commitments are the same bytes in the three groups, in another order of first appearance
    ab, a, baa = (named[k] for k in ("share-AB", "share-A", "share-BAA"))
    assert ab.first == [ab.c[0], ab.c[1]] and a.first == [ab.c[0]] and baa.first == [ab.c[1], ab.c[0]] and baa.c == [ab.c[1], ab.c[0], ab.c[0]]


def test_the_calls_have_the_counts_they_are_named_after(named):
    assert set(ss.CALLS) == set(ss.COUNTS)
    for name in ss.CALLS:
        gs = ss.call(named, name)
        assert ss.counts(gs) == list(ss.COUNTS[name])
        live = [g for g in gs if g.n]
        assert len({tuple(g.blobs) for g in live}) == len(live), name        # no two groups of a call are alike
        if not name.startswith("shared"):                         # and no blob sits in two groups; within a group only A, A repeats one
            blobs = [b for g in live for b in set(g.blobs)]
            assert len(set(blobs)) == len(blobs), name
        for g in (g for g in live if g.kind == "valid"):
            assert len(set(g.blobs)) == g.distinct, (name, g.name)
    assert sum(ss.COUNTS["offsets-7"]) == 7 and sum(ss.COUNTS["offsets-3"]) == 3 and sum(ss.COUNTS["route-6"]) == 6 and sum(ss.COUNTS["route-7"]) == 7
    assert [g.kind for g in ss.call(named, "statuses")] == list(ss.STATUSES_KINDS)


def test_spoils_sit_in_the_last_blob_of_their_group(named):
    for spoiled, base in (("distinct2@9-element1.4095", "distinct2@9"), ("three-ABA-element2.2077=r", "three-ABA"),
                          ("dedup-ABAC-proof3.127-off-curve", "dedup-ABAC")):
        s, g = named[spoiled], named[base]
        last = g.n - 1
        assert s.blobs[:last] == g.blobs[:last] and s.c == g.c and s.p[:N * last] == g.p[:N * last], spoiled
        assert (s.blobs[last] != g.blobs[last]) != (s.p[N * last:] != g.p[N * last:]), spoiled
    assert int.from_bytes(named["three-ABA-element2.2077=r"].blobs[2][32 * 2077:32 * 2078], "big") == cs.R


def test_slicing_the_flat_arrays_by_the_counts_gives_each_group_back(named):
    for name in ss.CALLS:
        gs = ss.call(named, name)
        blobs, c, p, cnts = ss.flat(gs)
        assert len(blobs) == len(c) == sum(cnts) and len(p) == N * sum(cnts)
        assert ss.slices(blobs, c, p, cnts) == [g.args for g in gs], name
    gs = ss.chunked(named)
    blobs, c, p, cnts = ss.flat(gs)
    assert sum(cnts) == 2050 and ss.slices(blobs, c, p, cnts) == [g.args for g in gs]
    with pytest.raises(AssertionError):                           # counts that do not add up to the arrays
        ss.slices(blobs, c, p, cnts[:-1])


def test_the_answer_of_a_group_is_the_spec_on_that_group_alone(oracle, fx, named):
    seen = {"valid": 0, "spoiled": 0, "malformed": 0}
    for name, g in named.items():
        got = ss.answer(oracle, fx, g)
        if g.n == 0:
            assert got == (bytes(176), True)
            continue
        seen[g.kind] += 1
        if g.kind == "malformed":
            assert got == "BadArgs", name
            with pytest.raises(cs.BadArgs):
                sc.expected(oracle, fx, g)
            continue
        ok, parts = cs.verify_cell_kzg_proof_batch(oracle, *bcc.group_args(g.cells, g.c, g.p), mono=fx["mono"], g2=fx["g2"], intermediates=True)
        assert got == (parts["r"] + parts["itau"] + parts["ll"] + parts["rl"], ok) and ok is (g.kind == "valid"), name
        r, uniq, _ = cs.challenge(*bcc.group_args(g.cells, g.c, g.p))
        assert got[0][:32] == cs._be(r) and uniq == g.first, name
    assert seen == {"valid": 17, "spoiled": 1, "malformed": 2}
    # groups that share commitments have their own r
    assert len({ss.answer(oracle, fx, named[k])[0][:32] for k in ("share-AB", "share-A", "share-BAA")}) == 3
