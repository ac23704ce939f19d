"""CPU only: the inputs and the CPU answers of tests/test_gpu_blob_cell_shapes.py (tests/blob_cell_shape_cases.py) are what they say.  Every
group's claims (kind, distinct commitments, order of first appearance) equal what observed() reads from its bytes, a sample of mixture and
low-degree blobs passes cell_spec.verify_cell_kzg_proof_batch over all 128 (cell, proof) pairs against the blob's commitment, the spec's verdict of
every group is what its kind says -- valid True, spoiled False, malformed BadArgs, none "may still verify" -- and BigReference, the shortened
computation used for the 128- and 129-blob groups, gives the spec's 176 bytes on small groups.  The 128- and 129-blob groups themselves are built and
answered only in the GPU module's fixture (23 s of CPU), where their claims are checked too, so that this module stays short."""
import pytest

import blob_cell_cases as bcc
import blob_cell_shape_cases as sc
import cell_spec as cs

N = sc.N


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def pools(oracle, fx):
    return sc.Pools(oracle, fx)


@pytest.fixture(scope="module")
def groups(pools):
    return sc.small_groups(pools)


def test_every_group_claims_what_it_holds(groups, pools):
    names = {g.name for g in groups}
    assert len(groups) == len(names) == 24 and [g.kind for g in groups].count("spoiled") == 3 and [g.kind for g in groups].count("malformed") == 2
    for g in groups:
        sc.check_claims(g)
        assert sc.observed(g) == (g.distinct, g.first), g.name
    want = {"dedup-ABAC": (4, 3, [0, 1, 3]), "dedup-AABAC": (5, 3, [0, 2, 4]), "dedup-ABCDA": (5, 4, [0, 1, 2, 3]), "distinct7": (7, 7, list(range(7))),
            "dedup-kinds": (4, 4, [0, 1, 2, 3]), "three-ABA": (3, 2, [0, 1]), "two-AA": (2, 1, [0])}
    by_name = {g.name: g for g in groups}
    for name, (n, distinct, firsts) in want.items():
        g = by_name[name]
        assert (g.n, g.distinct) == (n, distinct) and g.first == [g.c[b] for b in firsts], name
    assert by_name["dedup-kinds"].c[1] == sc.INF and by_name["dedup-kinds"].c.count(sc.INF) == 1
    for n, count in sc.LAUNCH_SETS:
        gs = sc.launch_set_groups(pools, n, count)
        assert len(gs) == count and all(g.n == n for g in gs) and len({g.name for g in gs}) == count
    # the spoils at seven: the last blob, one part each
    base, spoils = by_name["distinct7"], sc.spoils_at_seven(pools)
    changed = {what: [s.blobs != base.blobs, s.c != base.c, s.p != base.p] for what, s in spoils.items()}
    assert changed == {"element": [True, False, False], "commitments": [False, True, False], "proofs": [False, False, True],
                       "element=r": [True, False, False], "off-curve proof": [False, False, True]}
    assert spoils["commitments"].first == base.first[:5] + [base.first[6], base.first[5]] and spoils["commitments"].distinct == 7
    assert int.from_bytes(spoils["element=r"].blobs[6][32 * 2077:32 * 2078], "big") == cs.R


def test_a_claim_that_does_not_hold_and_a_spoiling_that_changes_nothing_are_errors(pools):
    g = sc.dedup_group(pools, "ABAC")
    with pytest.raises(AssertionError):
        h = g.copy("collapsed", "valid")
        h.c[3] = h.c[1]
        sc.check_claims(h)
    with pytest.raises(AssertionError):
        h = g.copy("reordered", "valid")
        h.c[0], h.c[1] = h.c[1], h.c[0]
        sc.check_claims(h)
    with pytest.raises(AssertionError):
        sc.spoil_swap_proofs(g, 1, 7, 7)
    with pytest.raises(AssertionError):                          # A and A
        sc.spoil_swap_commitments(g, 0, 2)
    low = sc.planned("low", [pools.low("deg63")], [0])
    with pytest.raises(AssertionError):                          # every proof of a blob of degree < 64 is the point at infinity
        sc.spoil_swap_proofs(low, 0, 127, 126)


def test_whole_blobs_pass_the_cell_check(oracle, fx, pools):
    sample = [pools.mix(0), pools.mix(12), pools.mix(16)] + [pools.low(what) for what in ("zero", "deg63", "x64", "deg127")]
    assert len({w.c for w in sample}) == len(sample)
    for w in sample:
        assert cs.verify_cell_kzg_proof_batch(oracle, [w.c] * N, list(range(N)), w.cells, w.p, mono=fx["mono"], g2=fx["g2"]) is True, w.tag
        assert w.cells[:64] == [w.blob[2048 * k:2048 * k + 2048] for k in range(64)], w.tag
    w = sample[0]                                                 # and the check is not vacuous
    assert cs.verify_cell_kzg_proof_batch(oracle, [w.c] * N, list(range(N)), w.cells, w.p[1:] + w.p[:1], mono=fx["mono"], g2=fx["g2"]) is False


def test_the_spec_says_what_each_kind_says(oracle, fx, groups):
    seen = {"valid": 0, "spoiled": 0, "malformed": 0}
    for g in groups:
        if g.kind == "malformed":
            with pytest.raises(cs.BadArgs):
                sc.expected(oracle, fx, g)
        else:
            out, ok = sc.expected(oracle, fx, g)
            assert ok is (g.kind == "valid"), (g.name, g.kind, ok)
            r, uniq, _ = cs.challenge(*bcc.group_args(g.cells, g.c, g.p))
            assert out[:32] == cs._be(r) and uniq == g.first, g.name
        seen[g.kind] += 1
    assert seen == {"valid": 19, "spoiled": 3, "malformed": 2}


def test_big_reference_is_the_spec_on_small_groups(oracle, fx, pools):
    big = sc.BigReference(oracle, fx)
    g = sc.distinct_group(pools, 2, 9)
    aba = sc.dedup_group(pools, "ABAC")
    swapped = sc.spoil_swap_proofs(aba, 3, 127, 126)
    for grp, verdict in ((g, True), (aba, True), (swapped, False)):
        assert big(grp) == sc.expected(oracle, fx, grp) and big(grp)[1] is verdict, grp.name
    with pytest.raises(cs.BadArgs):
        big(sc.malformed_proof(aba, 3, 127, sc.dcases.off_curve(oracle)))
    with pytest.raises(AssertionError):                          # a blob that is no mixture has no coefficients here
        big(sc.spoil_element(aba, 3, 5))
