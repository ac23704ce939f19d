"""-m "not gpu": tests/blob_sets_cases.py, the calls and CPU answers the verify_blob_kzg_proof_batch_many_sets tests compare the device with.
Pinned here without a GPU: the slices tile the arrays, empty groups answer true, a group of one equals verify_blob_kzg_proof, the whole 64-blob
fixture reproduces its recorded r / proof_lincomb / rhs, every spoil changes exactly the groups it names, and the two host-side rules the GPU
tests predict (launch-set breaks, device cuts) behave as include/kzg355.h states them."""
import pytest

import blob_sets_cases as bs


@pytest.fixture(scope="module")
def clean(oracle, oracle_settings):
    call = bs.borders()
    return call, bs.answers(oracle, oracle_settings, call)


def test_slices_tile_the_arrays_with_no_gap():
    for call in (bs.borders(), bs.borders().reversed(), bs.many(), bs.large(), bs.whole512()):
        assert call.off[0] == 0 and call.off[-1] == call.total == sum(call.counts)
        assert all(call.off[g + 1] - call.off[g] == call.counts[g] for g in range(len(call.counts)))
    assert bs.borders().total == 31 and bs.many().total == 286 and sum(1 for c in bs.MANY if c > 1) == 78 and len(bs.MANY) == 130
    call = bs.borders()
    blobs, cs, ps = call.flat()
    assert len(blobs) == 131072 * 31 and len(cs) == len(ps) == 48 * 31
    groups = call.groups()
    assert b"".join(b"".join(g[0]) for g in groups) == blobs and b"".join(b"".join(g[1]) for g in groups) == cs
    assert b"".join(b"".join(g[2]) for g in groups) == ps
    # 10 blobs are 62 lincomb items and 11 are 68: a 64-lane wave straddles groups 5 | 6 and group 6 spans two waves
    item0 = [2 * (3 * o + l) for l, o in enumerate(bs.offsets([c for c in bs.BORDERS if c]))]
    assert item0[3] - item0[2] == 62 and item0[4] - item0[3] == 68
    assert item0[3] % 64 != 0 and item0[3] // 64 != (item0[4] - 1) // 64


def test_empty_groups_answer_true_and_singles_equal_the_single_check(oracle, oracle_settings, clean):
    call, ans = clean
    for g, n in enumerate(call.counts):
        if n == 0:
            assert ans[g] == (True, bs.ZERO128)
        else:
            blobs, cs, ps = call.group(g)
            assert ans[g][0] is True and ans[g][0] == oracle.verify_blob_kzg_proof_batch(blobs, cs, ps, oracle_settings)
        if n == 1:
            blobs, cs, ps = call.group(g)
            assert ans[g][0] == oracle.verify_blob_kzg_proof(blobs[0], cs[0], ps[0], oracle_settings)
            assert ans[g][1][:32] == bs.ONE and ans[g][1][32:80] == ps[0]         # r^0 = 1: proof_lincomb is the proof itself
    # the reversed counts cut other slices: other r's
    rev = call.reversed()
    rans = bs.answers(oracle, oracle_settings, rev)
    assert [a[0] for a in rans] == [True] * len(rev.counts)
    assert {a[1][:32] for a in rans if a[1][:32] not in (bs.ONE, bytes(32))}.isdisjoint({a[1][:32] for a in ans})


def test_the_whole_fixture_reproduces_its_recorded_intermediates(oracle, oracle_settings):
    call = bs.whole64()
    (ok, dump), = bs.answers(oracle, oracle_settings, call)
    raw = call.fx.raw
    assert ok is raw["expect"] is True
    assert (dump[:32].hex(), dump[32:80].hex(), dump[80:].hex()) == (raw["r"], raw["proof_lincomb"], raw["rhs"])


def test_spoils_change_exactly_the_groups_they_name(oracle, oracle_settings, golden_vectors, clean):
    call, ans = clean
    spoiled = bs.spoil_calls(golden_vectors, oracle)
    assert set(spoiled) == {"swapped-proofs", "modulus-last", "modulus-first", "commitment-x-above-p", "commitment-off-subgroup"}
    for name, (sc, changed) in spoiled.items():
        got = bs.answers(oracle, oracle_settings, sc)
        for g in range(len(sc.counts)):
            if g in changed:
                assert (got[g] if got[g] == "BadArgs" else got[g][0]) == changed[g], (name, g)
            else:
                assert got[g] == ans[g], (name, g)
    assert spoiled["commitment-x-above-p"][0].counts[7] == 1
    large_x, off_subgroup = bs.bad_commitments(golden_vectors, oracle)
    assert int.from_bytes(bytes([large_x[0] & 0x1F]) + large_x[1:], "big") >= bs.FP_MODULUS
    assert oracle.g1_uncompress_only(off_subgroup) == 0 and oracle.g1_validate(off_subgroup) != 0
    last = bs.modulus_in_last_element(call.fx.blob(0))
    assert int.from_bytes(last[-32:], "big") == bs.FR_MODULUS and last[:-32] == call.fx.blob(0)[:-32]


def test_set_breaks_and_device_cuts_follow_the_stated_rules():
    # a limit of 5 blobs: no two neighbours that sum above 5 share a set; the 10- and 11-blob groups are sets of their own
    live = [c for c in bs.BORDERS if c]
    assert live == [1, 2, 10, 11, 1, 6]
    assert bs.set_breaks(bs.BORDERS, 5) == [0, 2, 3, 4, 5] and bs.set_breaks(bs.BORDERS, 32768) == [0]
    # limits 1 .. 5 on the many-groups call break between every pair of neighbouring groups at least once
    nlive = sum(1 for c in bs.MANY if c)
    seen = set()
    for limit in (1, 5):
        seen |= set(bs.set_breaks(bs.MANY, limit))
    assert seen == set(range(nlive))
    # three devices, 286 blobs: borders nearest to 95.33 and 190.67 on the prefix sums
    per = bs.device_cuts(bs.MANY, 3)
    assert sum(per) == 286 and per == [94, 98, 94]
    assert bs.device_cuts([4, 4], 2) == [4, 4] and bs.device_cuts([9, 1], 2) == [9, 1] and bs.device_cuts([1, 9], 2) == [1, 9]
    assert bs.device_cuts([2, 2, 2], 2) == [2, 4]                 # 3 lies between the borders 2 and 4, equally near: the lower one
