"""-m "not gpu": the call layouts of tests/test_gpu_cells_at_layouts.py (tests/cells_at_layout_cases.py) pinned on the CPU.  The chunk model
gives the launch sets the layouts were made for with CQ_CHUNK and CC_CHUNK as engine.h has them -- a change of either fails here instead of
silently taking the borders out from under the GPU tests --; the fuzz seeds hold what they were chosen for; the answer model agrees with the
fixture slot by slot; statuses and slots follow the counts as given; and every refused unit is refused for its stated reason and for no
other, by recover_spec / cell_spec where they have the rule."""
import random

import pytest

import cell_spec as cs
import cells_at_layout_cases as lay
import recover_at_cases as rc
import recover_spec as rs

MSM_NAMES = ["msm_%d" % t for t in lay.MSM_TOTALS]
ALL = [(call, name) for call in lay.CALLS for name in list(lay.NAMED) + MSM_NAMES]


def every_call():
    for call, name in ALL:
        yield "%s %s" % (call, name), call, lay.layout(call, name)
    for call in lay.CALLS:
        for seed in lay.FUZZ_SEEDS[call]:
            yield "%s fuzz %d" % (call, seed), call, lay.fuzz(call, seed)
        for middle in ("ragged", "refused_at_border"):
            yield "%s replicas %s" % (call, middle), call, lay.replicas_call(call, middle)


def test_constants_are_those_the_layouts_were_made_for():
    assert (lay.CQ_CHUNK, lay.CC_CHUNK) == (1152, 512)


@pytest.mark.parametrize("call", lay.CALLS)
def test_named_layouts_split_as_stated(call):
    counts = lambda name: [len(u.want) for u in lay.layout(call, name)]      # noqa: E731
    kinds = lambda name: ["H" if u.host else "D" if u.refusal else "" for u in lay.layout(call, name)]      # noqa: E731
    assert counts("ragged") == [128] * 8 + [100, 60, 5, 0, 128, 1] and set(kinds("ragged")) == {""}
    assert counts("riders") == [128] * 8 + [127, 1, 0, 0, 1, 3] and kinds("riders") == [""] * 11 + ["D", "", ""]
    assert counts("refused_at_border") == [128] * 8 + [120, 129, 8, 3, 5, 7, 0, 2]
    assert kinds("refused_at_border") == [""] * 9 + ["H", "", "H", "D", "", "", ""]
    ub = lay.layout(call, "unit_border")
    assert len(ub) == 516 and [i for i, u in enumerate(ub) if u.refusal] == [0, 511, 512, 515]
    assert all(u.host and len(u.want) == 2 if u.refusal else len(u.want) == i % 3 for i, u in enumerate(ub))
    assert counts("empty_chunk_first") == [0] * 512 + [3] and set(kinds("empty_chunk_first")) == {""}
    for name in lay.NAMED:
        chunks = lay.split(lay.layout(call, name))
        assert [c[1:] for c in chunks] == lay.CHUNKS[name], name
        assert [c[0] for c in chunks] == [0, chunks[0][1]], name
    assert lay.CHUNKS == {"ragged": [(9, 1124, 1124), (5, 194, 194)], "riders": [(12, 1152, 1152), (2, 4, 4)],
                          "refused_at_border": [(12, 1152, 1284), (4, 14, 14)], "unit_border": [(512, 510, 514), (4, 1, 5)],
                          "empty_chunk_first": [(512, 0, 0), (1, 3, 3)]}
    # a refused unit at every side of a border: last in a launch set, first in one (the host's refusal only behind CC_CHUNK units), and the
    # device's refusal first in one
    rab = lay.layout(call, "refused_at_border")
    assert rab[11].host and rab[12].refusal == lay.DEVICE and ub[511].host and ub[512].host and lay.refused_at_the_border(rab)
    assert lay.layout(call, "riders")[11].refusal == lay.DEVICE
    assert len({u.refusal for name in lay.NAMED for u in lay.layout(call, name) if u.host}) == len(lay.HOST_KINDS[call])


@pytest.mark.parametrize("call", lay.CALLS)
def test_msm_borders_are_single_launch_sets_of_the_stated_pairs(call):
    assert lay.MSM_TOTALS == (15, 16, 127, 128, 1023, 1024)
    for total in lay.MSM_TOTALS:
        units = lay.layout(call, "msm_%d" % total)
        assert len(units) >= 3 and not any(u.refusal for u in units), total
        assert lay.split(units) == [(0, len(units), total, total)], total


@pytest.mark.parametrize("call", lay.CALLS)
def test_fuzz_seeds_hold_what_they_were_chosen_for(call):
    seeds = lay.FUZZ_SEEDS[call]
    assert len(set(seeds)) == 8
    all_units = [lay.fuzz(call, s) for s in seeds]
    for units in all_units:
        assert 1 <= len(units) <= 24
        for u in units:
            assert len(u.want) in lay.FUZZ_COUNTS or u.refusal in ("count of 129", "129 wanted"), u
    assert sum(len(lay.split(units)) == 2 for units in all_units) >= 3
    assert sum(lay.refused_at_the_border(units) for units in all_units) >= 1
    assert max(len(lay.split(units)) for units in all_units) == 2
    kinds = {u.refusal for units in all_units for u in units if u.refusal}
    assert lay.DEVICE in kinds and len(kinds) >= 3
    n = sum(len(units) for units in all_units)
    assert n / 12 < sum(1 for units in all_units for u in units if u.refusal) < n / 3      # about one in six


def test_replica_ranges_run_in_two_launch_sets_each():
    assert lay.ranges(5, 3) == [(0, 1), (1, 2), (3, 2)] and lay.ranges(2, 3) == [(0, 1), (1, 1)]      # (what the existing replicas tests state)
    for call in lay.CALLS:
        units = lay.replicas_call(call, "ragged")
        assert len(units) == 44 and [len(units[0].want), len(units[-1].want)] == [3, 9]
        assert lay.ranges(44, 3) == [(0, 14), (14, 15), (29, 15)]
        for lo, n in lay.ranges(44, 3):
            assert len(lay.split(units[lo:lo + n])) == 2, lo
        units = lay.replicas_call(call, "refused_at_border")
        assert len(units) == 46 and lay.ranges(46, 3) == [(0, 15), (15, 15), (30, 16)]
        for lo, n in lay.ranges(46, 3):
            assert len(lay.split(units[lo:lo + n])) == 2, lo
        mid = units[15:30]
        assert mid == lay.layout(call, "refused_at_border")[:15] and lay.refused_at_the_border(mid)      # the middle range holds all its refusals


def test_expected_agrees_with_the_fixture_on_sampled_slots():
    fx = rc.fixture()
    assert fx["cells"][1] == cs.compute_cells(fx["blobs"][1])
    rng = random.Random(2048)
    for label, call, units in every_call():
        statuses, c, p, holes = lay.expected(units)
        owner = [(i, k) for i, u in enumerate(units) for k in u.want]      # of every slot: (unit, wanted index)
        assert len(c) == lay.CELL * len(owner) and len(p) == 48 * len(owner), label
        refused_slots = {s for lo, hi in holes for s in range(lo, hi)}
        assert refused_slots == {s for s, (i, _) in enumerate(owner) if units[i].refusal}, label
        for s in [0, len(owner) - 1] + [rng.randrange(len(owner)) for _ in range(12)]:
            i, k = owner[s]
            assert units[i].b == i % 3 or "replicas" in label, label
            if units[i].refusal:
                continue
            assert c[lay.CELL * s:lay.CELL * (s + 1)] == fx["cells"][units[i].b][k], (label, s)
            assert p[48 * s:48 * (s + 1)] == bytes.fromhex(fx["proofs"][units[i].b][k]), (label, s)
        assert lay.blank(c, holes, lay.CELL) == c and lay.blank(bytes([7]) * len(p), holes, 48).count(0) == 48 * len(refused_slots), label


def test_statuses_and_slots_follow_the_counts_as_given():
    for label, call, units in every_call():
        statuses, c, p, holes = lay.expected(units)
        assert statuses == [lay.BADARGS if u.refusal else 0 for u in units], label
        data, kc, ki, wc, wi = lay.call_arrays(call, units)
        assert wc == [len(u.want) for u in units] and sum(wc) == len(wi) == len(c) // lay.CELL == len(p) // 48, label
        assert sum(s for _, _, _, s in lay.split(units)) == sum(wc) and sum(m for _, m, _, _ in lay.split(units)) == len(units), label
        if call == "compute":
            assert (kc, ki) == (None, None) and len(data) == lay.BLOB * len(units), label
        else:
            assert sum(kc) == len(ki) and len(data) == lay.CELL * len(ki), label
            if len(units) > 100:
                assert set(kc) <= {63, 64, 129}, label                # hundreds of units bring 64 known cells each
            elif len(units) >= 14 and "fuzz" not in label:
                assert len({u.known for u in units if not u.refusal}) >= 8, label      # neighbours differ in blob, set and wants


def canonical(data):
    return all(int.from_bytes(data[32 * i:32 * i + 32], "big") < lay.R for i in range(len(data) // 32))


def test_every_refused_unit_is_refused_for_its_stated_reason_alone():
    fx = rc.fixture()
    seen = {call: set() for call in lay.CALLS}
    for label, call, units in every_call():
        for u in units:
            want_ok = len(u.want) <= 128 and all(k < 128 for k in u.want)
            if call == "compute":
                blob = lay.blob_of(u)
                data_ok, lists_ok = blob == fx["blobs"][u.b], True
                if not data_ok:
                    assert not canonical(blob) and sum(a != b for a, b in zip(blob, fx["blobs"][u.b])) <= 32, label
            else:
                cells = lay.known_cells_of(u)
                assert len(cells) == len(u.known), label
                lists_ok = True
                try:
                    rs.check_indices(u.known)
                except cs.BadArgs as e:
                    lists_ok = False
                    assert str(e) == {"63 known cells": "number of cells", "129 known cells": "number of cells",
                                      "known indices not ascending": "cell indices not strictly ascending"}[u.refusal], label
                data_ok = cells == [fx["cells"][u.b][k % 128] for k in u.known]
                if not data_ok:
                    at, _ = u.spoil
                    with pytest.raises(cs.BadArgs, match="non-canonical"):
                        cs.cell_values(cells[at])
            assert [lists_ok, data_ok, want_ok].count(False) == (1 if u.refusal else 0), (label, u.refusal)
            if u.refusal:
                assert {"count of 129": not want_ok and len(u.want) == 129, "129 wanted": not want_ok and len(u.want) == 129,
                        "wanted index 128": not want_ok and 128 in u.want and len(u.want) <= 128, lay.DEVICE: not data_ok}.get(u.refusal, not lists_ok)
                assert u.host == (u.refusal != lay.DEVICE)
                seen[call].add(u.refusal)
    for call in lay.CALLS:
        assert seen[call] == set(lay.HOST_KINDS[call]) | {lay.DEVICE}, call
