"""The calls of tests/test_gpu_cell_sets.py (GPU) and tests/test_cell_sets_cases.py (CPU): lists of cell_batch_cases.Group of DIFFERENT sizes for
verify_cell_kzg_proof_batch_many_sets, built with that module's builders and pools from the CPU alone.  A Call states what it claims -- its counts,
which neighbouring groups share a commitment or a column, which group is spoiled and how -- and check_call recomputes all of it from the bytes, so
that a call cannot silently lose what it is named after.  The CPU's answer for a call is cell_batch_cases.Reference on every non-empty group,
one group at a time: that is the contract of the _sets call."""
import cell_batch_cases as bc
import cell_shard_cases as sc
import cell_spec as cs

SIDE_BY_SIDE = [1, 129, 0, 2, 257, 128, 0, 0, 3]      # k_cell_sum's second pass: side 0 at 128 | 129, side 2 at 256 | 257
MANY_SMALL = [(1, 2, 3, 0)[t % 4] for t in range(70)]
ZERO_DEBUG = bytes(176)


class Call:
    def __init__(self, name, groups, counts, share_commitment=(), share_column=(), spoiled=None):
        """share_*: pairs (g, h) of group numbers, neighbours but for empty groups between them; spoiled: {group number: how}"""
        self.name, self.groups, self.counts = name, groups, list(counts)
        self.share_commitment, self.share_column, self.spoiled = list(share_commitment), list(share_column), dict(spoiled or {})


def empty(tag):
    return bc.Group(f"empty-{tag}", [], "valid", distinct=0, first=[], columns={})


def cut(pools, name, first, n, pool="mixed"):
    """n consecutive items of a pool from item `first` on (wrapping around)"""
    p = getattr(pools, pool)
    return bc.planned(name, p, [(first + t) % len(p) for t in range(n)])


def neighbours(call):
    live = [t for t, g in enumerate(call.groups) if g.n]
    return list(zip(live, live[1:]))


def check_call(call):
    assert [g.n for g in call.groups] == call.counts, call.name
    assert len({g.name for g in call.groups}) == len(call.groups), call.name
    for g in call.groups:
        bc.check_claims(g)
    near = neighbours(call)
    for a, b in near:                                             # the cross-border claims: exactly the stated neighbours share something
        ga, gb = call.groups[a], call.groups[b]
        assert bool(set(ga.c) & set(gb.c)) == ((a, b) in call.share_commitment), (call.name, a, b)
        if (a, b) in call.share_column:
            assert set(ga.i) & set(gb.i), (call.name, a, b)
    assert set(call.share_commitment) <= set(near) and set(call.share_column) <= set(near), call.name
    kinds = {t: g.kind for t, g in enumerate(call.groups) if g.kind != "valid"}
    assert set(kinds) == set(call.spoiled), (call.name, kinds)


def side_by_side(pools):
    layouts = ["mixed", "mixed", None, "columns", "columns", "columns", None, None, "mixed"]
    groups = [bc.distinct_group(pools, n, lay) if n else empty(t) for t, (n, lay) in enumerate(zip(SIDE_BY_SIDE, layouts))]
    # groups of one pool are cut from its start: a smaller one's commitments are all in the larger one beside it
    return Call("side-by-side", groups, SIDE_BY_SIDE, share_commitment=[(0, 1), (3, 4), (4, 5)], share_column=[(0, 1), (3, 4), (4, 5)])


def empty_ends(pools):
    return Call("empty-ends", [empty("a"), cut(pools, "five", 50, 5), empty("b")], [0, 5, 0])


def all_empty():
    return Call("all-empty", [empty(t) for t in "abc"], [0, 0, 0])


def borders(pools):
    """group 0 ends with commitment X on column c, group 1 begins with X on column c and repeats it twice; then "two" and "half" dedup groups
    of different sizes, whose infinity padding slots (n - distinct of them) sit beside the live slots of the next group"""
    a = bc.planned("border-a", pools.mixed, [30, 31, 32, 40])
    b = bc.planned("border-b", pools.mixed, [40, 41, 40, 42, 40])
    groups = [a, b, bc.dedup_group(pools, 7, "two"), bc.dedup_group(pools, 10, "half"), bc.dedup_group(pools, 4, "two"), bc.dedup_group(pools, 5, "half")]
    call = Call("borders", groups, [4, 5, 7, 10, 4, 5], share_commitment=[(0, 1), (2, 3), (3, 4)], share_column=[(0, 1)])
    assert (a.c[-1], a.i[-1]) == (b.c[0], b.i[0]) and b.c.count(b.c[0]) == 3
    assert [g.n - g.distinct for g in groups] == [0, 2, 5, 5, 2, 3]
    return call


def bad_commitment(g, j, point):
    """g with the commitment of item j (which appears once) replaced by a point that fails validate_kzg_g1"""
    assert g.c.count(g.c[j]) == 1 and point not in g.c
    items = g.items()
    first = [point if c == g.c[j] else c for c in g.first]
    items[j] = (point,) + items[j][1:]
    return bc.Group(f"{g.name}-badcommitment{j}", items, "malformed", distinct=g.distinct, first=first, columns=g.columns)


STATUS_SIZES = [3, 4, 5, 2, 6]
STATUS_SIZES_LARGE = [3, 200, 300, 5, 7]      # 515 cells: more than the 1024 points up to which the subgroup test runs four lanes per point


def status_calls(pools, not_in_subgroup, off_curve):
    """five-group calls in which exactly one thing is wrong, at the last cell of group 1 or the first cell of group 2"""
    def base(sizes, tag):
        firsts = [sum(sizes[:t]) for t in range(len(sizes))]
        return [cut(pools, f"st{tag}{t}", 60 + firsts[t], n) for t, n in enumerate(sizes)]
    small = base(STATUS_SIZES, "s")
    large = base(STATUS_SIZES_LARGE, "l")
    last, calls = STATUS_SIZES[1] - 1, []

    def one(name, groups, at, new, also=None, counts=STATUS_SIZES, share=()):
        gs = list(groups)
        new.name = f"{name}/{new.name}"                           # (the builders name a group after its parent and the cell alone)
        gs[at] = new
        spoiled = {at: "malformed"}
        if also is not None:                                      # a well-formed False group between True ones
            gs[also] = bc.spoil(gs[also], "cell", 0)
            spoiled[also] = "spoiled"
        calls.append(Call(name, gs, counts, share_commitment=share, spoiled=spoiled))
    one("proof-last-of-1", small, 1, sc.with_item(small[1], last, "malformed", proof=not_in_subgroup), also=3)
    one("proof-first-of-2", small, 2, sc.with_item(small[2], 0, "malformed", proof=not_in_subgroup))
    one("proof-first-of-2-large", large, 2, sc.with_item(large[2], 0, "malformed", proof=not_in_subgroup), counts=STATUS_SIZES_LARGE,
        share=[(1, 2), (2, 3)])                                   # (its 300-cell group holds the whole pool once)
    one("proof-off-curve-last-of-1", small, 1, sc.with_item(small[1], last, "malformed", proof=off_curve))
    one("commitment-last-of-1", small, 1, bad_commitment(small[1], last, off_curve))
    one("commitment-first-of-2", small, 2, bad_commitment(small[2], 0, not_in_subgroup))
    one("element-r-last-of-1", small, 1, sc.with_item(small[1], last, "malformed", cell=sc.noncanonical(small[1].cells[last])))
    one("element-r-first-of-2", small, 2, sc.with_item(small[2], 0, "malformed", cell=sc.noncanonical(small[2].cells[0])))
    one("index-128-last-of-1", small, 1, bc.malformed_index(small[1], last))
    one("index-128-first-of-2", small, 2, bc.malformed_index(small[2], 0), also=0)
    return calls


def uniform(pools):
    return Call("uniform", [cut(pools, f"uni{t}", 5 * t, 5) for t in range(4)], [5] * 4)


def many_small(pools):
    groups, at = [], 0
    for t, n in enumerate(MANY_SMALL):
        groups.append(cut(pools, f"small{t}", at, n) if n else empty(t))
        at += n
    return Call("many-small", groups, MANY_SMALL)


def two_groups(pools):
    return Call("two-groups", [cut(pools, "pair0", 200, 4), cut(pools, "pair1", 204, 7)], [4, 7])


def cpu_answer(reference, g):
    """the contract of the _sets call for one group: (verdict or "BadArgs", 176 debug bytes or None)"""
    if g.n == 0:
        return True, ZERO_DEBUG
    try:
        r, itau, ll, rl, ok = reference(*g.args)
    except cs.BadArgs:
        return "BadArgs", None
    return ok, r + itau + ll + rl

