"""Inputs shared by tests/test_gpu_blob_cell_sets.py (GPU) and tests/test_blob_cell_sets_cases.py (CPU): calls of
verify_blob_cell_proofs_batch_many_sets -- lists of groups of whole blobs, every group with its own blob count -- built from the groups of
tests/blob_cell_shape_cases.py (Pools, planned, distinct_group, the spoilings; nothing here calls the library under test).  A call is a list of
Group; flat() lays it out as the C ABI takes it (the three arrays group after group with no padding, and the counts) and slices() cuts such arrays
by the counts again.  The CPU's answer of a group is the answer for that group ALONE: blob_cell_shape_cases.expected, that is
cell_spec.verify_cell_kzg_proof_batch over its 128 n cells; an empty group is True with zero debug bytes.

The groups are small and named, so that a test module computes each CPU answer once per name (0.1 s a blob) however many calls use the group:
  distinct1@14, distinct1@15, distinct1@16     one mixture blob each
  distinct2@9, two-AA, two-x64-mix, two-mix-zero     two blobs: distinct, one commitment twice, X^64 and a mixture, a mixture and the zero blob
  distinct3@4, three-ABA       three blobs = 384 cells: k_cell_sum's second pass
  dedup-ABAC, dedup-kinds      four blobs; dedup-kinds has the commitment at infinity in slot 1
  share-AB, share-A, share-BAA (and the same with B the zero blob: zshare-...)   groups of ONE call that share commitments
Blobs within a group differ, and so do the groups of a call (but for the share-* calls, whose point is that they do not).  Spoils and
malformations sit in the LAST blob of their group.

CALLS, by the boundary each crosses (counts; the launch set's blob total decides the interpolation route: columns up to 6, coefficients above):
  offsets-7 (1, 3, 0, 2, 1), offsets-3 (2, 0, 1), route-6 (1, 2, 3), route-7 (1, 2, 4), largest-first (4, 1, 1), largest-last (1, 1, 4),
  shared (2, 1, 3), shared-zero (2, 1, 3), statuses (2, 3, 1, 2, 4): False, BadArgs, True, True, BadArgs, hash-2 (2, 1), hash-3 (3, 1, 2),
  uniform (2, 2, 2, 2), replicas-5 (1, 0, 3, 2, 0, 4, 1), replicas-2 (0, 2, 1), shrink (1, 2) after grow's (4, 3, 2, 1), all-empty (0, 0, 0)
chunked(): 898 groups, 2050 blobs: distinct1@16, then 128 times the cycle 1, 2, 3, 4, 2, 1, 3 (16 blobs), then distinct1@14 -- the last group
of the last cycle is blobs 2046 .. 2048, so it would straddle blob 2048 and opens the second launch set, which distinct1@14 shares with it."""
import blob_cell_shape_cases as sc
import cell_device_cases as dcases

N = sc.N
EMPTY_ANSWER = (bytes(176), True)


def empty():
    return sc.planned("empty", [], [])


def named_groups(pools):
    """{name: Group}: every group the calls are made of"""
    out = {}

    def add(*gs):
        for g in gs:
            assert g.name not in out, g.name
            out[g.name] = g
    add(empty())
    add(*[sc.distinct_group(pools, 1, 14 + t) for t in range(3)])
    add(*sc.launch_set_groups(pools, 2, 4))
    add(*sc.launch_set_groups(pools, 3, 2))
    add(sc.dedup_group(pools, "ABAC"), sc.dedup_group(pools, "kinds"))
    for tag, b in (("share", pools.mix(1)), ("zshare", pools.low("zero"))):
        ab = [pools.mix(0), b]
        add(sc.planned(f"{tag}-AB", ab, [0, 1]), sc.planned(f"{tag}-A", ab, [0]), sc.planned(f"{tag}-BAA", ab, [1, 0, 0]))
    # spoils and malformations, each in the last blob of its group
    add(sc.spoil_element(out["distinct2@9"], 1, 4095), sc.malformed_element(out["three-ABA"], 2, 2077),
        sc.malformed_proof(out["dedup-ABAC"], 3, 127, dcases.off_curve(pools.o)))
    return out


CALLS = {
    "offsets-7": ("distinct1@14", "distinct3@4", "empty", "two-AA", "distinct1@15"),
    "offsets-3": ("distinct2@9", "empty", "distinct1@16"),
    "route-6": ("distinct1@14", "two-x64-mix", "three-ABA"),
    "route-7": ("distinct1@14", "two-mix-zero", "dedup-ABAC"),
    "largest-first": ("dedup-kinds", "distinct1@14", "distinct1@15"),
    "largest-last": ("distinct1@15", "distinct1@16", "dedup-ABAC"),
    "shared": ("share-AB", "share-A", "share-BAA"),
    "shared-zero": ("zshare-AB", "zshare-A", "zshare-BAA"),
    "statuses": ("distinct2@9-element1.4095", "three-ABA-element2.2077=r", "distinct1@14", "two-x64-mix", "dedup-ABAC-proof3.127-off-curve"),
    "hash-2": ("two-AA", "distinct1@14"),
    "hash-3": ("three-ABA", "distinct1@15", "two-mix-zero"),
    "uniform": ("distinct2@9", "two-AA", "two-x64-mix", "two-mix-zero"),
    "replicas-5": ("distinct1@14", "empty", "distinct3@4", "two-AA", "empty", "dedup-ABAC", "distinct1@15"),
    "replicas-2": ("empty", "two-AA", "distinct1@14"),
    "grow": ("dedup-kinds", "distinct3@4", "two-x64-mix", "distinct1@16"),
    "shrink": ("distinct1@15", "distinct2@9"),
    "all-empty": ("empty", "empty", "empty"),
}
COUNTS = {
    "offsets-7": (1, 3, 0, 2, 1), "offsets-3": (2, 0, 1), "route-6": (1, 2, 3), "route-7": (1, 2, 4), "largest-first": (4, 1, 1),
    "largest-last": (1, 1, 4), "shared": (2, 1, 3), "shared-zero": (2, 1, 3), "statuses": (2, 3, 1, 2, 4), "hash-2": (2, 1), "hash-3": (3, 1, 2),
    "uniform": (2, 2, 2, 2), "replicas-5": (1, 0, 3, 2, 0, 4, 1), "replicas-2": (0, 2, 1), "grow": (4, 3, 2, 1), "shrink": (1, 2),
    "all-empty": (0, 0, 0),
}
STATUSES_KINDS = ("spoiled", "malformed", "valid", "valid", "malformed")
CHUNK_CYCLE = ("distinct1@14", "distinct2@9", "distinct3@4", "dedup-ABAC", "two-AA", "distinct1@15", "three-ABA")
CHUNK_CYCLES = 128
CHUNK_BLOBS = 2048                                               # blobs per launch set (BLOB_CELLS_MAX_BLOBS)


def call(named, name):
    gs = [named[k] for k in CALLS[name]]
    assert counts(gs) == list(COUNTS[name]), name
    return gs


def chunked(named):
    gs = [named["distinct1@16"]] + [named[k] for k in CHUNK_CYCLE] * CHUNK_CYCLES + [named["distinct1@14"]]
    off = offsets(counts(gs))
    assert sum(named[k].n for k in CHUNK_CYCLE) == 16 and off[-1] == CHUNK_BLOBS + 2 and len(gs) == 898
    # the group that would straddle the border opens the second launch set
    assert off[-3] < CHUNK_BLOBS < off[-2] and gs[-2].name == "three-ABA" and off[-2] - off[-3] == 3
    return gs


def counts(groups):
    return [g.n for g in groups]


def offsets(cnts):
    off = [0]
    for c in cnts:
        off.append(off[-1] + c)
    return off


def flat(groups):
    """(blobs, commitments, cell_proofs, counts): the three lists group after group with no padding, as the `_sets` ABI takes them"""
    return ([b for g in groups for b in g.blobs], [c for g in groups for c in g.c], [p for g in groups for p in g.p], counts(groups))


def slices(blobs, commitments, cell_proofs, cnts):
    """the (blobs, commitments, cell_proofs) of every group, cut from flat arrays by the counts: group g is blobs [boff_g, boff_g + counts[g]),
    the same commitments and proofs [128 boff_g, 128 (boff_g + counts[g]))"""
    off = offsets(cnts)
    assert len(blobs) == len(commitments) == off[-1] and len(cell_proofs) == N * off[-1]
    return [(blobs[off[g]:off[g + 1]], commitments[off[g]:off[g + 1]], cell_proofs[N * off[g]:N * off[g + 1]]) for g in range(len(cnts))]


def answer(o, fx, g):
    """the CPU's answer for the group alone: (176 bytes, verdict), or "BadArgs\""""
    if g.n == 0:
        return EMPTY_ANSWER
    try:
        return sc.expected(o, fx, g)
    except sc.cs.BadArgs:
        return "BadArgs"
