"""The calls of the verify_blob_kzg_proof_batch_many_sets tests and their CPU answers, built without a GPU (tests/test_blob_sets_cases.py pins this
module; tests/test_gpu_blob_sets.py runs the calls).  Inputs are the committed fixtures tests/golden/batch64.json and batch512.json: blob i of a
fixture is synth.random_blob(first_index + i), with its valid commitment and proof.

A call is a list of counts over a prefix of a fixture; group g is the slice [off[g], off[g + 1]) of the three arrays.  The CPU answer of a group
is the oracle's on that slice ALONE:
    count 0        (True, 128 zero bytes)                                  kzg.rs:653-655
    count n >= 1   oracle.verify_batch_intermediates(slice): verdict, r | proof_lincomb | rhs; an OracleError is "BadArgs"
    count 1        the same, with the r field replaced by 1: the reference takes the single-proof path for one blob (kzg.rs:658-660), the
                   product takes r^0 = 1 with no hash and its read-back says so (as kzg355_debug_batch_intermediates does for n = 1); the
                   oracle's batch routine hashes a transcript of one record for its dump, whose r multiplies nothing (r^0 = 1), so
                   proof_lincomb and rhs are the same group elements either way
Answers are cached per (fixture, lo, hi, spoil) so that calls sharing a slice share its answer."""
import json
import os

from synth import random_blob

HERE = os.path.dirname(os.path.abspath(__file__))
FR_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FP_MODULUS = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
ONE = (1).to_bytes(32, "big")
ZERO128 = bytes(128)

BORDERS = [0, 1, 2, 0, 0, 10, 11, 1, 6, 0]                        # case 1: 31 blobs; 10 blobs are 62 items, 11 are 68
MANY = [(2, 3, 0, 1, 5)[g % 5] for g in range(130)]               # case 2: 286 blobs, 78 groups with a transcript
LARGE = [64, 1, 447]                                              # case 3
MINIMAL = [1, 3, 0, 2]                                            # case 7


class Fixture:
    def __init__(self, n):
        d = json.load(open(os.path.join(HERE, "golden", f"batch{n}.json")))
        self.name, self.n, self.first_index, self.raw = f"batch{n}", n, d["first_index"], d
        self.commitments = [bytes.fromhex(x) for x in d["commitments"]]
        self.proofs = [bytes.fromhex(x) for x in d["proofs"]]
        self._blobs = {}

    def blob(self, i):
        if i not in self._blobs:
            self._blobs[i] = random_blob(self.first_index + i)
        return self._blobs[i]


class ListFixture:
    """blobs, commitments and proofs given as lists (the minimal preset's, from tests/golden/minimal.json)"""

    def __init__(self, name, blobs, commitments, proofs):
        self.name, self.n, self.commitments, self.proofs, self._blobs = name, len(blobs), commitments, proofs, blobs

    def blob(self, i):
        return self._blobs[i]


_FIXTURES = {}


def fixture(n):
    if n not in _FIXTURES:
        _FIXTURES[n] = Fixture(n)
    return _FIXTURES[n]


def offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


class Call:
    """counts over blobs [0, sum(counts)) of a fixture; spoils: {blob index: (what, bytes)} replacing that blob's blob / commitment / proof"""

    def __init__(self, name, fx, counts, spoils=None):
        self.name, self.fx, self.counts, self.off = name, fx, list(counts), offsets(counts)
        self.spoils = dict(spoils or {})
        self.total = self.off[-1]
        assert self.total <= fx.n

    def item(self, i):
        b, c, p = self.fx.blob(i), self.fx.commitments[i], self.fx.proofs[i]
        for what, data in self.spoils.get(i, ()):
            if what == "blob":
                b = data
            elif what == "commitment":
                c = data
            else:
                assert what == "proof"
                p = data
        return b, c, p

    def group(self, g):
        items = [self.item(i) for i in range(self.off[g], self.off[g + 1])]
        return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]

    def groups(self):
        return [self.group(g) for g in range(len(self.counts))]

    def flat(self):
        items = [self.item(i) for i in range(self.total)]
        return b"".join(x[0] for x in items), b"".join(x[1] for x in items), b"".join(x[2] for x in items)

    def reversed(self):
        """the same blobs under the counts in reverse order (other slices, other answers)"""
        return Call(self.name + "-reversed", self.fx, self.counts[::-1], self.spoils)

    def key(self, g):
        lo, hi = self.off[g], self.off[g + 1]
        return self.fx.name, lo, hi, tuple(sorted((i, tuple(v)) for i, v in self.spoils.items() if lo <= i < hi))


_ANSWERS = {}


def group_answer(oracle, oracle_settings, call, g):
    """"BadArgs" or (verdict, 128 bytes r | proof_lincomb | rhs)"""
    from oracle.oracle import OracleError
    k = call.key(g)
    if k not in _ANSWERS:
        n = call.counts[g]
        if n == 0:
            _ANSWERS[k] = (True, ZERO128)
        else:
            try:
                d = oracle.verify_batch_intermediates(*call.group(g), oracle_settings)
                _ANSWERS[k] = (d["ok"], (ONE if n == 1 else d["r"]) + d["proof_lincomb"] + d["rhs"])
            except OracleError:
                _ANSWERS[k] = "BadArgs"
    return _ANSWERS[k]


def answers(oracle, oracle_settings, call):
    return [group_answer(oracle, oracle_settings, call, g) for g in range(len(call.counts))]


def borders():
    return Call("borders", fixture(64), BORDERS)


def many():
    return Call("many", fixture(512), MANY)


def large():
    return Call("large", fixture(512), LARGE)


def whole512():
    return Call("whole512", fixture(512), [512])


def whole64():
    return Call("whole64", fixture(64), [64])


def minimal(fx_json):
    """case 7: counts [1, 3, 0, 2] on the first six blobs of the minimal preset's fixture (FIELD_ELEMENTS_PER_BLOB = 4)"""
    h = lambda xs: [bytes.fromhex(x) for x in xs]      # noqa: E731
    return Call("minimal", ListFixture("minimal", h(fx_json["blobs"]), h(fx_json["commitments"]), h(fx_json["blob_proofs"])), MINIMAL)


def modulus_in_last_element(blob):
    return blob[:-32] + FR_MODULUS.to_bytes(32, "big")


def bad_commitments(golden_vectors, oracle):
    """(a commitment with x >= p, a commitment on the curve and off the subgroup).  The second is the reference's invalid_commitment vector that
    decodes and fails the subgroup test (tests/golden/vectors.json).  The vectors hold NO 48-byte encoding with x >= p (their other invalid
    commitments are off the curve or of the wrong length), so the first is written out: x = p itself under the compression flag."""
    cands = sorted({bytes.fromhex(c["input"]["commitment"][2:]) for c in golden_vectors["verify_blob_kzg_proof"] if "invalid_commitment" in c["name"]})
    x_of = lambda b: int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")      # noqa: E731
    off_subgroup = [b for b in cands if len(b) == 48 and x_of(b) < FP_MODULUS and oracle.g1_uncompress_only(b) == 0 and oracle.g1_validate(b) != 0]
    assert off_subgroup, len(cands)
    large_x = bytearray(FP_MODULUS.to_bytes(48, "big"))
    large_x[0] |= 0x80
    assert oracle.g1_uncompress_only(bytes(large_x)) != 0
    return bytes(large_x), off_subgroup[0]


def spoil_calls(golden_vectors, oracle):
    """case 4, on the counts of case 1: name -> (call, groups expected to differ from the clean call)"""
    base = borders()
    off = base.off
    fx = base.fx
    a, b = off[5] + 3, off[8] + 2                                  # a blob of group 5 and a blob of group 8
    large_x, off_subgroup = bad_commitments(golden_vectors, oracle)
    last6 = off[7] - 1                                             # the last blob of group 6
    first_live = off[1]                                            # the first blob of the first non-empty group (group 1)
    one_blob = off[7]                                              # the blob of group 7, a one-blob group
    return {
        "swapped-proofs": (Call("swapped-proofs", fx, BORDERS, {a: [("proof", fx.proofs[b])], b: [("proof", fx.proofs[a])]}), {5: False, 8: False}),
        "modulus-last": (Call("modulus-last", fx, BORDERS, {last6: [("blob", modulus_in_last_element(fx.blob(last6)))]}), {6: "BadArgs"}),
        "modulus-first": (Call("modulus-first", fx, BORDERS, {first_live: [("blob", modulus_in_last_element(fx.blob(first_live)))]}), {1: "BadArgs"}),
        "commitment-x-above-p": (Call("commitment-x-above-p", fx, BORDERS, {one_blob: [("commitment", large_x)]}), {7: "BadArgs"}),
        "commitment-off-subgroup": (Call("commitment-off-subgroup", fx, BORDERS, {one_blob: [("commitment", off_subgroup)]}), {7: "BadArgs"}),
    }


def set_breaks(counts, limit):
    """the launch sets of the non-empty groups under a set limit, as include/kzg355.h states the rule: whole groups in order while the set stays
    within `limit` blobs, a larger group a set of its own.  Returns the indices (among the non-empty groups) at which a new set starts."""
    live = [c for c in counts if c]
    starts, fill = [], None
    for i, c in enumerate(live):
        if fill is None or fill + c > limit:
            starts.append(i)
            fill = c
        else:
            fill += c
    return starts


def device_cuts(counts, devices):
    """the ranges of non-empty groups a handle over `devices` devices gives each device: range d ends at the group border nearest to
    d N / D on the prefix sums of the counts (the lower of two equally near).  Returns the blobs per device."""
    off = offsets([c for c in counts if c])
    total = off[-1]
    cuts = [0]
    for d in range(1, devices):
        best = min(range(len(off)), key=lambda i: (abs(off[i] * devices - d * total), i))
        cuts.append(max(best, cuts[-1]))
    cuts.append(len(off) - 1)
    return [off[cuts[d + 1]] - off[cuts[d]] for d in range(devices)]
