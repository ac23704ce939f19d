"""-m "not gpu": every expectation of tests/point_eval_cases.py pinned on the CPU -- the match flag by hashlib, ok / status of the inputs whose hash
matches by the oracle's verify_kzg_proof on the four fields, and for a mismatch the precompile's rule: false, KZG355_OK, whatever follows the hash."""
import hashlib

import point_eval_cases as pc
from oracle.oracle import OracleError


def test_the_base_cases_are_the_84_well_formed_vectors():
    kinds = [c.kind for c in pc.BASE]
    assert len(pc.BASE) == 84
    assert (kinds.count("true"), kinds.count("false"), kinds.count("invalid")) == (36, 36, 12)
    assert all(len(c.data) == pc.INPUT_BYTES and c.match for c in pc.CASES if c.kind != "mismatch")
    assert len({c.name for c in pc.CASES}) == len(pc.CASES)


def test_the_length_cases_are_191_or_193_bytes():
    assert len(pc.LENGTHS) == 8
    assert sorted({len(d) for _, d in pc.LENGTHS}) == [191, 193]


def test_every_mismatch_variant_is_there():
    tags = {c.name.rsplit("/", 1)[1] for c in pc.MISMATCH}
    assert {"bit", "bit_last", "v00", "v02", "other"} <= tags
    by_name = {c.name: c for c in pc.BASE}
    behind = [by_name[c.name.rsplit("/", 1)[0]].kind for c in pc.MISMATCH]
    assert behind.count("invalid") >= 12 and behind.count("true") >= 6          # in front of every invalid input, and in front of true proofs
    for c in pc.MISMATCH:
        h, _, _, commitment, _ = pc.fields(c.data)
        good = pc.vh(commitment)
        tag = c.name.rsplit("/", 1)[1]
        assert h != good and (c.match, c.ok, c.status) == (False, False, pc.OK)
        if tag in ("bit", "bit_last"):                             # one bit, in bytes 1..31
            diff = [i for i in range(32) if h[i] != good[i]]
            assert len(diff) == 1 and diff[0] >= 1 and bin(h[diff[0]] ^ good[diff[0]]).count("1") == 1
        elif tag in ("v00", "v02"):
            assert h[1:] == good[1:] and h[0] == int(tag[1:], 16)
        else:                                                      # a well-formed versioned hash, of another commitment
            assert h[0] == 1 and h in {pc.vh(pc.fields(b.data)[3]) for b in pc.BASE}


def test_expectations_against_hashlib_and_the_oracle(oracle, oracle_settings):
    for c in pc.CASES:
        h, z, y, commitment, proof = pc.fields(c.data)
        match = h == b"\x01" + hashlib.sha256(commitment).digest()[1:]
        assert match == c.match, c.name
        if not match:                                              # the precompile fails at the hash and reports nothing else
            assert (c.ok, c.status) == (False, pc.OK), c.name
            continue
        try:
            ok, status = oracle.verify_kzg_proof(commitment, z, y, proof, oracle_settings), pc.OK
        except OracleError:
            ok, status = False, pc.BADARGS
        assert (ok, status) == (c.ok, c.status), c.name


def test_helpers_keep_positions():
    for first, last in (("mismatch", "invalid"), ("invalid", "false"), ("false", "mismatch")):
        for n in (1, 63, 64, 65):
            sel = pc.select(n, first, last)
            assert len(sel) == n and sel[0].kind == first and (n == 1 or sel[-1].kind == last)
    idx = pc.tiled(70, {3: "mismatch", 69: "invalid", 70: "false"})
    data, ok, st, m = pc.arrays_of(idx)
    assert data.shape == (70, 192) and not m[3] and st[69] == pc.BADARGS and bytes(data[5]) == pc.CASES[5].data
    assert pc.record(pc.CASES[0].data) == pc.CASES[0].data[96:144] + pc.CASES[0].data[32:96] + pc.CASES[0].data[144:]
