"""Cases of the EIP-4844 point-evaluation precompile (kzg355_point_evaluation_many and kin), built from the 92 verify_kzg_proof vectors of
tests/golden/vectors.json.  An input is versioned_hash[32] | z[32] | y[32] | commitment[48] | proof[48] with vh(C) = 0x01 || sha256(C)[1:].

  BASE      the 84 vectors whose four fields have the right lengths, as vh(C) | z | y | C | proof: the hash matches, and ok / status are the
            vector's output (true, false, or None = KZG355_BADARGS)
  MISMATCH  inputs whose hash does not match: a bit flipped in hash bytes 1..31, version byte 0x00, version byte 0x02, the hash of another
            vector's commitment -- in front of true proofs and in front of every invalid input.  Expected: KZG355_OK, false, match false,
            whatever lies behind the hash
  LENGTHS   the 8 vectors with a field one byte short or long, concatenated the same way: 191 or 193 bytes, the single call's length cases

The expectations here follow from the vectors and the EIP's wording alone; tests/test_point_eval_cases.py pins every one of them on the CPU with
hashlib and the oracle's verify_kzg_proof."""
import collections
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, BADARGS = 0, 1
INPUT_BYTES = 192
BLS_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001

# kind: "true" / "false" / "invalid" for a matching hash, "mismatch" otherwise
Case = collections.namedtuple("Case", "name kind data match ok status")


def vh(commitment):
    return b"\x01" + hashlib.sha256(commitment).digest()[1:]


def fields(data):
    """versioned_hash, z, y, commitment, proof of a 192-byte input"""
    return data[:32], data[32:64], data[64:96], data[96:144], data[144:192]


def record(data):
    """the 160-byte record C | z | y | proof that verify_kzg_proof_many_device reads"""
    _, z, y, c, p = fields(data)
    return c + z + y + p


def _unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


def _build():
    vectors = json.load(open(os.path.join(GOLDEN, "vectors.json")))["functions"]["verify_kzg_proof"]
    base, lengths = [], []
    for v in vectors:
        i = v["input"]
        c, z, y, p = (_unhex(i[k]) for k in ("commitment", "z", "y", "proof"))
        data = vh(c) + z + y + c + p
        if (len(c), len(z), len(y), len(p)) != (48, 32, 32, 48):
            lengths.append((v["name"], data))
            continue
        out = v["output"]
        kind = "true" if out is True else "false" if out is False else "invalid"
        base.append(Case(v["name"], kind, data, True, out is True, BADARGS if out is None else OK))
    trues = [c for c in base if c.kind == "true"]
    invalid = [c for c in base if c.kind == "invalid"]

    def wrong(case, tag, h):
        assert h != case.data[:32]
        return Case(case.name + "/" + tag, "mismatch", h + case.data[32:], False, False, OK)

    def flip(h, byte, bit):
        return h[:byte] + bytes([h[byte] ^ (1 << bit)]) + h[byte + 1:]

    mismatch = []
    for k, t in enumerate(trues[:6]):                              # in front of true proofs
        h = t.data[:32]
        mismatch.append(wrong(t, "bit", flip(h, 1 + (5 * k) % 31, k % 8)))
        mismatch.append(wrong(t, "v00", b"\x00" + h[1:]))
        mismatch.append(wrong(t, "v02", b"\x02" + h[1:]))
    mismatch.append(wrong(trues[0], "bit_last", flip(trues[0].data[:32], 31, 0)))
    other = next(c for c in trues if fields(c.data)[3] != fields(trues[0].data)[3])
    mismatch.append(wrong(trues[0], "other", other.data[:32]))     # the hash of another vector's commitment
    for k, t in enumerate(invalid):                                # in front of every invalid input: nothing behind the hash is looked at
        h = t.data[:32]
        mismatch.append(wrong(t, "bit", flip(h, 1 + (7 * k) % 31, (k + 3) % 8)))
    mismatch.append(wrong(invalid[0], "v00", b"\x00" + invalid[0].data[1:32]))
    mismatch.append(wrong(invalid[1], "v02", b"\x02" + invalid[1].data[1:32]))
    return base, mismatch, lengths


BASE, MISMATCH, LENGTHS = _build()
CASES = BASE + MISMATCH
BY_KIND = {k: [c for c in CASES if c.kind == k] for k in ("true", "false", "invalid", "mismatch")}


def pack(cases):
    return b"".join(c.data for c in cases)


def expected(cases):
    """ok (bool), status (int32), match (bool) arrays, and the call's return value: the first non-OK status"""
    ok = np.array([c.ok for c in cases], dtype=bool)
    st = np.array([c.status for c in cases], dtype=np.int32)
    m = np.array([c.match for c in cases], dtype=bool)
    bad = st[st != OK]
    return ok, st, m, int(bad[0]) if len(bad) else OK


def select(n, first, last):
    """n cases: one of kind `first` in front, one of kind `last` at the end (n == 1: the first alone), all of CASES in turn in between"""
    out = [CASES[(7 * i) % len(CASES)] for i in range(n)]
    out[-1] = BY_KIND[last][n % len(BY_KIND[last])]
    out[0] = BY_KIND[first][n % len(BY_KIND[first])]
    return out


def tiled(n, pins):
    """the indices into CASES of n inputs made by tiling CASES, with pins {position: kind} replaced by a case of that kind (positions >= n are dropped)"""
    idx = np.arange(n, dtype=np.int64) % len(CASES)
    for pos, kind in pins.items():
        if pos < n:
            idx[pos] = CASES.index(BY_KIND[kind][0])
    return idx


def arrays_of(idx):
    """inputs (n x 192 uint8) and the expected ok / status / match arrays for indices into CASES"""
    table = np.frombuffer(pack(CASES), dtype=np.uint8).reshape(len(CASES), INPUT_BYTES)
    ok, st, m, _ = expected(CASES)
    return np.ascontiguousarray(table[idx]), ok[idx], st[idx], m[idx]
