"""The lazy G1 chain arithmetic of kzg_rust_amd/csrc (field.h: fp_mulsqr2_lz, fp_mul2_lz; g1.h: g1_dbl_lazy, g1_add_lazy, g1_add_lazy2,
g1x_add_lazy2, g1_in_subgroup, g1_decompress) compiled for the HOST (tests/native/lazy_chain_probe.cpp) and checked against Python big
integers.  The probe takes RAW limbs, so the operands sit at the bounds the callers really pass: values of up to 32p with the excess in the
top limb, all-ones lower limbs, lazy zeros (k p).  Runs without a GPU (-m "not gpu"); the same source runs on the device."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
LB, N = 29, 14
MONT_R = 1 << (LB * N)
MONT_RINV = pow(MONT_R, -1, P)
LOW = (1 << (LB * (N - 1))) - 1          # the thirteen lower limbs, all ones
Limbs = C.c_uint32 * N


@pytest.fixture(scope="module")
def lcp():
    src = os.path.join(NATIVE, "lazy_chain_probe.cpp")
    so = os.path.join(NATIVE, "liblazy_chain_probe.so")
    csrc = os.path.join(HERE, "..", "kzg_rust_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("field.h", "g1.h", "modinv.h", "consts_gen.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    return C.CDLL(so)


# ------------------------------------------------------------------------------------------------ limbs and curve arithmetic in Python
def to_limbs(v, n=1):
    """n values -> one ctypes array; 29-bit limbs, the top limb keeps the excess (a normalised lazy value)."""
    vs = [v] if isinstance(v, int) else list(v)
    out = []
    for x in vs:
        assert 0 <= x and (x >> (LB * (N - 1))) < (1 << 32)
        out += [(x >> (LB * i)) & ((1 << LB) - 1) for i in range(N - 1)] + [x >> (LB * (N - 1))]
    return (C.c_uint32 * len(out))(*out)


def from_limbs(a, k=0):
    return sum(int(a[N * k + i]) << (LB * i) for i in range(N))


def normalised(a, k=0):
    return all(int(a[N * k + i]) < (1 << LB) for i in range(N - 1))


def mont(v):
    return v * MONT_R % P


def unmont(v):
    return v * MONT_RINV % P


def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def ec_mul(k, a):
    r = None
    for bit in bin(k)[2:]:
        r = ec_add(r, r)
        if bit == "1":
            r = ec_add(r, a)
    return r


def jac_of(pt, z, ks=(0, 0, 0)):
    """Affine point -> lazy Montgomery Jacobian coordinates (x z^2, y z^3, z), coordinate i lifted by ks[i] multiples of p."""
    x, y = pt
    return [mont(x * z * z % P) + ks[0] * P, mont(y * z * z * z % P) + ks[1] * P, mont(z) + ks[2] * P]


def affine_of_jac(vals):
    X, Y, Z = (unmont(v % P) for v in vals)
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def curve_point(rng):
    while True:
        x = rng.randrange(P)
        y2 = (x * x * x + 4) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            return x, y


G = (GX, GY)
ORDER3 = (0, 2)                                                   # y^2 = 4: a point of order 3, outside the subgroup


def test_the_python_side_is_sound():
    assert (GY * GY - GX ** 3 - 4) % P == 0 and ec_mul(R_ORDER, G) is None
    assert ec_mul(3, ORDER3) is None and ec_add(ORDER3, ORDER3) is not None


# ------------------------------------------------------------------------------------------------ the new primitive
def _mulsqr2_operands():
    rng = random.Random(0x5152)
    # bounds of the doubling: a = E (stated < 6p), b = X3 - D + 4p (< 15.01p: 16p taken), c = 2B (8B < 16p  <=>  2B < 4p)
    ba, bb, bc = 6 * P, 16 * P, 4 * P
    cases = [(ba - 1, bb - 1, bc - 1), (0, 0, 0), (ba - 1, 0, bc - 1), (0, bb - 1, 0), (1, 1, 1), (P, P, P), (P - 1, P + 1, 2 * P)]
    # all-ones lower limbs with the largest top limb that keeps the value inside its bound, and top-limb excess alone
    top = lambda bound: ((bound - LOW - 1) >> (LB * (N - 1))) << (LB * (N - 1))
    cases.append((top(ba) + LOW, top(bb) + LOW, top(bc) + LOW))
    cases.append((top(ba), top(bb), top(bc)))
    cases.append((LOW, LOW, LOW))
    for _ in range(200):
        cases.append((rng.randrange(ba), rng.randrange(bb), rng.randrange(bc)))
    for _ in range(50):                                           # k p + small, k p - small: residues next to 0 under every lift
        k = [rng.randrange(1, 6), rng.randrange(1, 16), rng.randrange(1, 4)]
        d = [rng.randrange(-3, 4) for _ in range(3)]
        cases.append(tuple(ki * P + di for ki, di in zip(k, d)))
    return cases


def test_mulsqr2_matches_big_integers_at_the_callers_bounds(lcp):
    out = Limbs()
    for a, b, c in _mulsqr2_operands():
        lcp.lcp_mulsqr2(out, to_limbs(a), to_limbs(b), to_limbs(c))
        v = from_limbs(out)
        t = a * b + 2 * c * c
        # exactly (t + q p) / R for a q in [0, R): the Montgomery quotient, whatever the lifts of the operands
        num = v * MONT_R - t
        assert num >= 0 and num % P == 0 and num // P < MONT_R, (hex(a), hex(b), hex(c))
        assert v * MONT_R % P == t % P
        assert normalised(out) and v < P + (P >> 13), hex(v)     # lazy result: below p (1 + 2^-13), limbs below the top one < 2^29


def test_mul2_at_the_bounds_of_the_fused_y3(lcp):
    """Y3 = R (V - X3) + (2p - S1) HHH of the lazy additions under one reduction: R < 4p, V - X3 + 8p < 10p, 2p - S1 <= 2p, HHH < 2p."""
    rng = random.Random(0x5153)
    out = Limbs()
    bounds = (4 * P, 10 * P, 2 * P + 1, 2 * P)
    cases = [tuple(b - 1 for b in bounds)] + [tuple(rng.randrange(b) for b in bounds) for _ in range(100)]
    for a, b, c, d in cases:
        lcp.lcp_mul2(out, to_limbs(a), to_limbs(b), to_limbs(c), to_limbs(d))
        v = from_limbs(out)
        num = v * MONT_R - (a * b + c * d)
        assert num >= 0 and num % P == 0 and num // P < MONT_R
        assert normalised(out) and v < P + (P >> 13)


# ------------------------------------------------------------------------------------------------ the doubling
def _dbl_inputs():
    rng = random.Random(0x5154)
    pts = [G, ec_mul(5, G), ORDER3] + [curve_point(rng) for _ in range(6)]
    ins = []
    for i, pt in enumerate(pts):
        z = rng.randrange(1, P)
        ins.append((pt, jac_of(pt, z)))                                                 # canonical coordinates
        ins.append((pt, jac_of(pt, z, (31, 31, 31))))                                   # every coordinate at the top of its input bound (< 32p)
        ins.append((pt, jac_of(pt, 1, (rng.randrange(32), rng.randrange(32), rng.randrange(32)))))
    # coordinates whose residues sit next to 0 and p under the largest lift, and all-ones lower limbs
    ins.append((None, [31 * P + 5, 31 * P + 7, 31 * P]))                                # infinity as a lazy zero: Z = 31p
    ins.append((None, [mont(3), mont(9), 0]))                                           # infinity with all-zero Z
    ins.append((None, [0, 0, 0]))
    return ins


def _run_dbl(lcp, vals, k):
    raw, canon, ref = (C.c_uint32 * (3 * N))(), (C.c_uint32 * (3 * N))(), (C.c_uint32 * (3 * N))()
    lcp.lcp_dbl_chain(raw, canon, ref, to_limbs(vals), k)
    return raw, canon, ref


@pytest.mark.parametrize("k", [1, 2, 126])
def test_dbl_lazy_against_the_canonical_addition_and_python(lcp, k):
    for pt, vals in _dbl_inputs():
        assert all(v < 32 * P for v in vals)
        raw, canon, ref = _run_dbl(lcp, vals, k)
        rv = [from_limbs(raw, i) for i in range(3)]
        # the stated output contract, on the raw chain value: X < 12p, Y <= 2p, Z < 3p (inside the former 26p / 18p / 4p), limbs normalised
        assert rv[0] < 12 * P and rv[1] <= 2 * P and rv[2] < 3 * P and all(normalised(raw, i) for i in range(3))
        cv = [from_limbs(canon, i) for i in range(3)]
        assert all(v < P for v in cv)
        want = ec_mul(1 << k, pt) if pt is not None else None
        assert affine_of_jac(cv) == want                                                # Python's [2^k] P
        if want is None:
            assert cv[2] == 0 and rv[2] % P == 0                                        # infinity comes out as Z = 0 mod p
        else:
            assert list(canon) == list(ref)                                             # the same field elements as g1_add(P, P), k times


def test_dbl_lazy_chain_on_a_point_of_order_three(lcp):
    """2 T = -T for a point of order 3: a chain of 126 doublings alternates between the point and its negative and ends on T (2^126 = 1 mod 3)."""
    raw, canon, ref = _run_dbl(lcp, jac_of(ORDER3, 7, (31, 0, 31)), 126)
    assert affine_of_jac([from_limbs(canon, i) for i in range(3)]) == ec_mul(1 << 126, ORDER3) == ORDER3


# ------------------------------------------------------------------------------------------------ the additions with the fused Y3
def test_lazy_additions_against_python(lcp):
    rng = random.Random(0x5155)
    out = (C.c_uint32 * (3 * N))()
    outx = (C.c_uint32 * (4 * N))()
    for it in range(24):
        a, b = curve_point(rng), curve_point(rng)
        want = ec_add(a, b)
        za, zb = rng.randrange(1, P), rng.randrange(1, P)
        top = it % 3 == 0
        # g1_add_lazy: a lazy (X, Y, Z < 32p), b canonical
        ja = jac_of(a, za, (31, 31, 31) if top else tuple(rng.randrange(32) for _ in range(3)))
        lcp.lcp_add_lazy(out, to_limbs(ja), to_limbs(jac_of(b, zb)), 0)
        rv = [from_limbs(out, i) for i in range(3)]
        assert affine_of_jac(rv) == want and rv[0] < 8 * P and rv[1] < 2 * P and rv[2] < 2 * P and all(normalised(out, i) for i in range(3))
        # g1_add_lazy2: b within what g1_add_lazy leaves (X < 8p, Y < 4p, Z < 2p)
        jb = jac_of(b, zb, (7, 3, 1) if top else (rng.randrange(8), rng.randrange(4), rng.randrange(2)))
        lcp.lcp_add_lazy(out, to_limbs(ja), to_limbs(jb), 1)
        rv = [from_limbs(out, i) for i in range(3)]
        assert affine_of_jac(rv) == want and rv[0] < 8 * P and rv[1] < 2 * P and rv[2] < 2 * P and all(normalised(out, i) for i in range(3))
        # g1x_add_lazy2: both operands within the accumulator invariant X < 8p, Y < 4p, ZZ, ZZZ < 2p
        def xyzz(pt, z, ks):
            zz, zzz = z * z % P, z * z * z % P
            return [mont(pt[0] * zz % P) + ks[0] * P, mont(pt[1] * zzz % P) + ks[1] * P, mont(zz) + ks[2] * P, mont(zzz) + ks[3] * P]
        ks = (7, 3, 1, 1) if top else (rng.randrange(8), rng.randrange(4), rng.randrange(2), rng.randrange(2))
        lcp.lcp_addx_lazy2(outx, to_limbs(xyzz(a, za, ks)), to_limbs(xyzz(b, zb, ks)))
        X, Y, ZZ, ZZZ = (from_limbs(outx, i) for i in range(4))
        assert X < 8 * P and Y < 2 * P and ZZ < 2 * P and ZZZ < 2 * P and all(normalised(outx, i) for i in range(4))
        x, y, zz, zzz = (unmont(v % P) for v in (X, Y, ZZ, ZZZ))
        assert (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P) == want and zz ** 3 % P == zzz ** 2 % P


def test_lazy_additions_rare_paths(lcp):
    """P + P, P + (-P) and an operand at infinity leave through the canonical complete addition: still the right point."""
    out = (C.c_uint32 * (3 * N))()
    a = ec_mul(7, G)
    neg = (a[0], P - a[1])
    for both in (0, 1):
        for b, want in ((a, ec_add(a, a)), (neg, None)):
            lcp.lcp_add_lazy(out, to_limbs(jac_of(a, 11, (31, 31, 31))), to_limbs(jac_of(b, 13)), both)
            assert affine_of_jac([from_limbs(out, i) for i in range(3)]) == want
        lcp.lcp_add_lazy(out, to_limbs([31 * P + 1, 31 * P + 1, 31 * P]), to_limbs(jac_of(a, 13)), both)      # infinity (lazy zero) + a
        assert affine_of_jac([from_limbs(out, i) for i in range(3)]) == a
        lcp.lcp_add_lazy(out, to_limbs(jac_of(a, 11, (31, 31, 31))), to_limbs([0, 0, 0]), both)                # a + infinity
        assert affine_of_jac([from_limbs(out, i) for i in range(3)]) == a


# ------------------------------------------------------------------------------------------------ subgroup test and decompression
def test_subgroup_predicates_agree_and_are_right(lcp):
    rng = random.Random(0x5156)
    inside = [G, ec_mul(2, G), ec_mul(R_ORDER - 1, G)] + [ec_mul(rng.randrange(1, R_ORDER), G) for _ in range(4)]
    outside = [ORDER3, (0, P - 2), ec_add(G, ORDER3), ec_add(ec_mul(12345, G), (0, P - 2))] + [curve_point(rng) for _ in range(6)]
    for pt in inside:
        assert lcp.lcp_subgroup(to_limbs([mont(pt[0]), mont(pt[1])])) == 3
    for pt in outside:
        assert ec_mul(R_ORDER, pt) is not None                    # (a random curve point is outside the subgroup: the cofactor is ~2^126)
        assert lcp.lcp_subgroup(to_limbs([mont(pt[0]), mont(pt[1])])) == 0
    assert lcp.lcp_subgroup(to_limbs([0, 0])) == 3                # infinity


def _py_decompress(b):
    """(rc, point) by the rules of g1_parse_compressed / g1_decompress: 1 bad encoding, 2 not on the curve."""
    if not b[0] & 0x80:
        return 1, None
    if b[0] & 0x40:
        return (0, None) if b[0] == 0xC0 and not any(b[1:]) else (1, None)
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    if x >= P:
        return 1, None
    y2 = (x ** 3 + 4) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return 2, None
    if (y > (P - 1) // 2) != bool(b[0] & 0x20):
        y = P - y
    return 0, (x, y)


def _compress(pt, large=None):
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if (pt[1] > (P - 1) // 2 if large is None else large) else 0)
    return bytes(b)


def test_decompression_of_the_golden_points(lcp, golden_vectors):
    enc = set()
    for fn in ("verify_kzg_proof", "verify_blob_kzg_proof", "verify_blob_kzg_proof_batch", "compute_blob_kzg_proof"):
        for case in golden_vectors[fn]:
            for key, v in case["input"].items():
                for h in (v if isinstance(v, list) else [v]):
                    if isinstance(h, str) and len(h) == 98:
                        enc.add(bytes.fromhex(h[2:]))
    fx = json.load(open(os.path.join(HERE, "golden", "batch64.json")))
    enc |= {bytes.fromhex(h) for h in fx["commitments"][:8] + fx["proofs"][:8]}
    # both signs of y, x >= p, x = p - 1 + 1, off the curve, flag errors
    enc |= {_compress(G, False), _compress(G, True), _compress((P, 0), False), _compress((P + 5, 0), True), bytes([0x80]) + bytes(47),
            bytes(48), bytes([0xC0]) + bytes(46) + b"\x01", bytes([0xE0]) + bytes(47)}
    off = next(x for x in range(1, 100) if _py_decompress(_compress((x, 0), False))[0] == 2)
    enc |= {_compress((off, 0), False), _compress((off, 0), True)}
    rcs = set()
    xy = (C.c_uint32 * (2 * N))()
    for b in sorted(enc):
        want_rc, want = _py_decompress(b)
        buf = (C.c_uint8 * 48)(*b)
        rc = lcp.lcp_decompress(xy, buf)
        assert rc == want_rc, b.hex()
        rcs.add(rc)
        if rc == 0:
            got = (unmont(from_limbs(xy, 0)), unmont(from_limbs(xy, 1)))
            assert (got == (0, 0) and want is None) or got == want, b.hex()
            assert from_limbs(xy, 0) < P and from_limbs(xy, 1) < P
    assert rcs == {0, 1, 2} and len(enc) > 30


def test_sqrt_on_squares_and_non_squares(lcp):
    rng = random.Random(0x5157)
    out = Limbs()
    vals = [0, 1, 4, P - 1, P - 4] + [rng.randrange(P) for _ in range(40)]
    seen = set()
    for a in vals:
        ok = lcp.lcp_sqrt(out, to_limbs(mont(a)))
        is_sq = a == 0 or pow(a, (P - 1) // 2, P) == 1
        assert bool(ok) == is_sq
        seen.add(is_sq)
        if ok:
            r = unmont(from_limbs(out))
            assert from_limbs(out) < P and r * r % P == a and r == pow(a, (P + 1) // 4, P)
    assert seen == {True, False}
