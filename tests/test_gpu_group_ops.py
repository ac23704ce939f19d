"""The layers above the field arithmetic -- g1.h, tower.h, pairing.h, pairing_coop.h, pairing_lanes.h -- run ON THE DEVICE routine by routine
(tests/native/gpu_group_probe.hip, built by __graft_entry__.build()) against Python big integers (oracle/pyref.py); every comparison is exact.
tests/test_device_math_host.py checks the x86 build of the same headers; on gfx950 the cooperative lanes are real lanes with wave fences over LDS, the
carry of the combination is a DPP row shift, the twelve-lane form runs five checks per wave and the windowed multiplication shares one table per wave.
The tests that need the card are marked gpu one by one; the test of the basis conversion at the end runs anywhere."""
import ctypes as C
import os
import random
import re

import pytest

from oracle import pyref as pr
from oracle.pyref import P, R

from g1_cases import G1_GEN_BYTES, small_order_and_random_curve_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_rust_amd", "csrc")
INF = bytes([0xC0]) + bytes(47)
LANE_COUNTS = (1, 63, 64, 65, 200)                   # a lone lane, partial waves either side of a full one, a second workgroup
X2 = pr.X_ABS ** 2

# operation numbers of gpu_group_probe.hip
(G1_VALIDATE, G1_ADD, G1_ADD_MIXED, G1_DBL, G1X_ADD_MIXED, G1X_ADD_MIXED_LAZY, G1X_ADD_LAZY2, G1_DBL_LAZY, G1_ADD_LAZY, G1_ADD_LAZY2, G1_MUL_WORDS,
 G1_GLV_SPLITS, G1_GLV_MUL, G1_MUL128_W4, G1_PAIRPT) = range(15)
CO_MUL, CO_SQR, CO_LINE_W, CO_LINE_BS, CO_CYC_SQR, CO_CONJ, CO_FROB, CO_FROB2, CO_FP6INV, CO_IS_ONE = range(10)
L12_CYC_SQR, L12_MULF, L12_CONJ, L12_FROB, L12_FROB2, L12_IS_ONE = range(6)
(TW_FP2_MUL, TW_FP2_SQR, TW_FP2_INV, TW_FP2_SQRT, TW_FP2_LEX, TW_FP6_MUL, TW_FP6_INV, TW_FP12_MUL, TW_FP12_SQR, TW_FP12_INV, TW_FP12_FROB,
 TW_FP12_MUL_BY_014, TW_G2_DECOMPRESS) = range(13)
FULL_MASK, EVEN_MASK = 0xfff, 0x555
LINE_COEFFS = (0, 2, 3, 6, 8, 9)
LINE_MASK = sum(1 << j for j in LINE_COEFFS)


@pytest.fixture(scope="module")
def probe():
    so = os.path.join(ROOT, "tests", "native", "libgpu_group_probe.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    return C.CDLL(so)


# ------------------------------------------------------------------------------------------------ the w basis (pairing_coop.h's head)
# Fp12 = Fp[w] / (w^12 - 2 w^6 + 2) with w^2 = v, w^6 = 1 + u: the tower coefficient (x0 + x1 u) v^j w^i sits at m = 2 j + i as a_m += x0 - x1,
# a_{m+6} += x1.  pyref's element is f[i][j] = (x0, x1).
def to_w(f):
    a = [0] * 12
    for i in range(2):
        for j in range(3):
            x0, x1 = f[i][j]
            a[2 * j + i] = (x0 - x1) % P
            a[2 * j + i + 6] = x1 % P
    return a


def from_w(a):
    return tuple(tuple(((a[2 * j + i] + a[2 * j + i + 6]) % P, a[2 * j + i + 6] % P) for j in range(3)) for i in range(2))


def w_schoolbook_mul(a, b):
    d = [0] * 23
    for i in range(12):
        for j in range(12):
            d[i + j] += a[i] * b[j]
    for s in range(22, 11, -1):                      # w^s = 2 w^(s-6) - 2 w^(s-12)
        d[s - 6] += 2 * d[s]
        d[s - 12] -= 2 * d[s]
        d[s] = 0
    return [x % P for x in d[:12]]


def test_w_basis_conversion_matches_the_tower():
    rnd = random.Random(1201)
    for _ in range(8):
        a, b = [rnd.randrange(P) for _ in range(12)], [rnd.randrange(P) for _ in range(12)]
        assert to_w(from_w(a)) == a
        f = tuple(tuple((rnd.randrange(P), rnd.randrange(P)) for _ in range(3)) for _ in range(2))
        assert from_w(to_w(f)) == f
        assert w_schoolbook_mul(a, b) == to_w(pr.f12_mul(from_w(a), from_w(b)))
    assert to_w(pr.F12_ONE) == [1] + [0] * 11
    u = ((pr.F2_ZERO, pr.F2_ZERO, pr.F2_ZERO), (pr.F2_ZERO, pr.F2_ZERO, pr.F2_ZERO))
    w1 = [0, 1] + [0] * 10                           # w itself: w^2 = v, w^6 = v^3 = xi = 1 + u
    w2 = w_schoolbook_mul(w1, w1)
    assert from_w(w2) == ((pr.F2_ZERO, pr.F2_ONE, pr.F2_ZERO), u[1])
    w6 = w_schoolbook_mul(w_schoolbook_mul(w2, w2), w2)
    assert from_w(w6) == (((1, 1), pr.F2_ZERO, pr.F2_ZERO), u[1])


# ------------------------------------------------------------------------------------------------ G1
def _launched(st):
    """The probe's return value: a HIP error ends the whole session -- nothing more is started on a card that may have faulted."""
    if st < 0 and st != -4:
        pytest.exit(f"gpu_group_probe: HIP status {st}", returncode=3)
    assert st == 0, st


def _lanes(cases):
    """The case list dealt to 1, 63, 64, 65 and 200 lanes at successive offsets (cyclically): every case of a list of up to 393 is run."""
    assert len(cases) <= sum(LANE_COUNTS)
    off = 0
    for n in LANE_COUNTS:
        yield [cases[(off + i) % len(cases)] for i in range(n)]
        off += n


def _g1(probe, op, a, b, k, pre=0):
    n = len(a)
    out = C.create_string_buffer(64 * n); rc = (C.c_int * n)()
    _launched(probe.gpu_g1_ops(op, n, b"".join(a), b"".join(b), b"".join(x.to_bytes(32, "big") for x in k), pre, out, rc))
    return [out.raw[64 * i:64 * i + 64] for i in range(n)], list(rc)


_MUL_CACHE = {}


def _mul(pt, k):                                     # pyref's double-and-add is the slow part of this module: every product is computed once
    if (pt, k) not in _MUL_CACHE:
        _MUL_CACHE[(pt, k)] = pr.g1_mul(pt, k)
    return _MUL_CACHE[(pt, k)]


@pytest.fixture(scope="module")
def g1_points(setup_bytes):
    """(G1 points, curve points outside G1), as pyref points."""
    g1 = setup_bytes[0]
    inside = [pr.g1_uncompress(G1_GEN_BYTES)] + [pr.g1_uncompress(g1[48 * i:48 * i + 48]) for i in (0, 1, 77, 4095)]
    outside = [(0, 2)]                               # the curve point with x = 0 (order 3)
    return inside, outside


@pytest.fixture(scope="module")
def odd_points():
    return [pt for _, pt in small_order_and_random_curve_points(seed=381, trials=12)]


@pytest.mark.gpu
def test_g1_decoding_and_subgroup_checks_on_device(probe, g1_points, odd_points):
    inside, outside = g1_points
    enc = [INF] + [pr.g1_compress(p) for p in inside + outside + odd_points]
    rnd = random.Random(14)
    for _ in range(40):                              # random x, as test_g1_validate_matches_oracle: on the curve or not, almost surely outside G1
        b = bytearray(rnd.randrange(P).to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if rnd.random() < 0.5 else 0)
        enc.append(bytes(b))
    enc += [bytes(48), bytes([0x80]) + bytes(47), bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01", bytes([0x9A]) + b"\xff" * 47]
    want = {}
    for e in set(enc):
        try:
            pt = pr.g1_uncompress(e)
        except pr.KzgError as err:
            want[e] = (2 if "not on curve" in str(err) else 1,) * 2
            continue
        want[e] = (0, 0 if pt is None or pr.g1_mul(pt, R) is None else 3)
    assert sorted(set(w for w, _ in want.values())) == [0, 1, 2] and sum(w == (0, 3) for w in want.values()) >= 20
    for check in (0, 1):
        for lanes in _lanes(enc):
            out, rc = _g1(probe, G1_VALIDATE, lanes, lanes, [0] * len(lanes), check)
            assert rc == [want[e][check] for e in lanes]
            assert all(o[:48] == e for o, e, c in zip(out, lanes, rc) if c == 0)      # recompressed through g1_compress_affine


# header comments of g1.h: the bounds the lazy routines promise; `pre` lazy steps in front bring an operand from canonical to those magnitudes
PRE_STEPS = (0, 1, 3)


@pytest.mark.gpu
def test_g1_additions_and_doublings_on_device(probe, g1_points, odd_points):
    inside, outside = g1_points
    singles = [None] + inside + outside + odd_points[:1] + [pt for pt in odd_points if pr.g1_mul(pt, 3) is None][:1] \
        + [pt for pt in odd_points if pr.g1_mul(pt, 11) is None][:1]
    pairs = [(None, None)]
    for p in singles[1:]:
        pairs += [(None, p), (p, None), (p, p), (p, pr.g1_neg(p))]
    rnd = random.Random(2201)
    pairs += [(rnd.choice(singles[1:]), rnd.choice(singles[1:])) for _ in range(24)]
    pairs += [(_mul(p, 2), p) for p in inside[:3]] + [(p, _mul(p, 2)) for p in inside[:3]]      # 2P and P: a chain of equal operands one step on
    add = pr.g1_add
    ops = [(G1_ADD, 0, lambda a, b: add(a, b)), (G1_ADD_MIXED, 0, lambda a, b: add(a, b)), (G1_DBL, 0, lambda a, b: add(a, a)),
           (G1X_ADD_MIXED, 0, lambda a, b: add(a, b))]
    for pre in PRE_STEPS:
        ops += [(G1X_ADD_MIXED_LAZY, pre, lambda a, b, s=pre: add(a, _mul(b, s + 1))),
                (G1X_ADD_LAZY2, pre, lambda a, b, s=pre: _mul(add(a, b), s + 1)),
                (G1_DBL_LAZY, pre, lambda a, b, s=pre: _mul(a, 2 << s)),
                (G1_ADD_LAZY, pre, lambda a, b, s=pre: add(_mul(a, 1 << s), b)),
                (G1_ADD_LAZY2, pre, lambda a, b, s=pre: add(_mul(a, 1 << s), _mul(b, (1 << s) + 1 if s else 1)))]
    for op, pre, ref in ops:
        for lanes in _lanes(pairs):
            out, rc = _g1(probe, op, [pr.g1_compress(a) for a, _ in lanes], [pr.g1_compress(b) for _, b in lanes], [0] * len(lanes), pre)
            assert rc == [0] * len(lanes), (op, pre)
            got = [o[:48] for o in out]
            want = [pr.g1_compress(ref(a, b)) for a, b in lanes]
            assert got == want, (op, pre, [i for i in range(len(lanes)) if got[i] != want[i]][:8])


W4_SCALARS = [0, 1, 7, 8, 9, 15, 16, 1 << 127, (1 << 128) - 1, int("8" * 32, 16), int("7" * 32, 16)]
GLV_EDGE = [0, 1, X2 - 1, X2, X2 + 1, 2 * X2 - 1, 2 * X2, R - 1, R - 2, (X2 - 1) * X2, (X2 - 1) * X2 - 1, (X2 - 2) * X2 + X2 - 1,
            (1 << 255) - 1, (1 << 254), (1 << 127), (1 << 127) - 1, (1 << 128) - 1, (1 << 128), 3 * X2 - 1, 3 * X2]
GLV_EDGE += [m * X2 + d for m in (1, 2, 12345, X2 // 2, X2 - 2) for d in (-1, 0, 1)]


@pytest.mark.gpu
def test_g1_scalar_multiplications_on_device(probe, g1_points):
    inside, outside = g1_points
    rnd = random.Random(2202)
    zeros = lambda n: [INF] * n
    # both GLV splits of every scalar: k = a + b x^2, 0 <= a < x^2
    scal = GLV_EDGE + [rnd.randrange(R) for _ in range(2000)]
    for lanes in list(_lanes(GLV_EDGE)) + [scal]:
        out, rc = _g1(probe, G1_GLV_SPLITS, zeros(len(lanes)), zeros(len(lanes)), lanes)
        assert rc == [0] * len(lanes)
        for k, o in zip(lanes, out):
            assert [int.from_bytes(o[16 * i:16 * i + 16], "little") for i in range(4)] == [k % X2, k // X2] * 2, hex(k)
    pts = [None] + inside
    # double-and-add over 256 bits: any scalar, any curve point
    cases = [(p, k) for p in pts + outside for k in [0, 1, 2, R - 1, R, R + 5, (1 << 256) - 1] + [rnd.randrange(1 << 256) for _ in range(2)]]
    for lanes in _lanes(cases):
        out, rc = _g1(probe, G1_MUL_WORDS, [pr.g1_compress(p) for p, _ in lanes], zeros(len(lanes)), [k for _, k in lanes])
        assert rc == [0] * len(lanes)
        assert [o[:48] for o in out] == [pr.g1_compress(_mul(p, k)) for p, k in lanes]
    # the GLV form of k_lincomb: scalars below r, points of G1 (phi = [-x^2] only there)
    cases = [(p, k) for p in pts for k in [0, 1, 2, R - 1, (1 << 128) - 1, 1 << 128, X2, X2 - 1] + [rnd.randrange(R) for _ in range(2)]]
    for lanes in _lanes(cases):
        out, rc = _g1(probe, G1_GLV_MUL, [pr.g1_compress(p) for p, _ in lanes], zeros(len(lanes)), [k for _, k in lanes])
        assert rc == [0] * len(lanes)
        assert [o[:48] for o in out] == [pr.g1_compress(_mul(p, k)) for p, k in lanes]
    # signed 4-bit windows over 128 bits, one table per wave: a different point and scalar in every lane, neighbouring lanes on different digits
    scal = []
    for i in range(64):
        scal.append(W4_SCALARS[i % len(W4_SCALARS)] if i % 2 == 0 else rnd.randrange(1 << 128))
    cases = [((pts + outside)[(3 * i + i // 7) % 7], scal[i]) for i in range(64)]
    assert all(cases[i] != cases[i + 1] for i in range(63)) and set(W4_SCALARS) <= set(scal)
    for lanes in [cases] + list(_lanes(cases)):      # all 64 lanes of one wave first, then the usual counts
        out, rc = _g1(probe, G1_MUL128_W4, [pr.g1_compress(p) for p, _ in lanes], zeros(len(lanes)), [k for _, k in lanes])
        assert rc == [0] * len(lanes)
        got, want = [o[:48] for o in out], [pr.g1_compress(_mul(p, k)) for p, k in lanes]
        assert got == want, [i for i in range(len(lanes)) if got[i] != want[i]][:8]


@pytest.mark.gpu
def test_pairing_point_form_round_trip_on_device(probe, g1_points, odd_points):
    inside, outside = g1_points
    pts = [None] + inside + outside + odd_points[:8]
    for negate in (0, 1):
        for lanes in _lanes(pts):
            out, rc = _g1(probe, G1_PAIRPT, [pr.g1_compress(p) for p in lanes], [INF] * len(lanes), [0] * len(lanes), negate)
            assert rc == [0] * len(lanes)
            assert [o[:48] for o in out] == [pr.g1_compress(pr.g1_neg(p) if negate else p) for p in lanes]


# ------------------------------------------------------------------------------------------------ Fp12 in the w basis
def _header_bound(name, pattern):
    text = open(os.path.join(CSRC, name)).read()
    found = re.findall(pattern, text)
    assert len(found) == 1, (name, pattern, found)
    return int(found[0])


# The multiple of p the tests add to every (canonical, <= p - 1) coefficient so that it sits at the edge of the invariant its header states:
#   pairing_coop.h  "every coefficient stays below 32 p": (p - 1) + 31 p < 32 p
#   pairing_lanes.h "0 <= value <= 2p":                   (p - 1) + p <= 2 p
COOP_OFFSET, L12_OFFSET = 31, 1


def test_lazy_offsets_sit_at_the_bounds_the_headers_state():
    coop_bound = _header_bound("pairing_coop.h", r"every coefficient stays below (\d+) p: the lazy bound of an")
    l12_bound = _header_bound("pairing_lanes.h", r"operations: 0 <= value <= (\d+)p, limbs normalised")
    assert (P - 1) + COOP_OFFSET * P < coop_bound * P <= (P - 1) + (COOP_OFFSET + 1) * P
    assert (P - 1) + L12_OFFSET * P <= l12_bound * P < (P - 1) + (L12_OFFSET + 1) * P
    assert _header_bound("pairing_coop.h", r"odd k: (\d+)p - a_k \(coefficients are lazy, < \d+p\)") == coop_bound      # coop_conj subtracts from the same bound


def _f12(fn, n, a, ka, b, kb, *extra):
    pack = lambda els: b"".join(c.to_bytes(48, "big") for e in els for c in e)
    out = C.create_string_buffer(576 * n); rc = (C.c_int * n)()
    _launched(fn(n, pack(a), bytes(ka) * (12 * n), pack(b), bytes(kb) * (12 * n), *extra, out, rc))
    return [[int.from_bytes(out.raw[576 * i + 48 * k:576 * i + 48 * k + 48], "big") for k in range(12)] for i in range(n)], list(rc)


def _coop(probe, op, a, b, offset):
    return _f12(lambda *args: probe.gpu_coop_ops(op, *args), len(a), a, [offset], b, [offset])


def _l12(probe, op, a, b, offset, jmask=FULL_MASK):
    return _f12(lambda *args: probe.gpu_l12_ops(op, *args), len(a), a, [offset], b, [offset], C.c_uint32(jmask))


def _frob(f, power):
    for _ in range(power):
        f = pr.f12_frob(f)
    return f


@pytest.fixture(scope="module")
def f12_inputs():
    """(general elements, elements of the cyclotomic subgroup), w basis."""
    rnd = random.Random(2203)
    general = [[0] * 12, [1] + [0] * 11]
    general += [[rnd.randrange(1, P) if j == k else 0 for j in range(12)] for k in range(12)]
    general += [[P - 1] * 12]
    general += [[rnd.randrange(P) for _ in range(12)] for _ in range(64)]
    cyc = [[1] + [0] * 11]
    for a in general[-32:]:                          # f^((p^6 - 1)(p^2 + 1)): conj(f) / f, then its p^2-power Frobenius times itself
        f = from_w(a)
        g = pr.f12_mul(pr.f12_conj(f), pr.f12_inv(f))
        cyc.append(to_w(pr.f12_mul(_frob(g, 2), g)))
    return general, cyc


def _masked(a, mask):
    return [c if (mask >> k) & 1 else 0 for k, c in enumerate(a)]


@pytest.mark.gpu
def test_cooperative_fp12_operations_on_device(probe, f12_inputs):
    general, cyc = f12_inputs
    other = [general[(7 * i + 3) % len(general)] for i in range(len(general))]
    mul = lambda a, b: to_w(pr.f12_mul(from_w(a), from_w(b)))
    def fp6_inv(a):
        f = from_w(a)[0]
        return [0] * 12 if f == pr.F6_ZERO else to_w((pr.f6_inv(f), pr.F6_ZERO))
    ones = general[:14] + [[1] + [0] * 10 + [1], [1, P - 1] + [0] * 10, [2] + [0] * 11]
    for offset in (0, COOP_OFFSET):
        for op, a, b, ref in ((CO_MUL, general, other, mul), (CO_SQR, general, general, lambda a, b: mul(a, a)),
                              (CO_LINE_W, general, [_masked(x, LINE_MASK) for x in other], mul),
                              (CO_LINE_BS, general, [_masked(x, LINE_MASK) for x in other], mul),
                              (CO_CYC_SQR, cyc, cyc, lambda a, b: mul(a, a)),
                              (CO_CONJ, general, general, lambda a, b: to_w(pr.f12_conj(from_w(a)))),
                              (CO_FROB, general, general, lambda a, b: to_w(_frob(from_w(a), 1))),
                              (CO_FROB2, general, general, lambda a, b: to_w(_frob(from_w(a), 2))),
                              (CO_FP6INV, [_masked(x, EVEN_MASK) for x in general], general, lambda a, b: fp6_inv(a))):
            got, rc = _coop(probe, op, a, b, offset)
            assert rc == [0] * len(a), (op, offset)
            want = [ref(x, y) for x, y in zip(a, b)]
            assert got == want, (op, offset, [i for i in range(len(a)) if got[i] != want[i]][:8])
        got, rc = _coop(probe, CO_IS_ONE, ones, ones, offset)
        assert rc == [101 if x == [1] + [0] * 11 else 100 for x in ones] and got == ones, offset


@pytest.mark.gpu
def test_twelve_lane_fp12_operations_on_device(probe, f12_inputs):
    general, cyc = f12_inputs
    other = [general[(7 * i + 3) % len(general)] for i in range(len(general))]
    mul = lambda a, b: to_w(pr.f12_mul(from_w(a), from_w(b)))
    ones = general[:14] + [[1] + [0] * 10 + [1], [1, P - 1] + [0] * 10, [2] + [0] * 11]
    assert len(general) % 5 and len(cyc) % 5         # a wave with idle groups at the end of both lists
    for offset in (0, L12_OFFSET):
        for op, a, b, mask, ref in ((L12_CYC_SQR, cyc, cyc, FULL_MASK, lambda a, b: mul(a, a)),
                                    (L12_MULF, general, other, FULL_MASK, mul),
                                    (L12_MULF, general, other, EVEN_MASK, lambda a, b: mul(a, _masked(b, EVEN_MASK))),
                                    (L12_MULF, general, other, LINE_MASK, lambda a, b: mul(a, _masked(b, LINE_MASK))),
                                    (L12_CONJ, general, general, FULL_MASK, lambda a, b: to_w(pr.f12_conj(from_w(a)))),
                                    (L12_FROB, general, general, FULL_MASK, lambda a, b: to_w(_frob(from_w(a), 1))),
                                    (L12_FROB2, general, general, FULL_MASK, lambda a, b: to_w(_frob(from_w(a), 2)))):
            got, rc = _l12(probe, op, a, b, offset, mask)
            assert rc == [0] * len(a), (op, offset)
            want = [ref(x, y) for x, y in zip(a, b)]
            assert got == want, (op, mask, offset, [i for i in range(len(a)) if got[i] != want[i]][:8])
        got, rc = _l12(probe, L12_IS_ONE, ones, ones, offset)
        assert rc == [101 if x == [1] + [0] * 11 else 100 for x in ones] and got == ones, offset


# ------------------------------------------------------------------------------------------------ the whole pairing check
def _g2_compress(pt):                                # 96 bytes, x.c1 with the flags then x.c0 (the inverse of pyref.g2_uncompress)
    (x0, x1), (y0, y1) = pt
    big = y1 > (P - 1) // 2 if y1 else y0 > (P - 1) // 2
    out = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if big else 0)
    return bytes(out)


@pytest.mark.gpu
def test_pairing_checks_on_device(probe, setup_bytes):
    g1, g2 = setup_bytes
    q0, q1 = g2[:96], g2[96:192]
    a = random.Random(16).randrange(R)
    gen = pr.g1_uncompress(G1_GEN_BYTES)
    aG, a1G = pr.g1_compress(_mul(gen, a)), pr.g1_compress(_mul(gen, (a + 1) % R))
    cases = [(aG, q0, aG, q0), (aG, q0, G1_GEN_BYTES, q0), (aG, q1, G1_GEN_BYTES, q0), (INF, q0, INF, q1), (INF, q0, G1_GEN_BYTES, q1),
             (g1[:48], q1, g1[48:96], q0), (g1[48:96], q0, g1[:48], q1),            # the seven of test_g2_decompress_and_pairing ...
             (aG, q1, a1G, q1), (aG, q1, aG, q1)]                                   # ... and [a]G against [a + 1]G and against itself
    # In every true case above the two Miller loops walk the SAME G2 point with opposite G1 points: their product lies in Fp6 and the easy part of
    # the final exponentiation alone sends it to 1.  e([a]G, [5]G2) == e([5a]G, G2) is true only through the hard part; [5a + 1]G makes it false.
    q5 = _g2_compress(pr.g2_mul(pr.G2_GEN, 5))
    assert q0 == _g2_compress(pr.G2_GEN)
    cases += [(aG, q5, pr.g1_compress(_mul(gen, 5 * a % R)), q0), (aG, q5, pr.g1_compress(_mul(gen, (5 * a + 1) % R)), q0)]
    want = [pr.pairings_verify(pr.g1_uncompress(p1), pr.g2_uncompress(qa), pr.g1_uncompress(p2), pr.g2_uncompress(qb)) for p1, qa, p2, qb in cases]
    assert want[-2:] == [True, False] and want.count(True) >= 4
    n = len(cases)
    ok_coop, ok_l12, rc = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    _launched(probe.gpu_pairing_checks(n, *(b"".join(c[i] for c in cases) for i in range(4)), ok_coop, ok_l12, rc))
    assert list(rc) == [0] * n                       # every coefficient of the twelve-lane result equals the cooperative run's
    assert [bool(v) for v in ok_coop] == want
    assert [bool(v) for v in ok_l12] == want


# ------------------------------------------------------------------------------------------------ lane routines of tower.h / pairing.h
def _flat(f):                                        # an Fp2, Fp6 or Fp12 element of pyref -> its base-field coefficients in tower order
    return [f] if isinstance(f, int) else [c for x in f for c in _flat(x)]


def _tower(probe, op, a, b=None):
    n = len(a)
    pack = lambda els: b"".join(b"".join(c.to_bytes(48, "big") for c in _flat(e)).ljust(576, b"\0") for e in els)
    out = C.create_string_buffer(576 * n); rc = (C.c_int * n)()
    _launched(probe.gpu_tower_ops(op, n, pack(a), pack(b if b is not None else a), out, rc))
    return [[int.from_bytes(out.raw[576 * i + 48 * k:576 * i + 48 * k + 48], "big") for k in range(12)] for i in range(n)], list(rc)


def _padded(f):
    c = _flat(f)
    return c + [0] * (12 - len(c))


@pytest.mark.gpu
def test_tower_lane_routines_on_device(probe, setup_bytes):
    rnd = random.Random(2204)
    f2 = lambda: (rnd.randrange(P), rnd.randrange(P))
    f6 = lambda: (f2(), f2(), f2())
    f12 = lambda: (f6(), f6())
    e2 = [pr.F2_ZERO, pr.F2_ONE, (0, 1), (P - 1, P - 1), (P - 1, 0), (0, P - 1), (1, 1)]
    a2 = e2 + [f2() for _ in range(200 - len(e2))]
    b2 = [a2[(7 * i + 3) % len(a2)] for i in range(len(a2))]
    zero6, zero12 = pr.F6_ZERO, (pr.F6_ZERO, pr.F6_ZERO)
    unit6 = [tuple((1, 0) if j == k else (0, 0) for j in range(3)) for k in range(3)]
    a6 = [zero6, pr.F6_ONE, ((P - 1, P - 1),) * 3] + unit6 + [f6() for _ in range(65 - 6)]
    b6 = [a6[(7 * i + 3) % len(a6)] for i in range(len(a6))]
    a12 = [zero12, pr.F12_ONE, (((P - 1, P - 1),) * 3,) * 2] + [(u, zero6) for u in unit6] + [(zero6, u) for u in unit6] + [f12() for _ in range(65 - 9)]
    b12 = [a12[(7 * i + 3) % len(a12)] for i in range(len(a12))]
    lines = [(f2(), f2(), f2()) for _ in a12]
    lines[1], lines[2] = (pr.F2_ZERO,) * 3, (pr.F2_ONE, pr.F2_ZERO, pr.F2_ZERO)
    inv2 = lambda x: pr.F2_ZERO if x == pr.F2_ZERO else pr.f2_inv(x)
    inv6 = lambda x: zero6 if x == zero6 else pr.f6_inv(x)
    inv12 = lambda x: zero12 if x == zero12 else pr.f12_inv(x)
    for op, a, b, ref in ((TW_FP2_MUL, a2, b2, pr.f2_mul), (TW_FP2_SQR, a2, a2, lambda x, y: pr.f2_sqr(x)), (TW_FP2_INV, a2, a2, lambda x, y: inv2(x)),
                          (TW_FP6_MUL, a6, b6, pr.f6_mul), (TW_FP6_INV, a6, a6, lambda x, y: inv6(x)),
                          (TW_FP12_MUL, a12, b12, pr.f12_mul), (TW_FP12_SQR, a12, a12, lambda x, y: pr.f12_sqr(x)),
                          (TW_FP12_INV, a12, a12, lambda x, y: inv12(x)), (TW_FP12_FROB, a12, a12, lambda x, y: pr.f12_frob(x)),
                          (TW_FP12_MUL_BY_014, a12, lines, lambda x, l: pr.f12_mul(x, ((l[0], l[1], pr.F2_ZERO), (pr.F2_ZERO, l[2], pr.F2_ZERO))))):
        got, rc = _tower(probe, op, a, b)
        assert rc == [0] * len(a), op
        want = [_padded(ref(x, y)) for x, y in zip(a, b)]
        assert got == want, (op, [i for i in range(len(a)) if got[i] != want[i]][:8])
    _, rc = _tower(probe, TW_FP2_LEX, a2)            # the sign rule of the compressed G2 encoding: c1 decides unless it is zero
    half = (P - 1) // 2
    assert rc == [101 if (x[1] > half if x[1] else x[0] > half) else 100 for x in a2]
    # square roots: zero, the two units, 64 squares, 64 arbitrary values (about half of them are squares)
    sq = [pr.F2_ZERO, pr.F2_ONE, (0, 1)] + [pr.f2_sqr(x) for x in a2[-64:]] + a2[-128:-64]
    got, rc = _tower(probe, TW_FP2_SQRT, sq)
    n_none = 0
    for x, s, c in zip(sq, got, rc):
        want = pr.f2_sqrt(x)
        assert c == (2 if want is None else 0), x
        if want is None:
            n_none += 1
        else:
            assert s[2:] == [0] * 10
            s = (s[0], s[1])
            assert pr.f2_sqr(s) == x and s in (want, pr.f2_neg(want))
    assert 16 <= n_none <= 48
    # g2_decompress: the 65 setup points and the two bad encodings of test_g2_decompress_and_pairing
    g2 = setup_bytes[1]
    bad = bytearray(g2[:96]); bad[95] ^= 1
    enc = [g2[96 * i:96 * i + 96] for i in range(65)] + [bytes(bad), bytes(96)]
    n = len(enc)
    out = C.create_string_buffer(576 * n); rc = (C.c_int * n)()
    _launched(probe.gpu_tower_ops(TW_G2_DECOMPRESS, n, b"".join(e.ljust(576, b"\0") for e in enc), bytes(576 * n), out, rc))
    for i, e in enumerate(enc):
        try:
            pt = pr.g2_uncompress(e)
        except pr.KzgError as err:
            assert rc[i] == (2 if "not on curve" in str(err) else 1), i
            continue
        assert rc[i] == 0, i
        got = [int.from_bytes(out.raw[576 * i + 48 * k:576 * i + 48 * k + 48], "big") for k in range(4)]
        assert got == [pt[0][0], pt[0][1], pt[1][0], pt[1][1]], i
    assert rc[65] != 0 or pr.g2_uncompress(bytes(bad)) is not None
    assert rc[66] == 1
