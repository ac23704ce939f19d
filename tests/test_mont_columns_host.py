"""The column (product-scanning) forms of the lazy Montgomery products of kzg_rust_amd/csrc/field.h -- mont_mul_lazy_cols, mont_mul2_lazy_cols,
mont_sqr_cols, mont_mulsqr2_lazy_cols, the four wrappers of the one column body mont_cols -- compiled for the HOST
(tests/native/mont_columns_probe.cpp) and checked, for N = 9 (Fr) and N = 14 (Fp), against their row forms (mont_mul_lazy, mont_mul2_lazy: the
body mont_mul<N, TWO, LAZY>; mont_sqr, mont_mulsqr2_lazy: the body mont_sqr<N, LAZY, AB, SH>) limb for limb and against Python big integers.  The probe takes RAW limbs,
so the operands sit at the bounds the callers really pass: lazy values of up to 32p with the excess in the top limb, all-ones limbs, the
carry-free operands of the evaluation tree (limbs up to 2^30, 3 * 2^29 and 2^31), the doubling's operand bounds, zeros and multiples of the
modulus.  Runs without a GPU."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(HERE, "..", "kzg_rust_amd", "csrc")
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
LB = 29
LMASK = (1 << LB) - 1
MODULUS = {9: R_ORDER, 14: P}
ROW, COLS, COLS_PIN = 0, 1, 2


@pytest.fixture(scope="module")
def mcp():
    src = os.path.join(NATIVE, "mont_columns_probe.cpp")
    so = os.path.join(NATIVE, "libmont_columns_probe.so")
    deps = [src] + [os.path.join(CSRC, f) for f in ("field.h", "modinv.h", "consts_gen.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    return C.CDLL(so)


# ------------------------------------------------------------------------------------------------ limbs
def norm(v, n):
    """value -> n limbs, normalised: 29 bits each, the top limb keeps the excess"""
    assert 0 <= v and (v >> (LB * (n - 1))) < (1 << 32)
    return [(v >> (LB * i)) & LMASK for i in range(n - 1)] + [v >> (LB * (n - 1))]


def value(limbs):
    return sum(int(x) << (LB * i) for i, x in enumerate(limbs))


def arr(limbs):
    return (C.c_uint32 * len(limbs))(*limbs)


def check_quotient(out, t, n):
    """out is exactly (t + q m) / R for a q in [0, R) -- the Montgomery quotient -- with every limb below the top one normalised"""
    m, R = MODULUS[n], 1 << (LB * n)
    v = value(out)
    num = v * R - t
    assert num >= 0 and num % m == 0 and num // m < R, hex(t)
    assert all(int(x) <= LMASK for x in list(out)[:n - 1])


def run3(fn, n, operands, *extra):
    """the row form, the column form and the pinned column form on the same raw limbs; the three results must be the same limbs"""
    outs = []
    for form in (ROW, COLS, COLS_PIN):
        o = (C.c_uint32 * n)()
        assert fn(o, *[arr(x) for x in operands], n, form, *extra) == 0
        outs.append(list(o))
    assert outs[0] == outs[1] == outs[2], [[hex(x) for x in op] for op in operands]
    return outs[0]


# ------------------------------------------------------------------------------------------------ operands
def lazy_values(n, rng, bound_in_m, count):
    """normalised lazy values below bound_in_m * m: the corners (zero, k m, k m +- small, the bound itself, all-ones lower limbs under the largest top
    limb, the top-limb excess alone) and random ones"""
    m = MODULUS[n]
    low = (1 << (LB * (n - 1))) - 1
    bound = bound_in_m * m
    top = ((bound - low - 1) >> (LB * (n - 1))) << (LB * (n - 1))
    vals = [0, 1, m - 1, m, m + 1, bound - 1, top + low, top, low, (bound_in_m - 1) * m, (bound_in_m - 1) * m + 3, (bound_in_m // 2) * m - 2]
    vals += [rng.randrange(bound) for _ in range(count)]
    return [v for v in vals if 0 <= v < bound]


def all_ones(n):
    return [LMASK] * n


@pytest.mark.parametrize("n", [9, 14])
def test_mul_columns_on_lazy_and_all_ones_operands(mcp, n):
    rng = random.Random(0x6301 + n)
    A = lazy_values(n, rng, 32, 40)
    B = lazy_values(n, rng, 32, 40)
    rng.shuffle(B)
    pairs = list(zip(A, B)) + [(a, b) for a in A[:12] for b in A[:12]]
    for a, b in pairs:
        out = run3(mcp.mcp_mul, n, (norm(a, n), norm(b, n)))
        check_quotient(out, a * b, n)
        if a * b < (1 << 12) * MODULUS[n] ** 2 and n == 14:
            assert value(out) < P + (P >> 13)                     # the stated result bound of the lazy Fp products
    out = run3(mcp.mcp_mul, n, (all_ones(n), all_ones(n)))        # every limb 2^29 - 1: the largest columns normalised operands can make
    check_quotient(out, value(all_ones(n)) ** 2, n)


@pytest.mark.parametrize("n", [9, 14])
def test_mul2_columns_on_lazy_and_all_ones_operands(mcp, n):
    rng = random.Random(0x6302 + n)
    # the fused Y3 of the lazy additions (R < 4p, V - X3 + 8p < 10p, 2p - S1 <= 2p, HHH < 2p) and wider: all four below 32 m
    for bounds in ((4, 10, 3, 2), (32, 32, 32, 32)):
        ops = [lazy_values(n, rng, b, 30) for b in bounds]
        for k in range(max(len(o) for o in ops)):
            a, b, c, d = (o[(k + 5 * i) % len(o)] for i, o in enumerate(ops))
            out = run3(mcp.mcp_mul2, n, (norm(a, n), norm(b, n), norm(c, n), norm(d, n)))
            check_quotient(out, a * b + c * d, n)
            if n == 14 and a * b + c * d < (1 << 12) * P * P:
                assert value(out) < P + (P >> 13)
    ones = all_ones(n)
    out = run3(mcp.mcp_mul2, n, (ones, ones, ones, ones))
    check_quotient(out, 2 * value(ones) ** 2, n)


def test_fr_raw_operands_at_the_evaluation_trees_bounds(mcp):
    """eval_core.h: A = n0 + n1 without carries (limbs < 2^30), B = n0 - n1 + K r limb by limb (limbs < 3 * 2^29) against normalised z^k and s below
    r -- 27 * 2^59 per column -- and the single product with one operand's limbs up to 2^31 against a normalised one (9 * 2^60 + 9 * 2^58)."""
    n, r = 9, R_ORDER
    rng = random.Random(0x6303)
    norm_ops = [r - 1, 0, 1, value(all_ones(n)) % r, rng.randrange(r), rng.randrange(r)]
    raw = lambda top: [[top - 1] * n, [0] * n, [top - 1] * (n - 1) + [0], [1] + [top - 1] * (n - 1)] + [[rng.randrange(top) for _ in range(n)] for _ in range(40)]
    As, Bs = raw(1 << 30), raw(3 << 29)
    for k, (A, B) in enumerate(zip(As, Bs)):
        zk, s = norm_ops[k % len(norm_ops)], norm_ops[(k // 2 + 1) % len(norm_ops)]
        out = run3(mcp.mcp_mul2, n, (A, norm(zk, n), B, norm(s, n)))
        check_quotient(out, value(A) * zk + value(B) * s, n)
        assert value(out) < r + (value(A) * zk + value(B) * s) // (1 << (LB * n)) + 1
    # the largest column the tree can make: every limb of A and B at its bound against all-ones (normalised) limbs
    out = run3(mcp.mcp_mul2, n, (As[0], all_ones(n), Bs[0], all_ones(n)))
    check_quotient(out, (value(As[0]) + value(Bs[0])) * value(all_ones(n)), n)
    for A in raw(1 << 31):
        for b in (r - 1, rng.randrange(r)):
            out = run3(mcp.mcp_mul, n, (A, norm(b, n)))
            check_quotient(out, value(A) * b, n)
    out = run3(mcp.mcp_mul, n, ([(1 << 31) - 1] * n, all_ones(n)))
    check_quotient(out, value([(1 << 31) - 1] * n) * value(all_ones(n)), n)


@pytest.mark.parametrize("n", [9, 14])
def test_sqr_columns_lazy_and_canonical(mcp, n):
    rng = random.Random(0x6304 + n)
    m = MODULUS[n]
    for a in lazy_values(n, rng, 32, 80):
        out = run3(mcp.mcp_sqr, n, (norm(a, n),), 1)
        check_quotient(out, a * a, n)
    out = run3(mcp.mcp_sqr, n, (all_ones(n),), 1)
    check_quotient(out, value(all_ones(n)) ** 2, n)
    R = 1 << (LB * n)
    for a in [0, 1, m - 1, m // 2] + [rng.randrange(m) for _ in range(40)]:          # the canonical form: operand below m, result the residue itself
        out = run3(mcp.mcp_sqr, n, (norm(a, n),), 0)
        assert value(out) == a * a * pow(R, -1, m) % m


@pytest.mark.parametrize("n", [9, 14])
def test_mulsqr2_columns_at_the_doublings_bounds(mcp, n):
    """g1_dbl_lazy: a = E (stated < 6p), b = X3 - D + 4p (16p taken), c = 2B < 4p; the same multiples of the modulus for N = 9"""
    rng = random.Random(0x6305 + n)
    m = MODULUS[n]
    ops = [lazy_values(n, rng, b, 60) for b in (6, 16, 4)]
    for k in range(max(len(o) for o in ops)):
        a, b, c = (o[(k + 7 * i) % len(o)] for i, o in enumerate(ops))
        out = run3(mcp.mcp_mulsqr2, n, (norm(a, n), norm(b, n), norm(c, n)))
        check_quotient(out, a * b + 2 * c * c, n)
        if n == 14:
            assert value(out) < P + (P >> 13)
    for a, b, c in ((6 * m - 1, 16 * m - 1, 4 * m - 1), (0, 0, 0), (m, m, m), (5 * m, 15 * m, 3 * m), (0, 16 * m - 1, 0), (6 * m - 1, 0, 4 * m - 1)):
        out = run3(mcp.mcp_mulsqr2, n, (norm(a, n), norm(b, n), norm(c, n)))
        check_quotient(out, a * b + 2 * c * c, n)
    ones = all_ones(n)                                             # the asserted column budget of the form: 58 * 2^58 + carry at N = 14
    out = run3(mcp.mcp_mulsqr2, n, (ones, ones, ones))
    check_quotient(out, 3 * value(ones) ** 2, n)


def test_both_forms_under_the_undefined_behaviour_sanitizer():
    """The probe as a stand-alone program under -fsanitize=undefined: shifts, signed overflow and array bounds of both forms on a fixed operand set."""
    src = os.path.join(NATIVE, "mont_columns_probe.cpp")
    exe = os.path.join(NATIVE, "mont_columns_ubsan")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-DMONT_COLUMNS_MAIN", "-o", exe, src], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and "0 mismatches" in done.stdout, done.stdout + done.stderr
