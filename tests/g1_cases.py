"""Points ON the curve y^2 = x^3 + 4 but (mostly) OUTSIDE G1, shared by the host and the device tests of g1.h: random curve points (order divisible by
cofactor primes), points of small order 3, 11, 33 (a subgroup ladder runs through infinity and P = +-Q additions there) and their sums with G1 points.
Pure Python big integers (oracle/pyref.py)."""
import random

from oracle import pyref as pr

COFACTOR = 0x396c8c005555e1568c00aaab0000aaab                 # of E(Fp)
G1_GEN_BYTES = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


def small_order_and_random_curve_points(seed=381, trials=12):
    """-> [(trial, point)]: per trial a random curve point T, then for q in 3, 11, 33 the point S = [h / q][r]T (where it is not infinity) with S + G and
    S + [12345]G."""
    rnd = random.Random(seed)

    def random_curve_point():
        while True:
            x = rnd.randrange(pr.P)
            y2 = (x * x * x + 4) % pr.P
            y = pow(y2, (pr.P + 1) // 4, pr.P)
            if y * y % pr.P == y2:
                return (x, y)
    gen = pr.g1_uncompress(G1_GEN_BYTES)
    out = []
    for trial in range(trials):
        T = random_curve_point()
        cands = [T]
        full = pr.g1_mul(T, pr.R)                          # kills the G1 component: order divides the cofactor
        for q in (3, 11, 33):
            S = pr.g1_mul(full, COFACTOR // q) if full is not None else None
            if S is not None:
                cands += [S, pr.g1_add(S, gen), pr.g1_add(S, pr.g1_mul(gen, 12345))]
        out += [(trial, pt) for pt in cands if pt is not None]
    return out
