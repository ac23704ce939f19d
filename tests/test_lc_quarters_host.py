"""The quarters form of the bucket linear combination, on the host: the split of a scalar by m = |x| (g1.h), the signed recoding, the group
identity behind it against the Python reference, the constant [m](-G), the dealing of the bucket kernel's tasks to its four waves and the
limits derived from it (kzg_rust_amd/csrc/lc_forms.h, compiled for the host in tests/native/lc_forms_probe.cpp)."""
import ctypes as C
import os
import random
import subprocess

import pytest

from oracle import pyref as M

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(HERE, "..", "kzg_rust_amd", "csrc")
SRC = os.path.join(NATIVE, "lc_forms_probe.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("field.h", "g1.h", "lc_forms.h", "modinv.h", "consts_gen.h")]
m = M.X_ABS
R = M.R
BETA = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


@pytest.fixture(scope="module")
def lp():
    so = os.path.join(NATIVE, "liblc_forms_probe.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return C.CDLL(so)


def _words(v, n):
    return (C.c_uint32 * n)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)])


def _split(lp, k):
    out = (C.c_uint32 * 8)()
    lp.lcp_quarter_split(out, _words(k, 8))
    return [out[2 * j] | (out[2 * j + 1] << 32) for j in range(4)]


def _digits(lp, a):
    d = (C.c_int8 * 16)()
    nw = lp.lcp_recode_quarter(d, _words(a, 2))
    return list(d)[:nw]


def _params(lp, form):
    out = (C.c_int * 8)()
    lp.lcp_params(form, out)
    return dict(zip(("bits", "windows", "per_term", "nb", "dig_stride", "tb", "maxt", "lds_entries"), out))


def _deal(lp, form):
    nt, task = (C.c_uint8 * 4)(), (C.c_uint8 * (4 * 13))()
    lp.lcp_deal(form, nt, task)
    return [[(task[13 * w + t] & 31, (task[13 * w + t] >> 5) & 1, task[13 * w + t] >> 6) for t in range(nt[w])] for w in range(4)]


SCALARS = [0, 1, m - 1, m, m * m - 1, m * m, m ** 3, R - 1]


def test_group_order_is_below_m4():
    assert R == m ** 4 - m ** 2 + 1 and R < m ** 4 and m < 1 << 64


def test_split_and_recoding(lp):
    p = _params(lp, 1)
    assert p["per_term"] == 4 and p["windows"] == (64 - 1) // p["bits"] + 1 and p["nb"] == 1 << (p["bits"] - 1)
    rnd = random.Random(7594)
    for k in SCALARS + [rnd.randrange(R) for _ in range(10000)]:
        a = _split(lp, k)
        assert sum(a[j] * m ** j for j in range(4)) == k, hex(k)
        assert all(x < m for x in a), hex(k)
        for x in a:
            d = _digits(lp, x)
            assert len(d) == p["windows"]
            assert sum(dw << (p["bits"] * w) for w, dw in enumerate(d)) == x, hex(x)
            assert all(-p["nb"] <= dw < p["nb"] for dw in d[:-1])
            assert 0 <= d[-1] <= 13, hex(x)


def test_halves_recoding_is_what_it_was(lp):
    """The same recoding body serves the halves: 25 signed 5-bit digits and a top digit, against the formula it replaced."""
    bias = sum(16 << (5 * w) for w in range(25))
    rnd = random.Random(5)
    for v in [0, 1, (1 << 128) - 1, m * m - 1] + [rnd.randrange(m * m) for _ in range(2000)]:
        d = (C.c_int8 * 28)()
        assert lp.lcp_recode_half(d, _words(v, 4)) == 26
        e = v + bias
        want = [((e >> (5 * w)) & 31) - 16 for w in range(25)] + [(e >> 125) & 31]
        assert list(d)[:26] == want


def test_identity_against_the_reference(lp):
    """[k]P = [a0]P + [a1]Q + [a2](-phi P) + [a3](-phi Q) with Q = [m]P, on a few points of G1."""
    rnd = random.Random(381)
    neg_phi = lambda pt: (BETA * pt[0] % M.P, (-pt[1]) % M.P)
    for t in range(4):
        Pt = M.g1_mul(M.G1_GEN, rnd.randrange(1, R))
        Q = M.g1_mul(Pt, m)
        assert neg_phi(Pt) == M.g1_mul(Pt, m * m)                 # [m^2] = -phi on G1
        for k in [SCALARS[2 * t], SCALARS[2 * t + 1], rnd.randrange(R)]:
            a = _split(lp, k)
            acc = None
            for pt, s in zip((Pt, Q, neg_phi(Pt), neg_phi(Q)), a):
                acc = M.g1_add(acc, M.g1_mul(pt, s))
            assert acc == M.g1_mul(Pt, k), hex(k)


def test_constant_m_times_neg_generator(lp):
    out = C.create_string_buffer(96)
    lp.lcp_neg_gen_x_abs(out)
    got = (int.from_bytes(out.raw[:48], "big"), int.from_bytes(out.raw[48:], "big"))
    assert got == M.g1_mul(M.g1_neg(M.G1_GEN), m)


def test_every_task_is_dealt_once(lp):
    for form in (0, 1):
        p, deal = _params(lp, form), _deal(lp, form)
        tasks = [t for wave in deal for t in wave]
        parts = p["nb"] // p["tb"]
        assert sorted(tasks) == sorted((w, c, q) for w in range(p["windows"]) for c in range(2) for q in range(parts))
        assert all(len(wave) <= p["maxt"] and p["tb"] * len(wave) <= 255 for wave in deal)       # list ranks are uint8_t


def test_wave_balance_quarters(lp):
    """Additions per wave of the bucket kernel at n = 64, from the digits of random scalars: the busiest wave is at most 3 % over the mean.
    A single batch scatters by about 1.5 % around its expectation (a digit falls into the lower or the upper half of the buckets with probability
    1/2), so the bound is put on the mean over 200 batches, which is what the kernel's time per launch set follows."""
    p, deal = _params(lp, 1), _deal(lp, 1)
    n, batches = 64, 200
    rnd = random.Random(64)
    tot = [0.0] * 4
    for _ in range(batches):
        cnt = {}
        for cls, terms in ((0, n), (1, 2 * n + 1)):
            for _t in range(terms):
                for a in _split(lp, rnd.randrange(R)):
                    for w, d in enumerate(_digits(lp, a)):
                        if d:
                            key = (w, cls, (abs(d) - 1) // p["tb"])
                            cnt[key] = cnt.get(key, 0) + 1
        for wv in range(4):
            tot[wv] += sum(cnt.get(t, 0) for t in deal[wv])
    mean = sum(tot) / 4
    print("additions per wave and batch:", [round(x / batches, 1) for x in tot], "mean", round(mean / batches, 1))
    assert max(tot) <= 1.03 * mean
    # the count of the form: 8.4 k insertions per batch
    assert 8200 <= sum(tot) / batches <= 8500 or p["bits"] != 6


def test_limits(lp):
    """What the kernel's fixed-size fields allow, re-derived from the dealing: item indices are 15 bits beside the sign, the lists of the busiest
    wave fit the LDS up to a threshold n and a global slab beyond it."""
    for form in (0, 1):
        p, deal = _params(lp, form), _deal(lp, form)
        cls_items = lambda c, n: p["per_term"] * (2 * n + 1 if c else n)
        for n in (8, 64, 129, 130, 500, 2730, 2731, 4096):
            want = max(sum(cls_items(c, n) for (_w, c) in {(w, c) for (w, c, _q) in wave}) for wave in deal)
            assert lp.lcp_max_entries(form, n) == want
            assert bool(lp.lcp_lists_in_lds(form, n)) == (want <= p["lds_entries"])
            assert bool(lp.lcp_items_fit(form, n)) == (n >= 8 and p["per_term"] * (3 * n + 1) <= 0x7FFF)
    assert [n for n in range(8, 400) if not lp.lcp_lists_in_lds(0, n)][0] == 130       # halves: 40 n + 14 <= 5200, as before


def test_probe_under_sanitizers(tmp_path):
    """The split, the recoding and the dealing as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
    exe = str(tmp_path / "lc_forms_probe_san")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DLC_PROBE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
