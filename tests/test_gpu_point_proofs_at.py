"""-m gpu: compute_kzg_proofs_at, openings of blobs at chosen points, each proof the commitment to its own quotient.
Expected values never come from the call under test: the reference's compute_kzg_proof vectors; kzg355_compute_kzg_proof_many of the same
handle on the same (blob, z) pairs with the blobs duplicated, byte for byte, on a bucket-form and a wide-table handle; closed forms (y = z^k
for the blob of X^k, ys = the blob itself on the whole domain); the round trip through verify_kzg_proof_many; chunk borders with the launch
count of the plan model; the device-resident form between guard bytes; statuses by position; replicas."""
import ctypes as C
import os
import random

import pytest

from oracle import pyref
from synth import random_blob
from test_point_plan_host import chunk_count
from vector_harness import ParseError, get_blob, parse_fixed

pytestmark = pytest.mark.gpu

R = pyref.R
BADARGS = 1
BLOB = 131072
ROOTS = pyref.compute_roots_of_unity(4096)                           # blob order: ROOTS[i] = w4096^rev12(i)
MONOMIALS = [1, 7, 8, 9, 511, 512, 4088, 4095]


def be(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, **options):
    g1, g2 = setup_bytes
    return kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], **options)


@pytest.fixture(scope="module")
def s8(kz, setup_bytes):
    """bucket form, no table"""
    s = _load(kz, setup_bytes, msm_bits=8)
    yield s
    s.free()


@pytest.fixture(scope="module")
def s12(kz, setup_bytes):
    """the smallest wide table"""
    s = _load(kz, setup_bytes, msm_bits=12)
    yield s
    s.free()


@pytest.fixture(scope="module", params=["bucket", "wide"])
def handle(request, s8, s12):
    return s8 if request.param == "bucket" else s12


def c_many(kz, s, blobs, lists, proofs=True, ys=True, status=True):
    """the host form through ctypes: (return value, statuses, proofs_out bytes, ys_out bytes)"""
    n = len(blobs)
    flat = [z for zs in lists for z in zs]
    total = len(flat)
    counts = (C.c_size_t * max(n, 1))(*[len(zs) for zs in lists])
    p_out = C.create_string_buffer(48 * max(total, 1)) if proofs else None
    y_out = C.create_string_buffer(32 * max(total, 1)) if ys else None
    st = (C.c_int * max(n, 1))(*([7] * max(n, 1))) if status else None
    rc = kz.kzg.lib().kzg355_compute_kzg_proofs_at_many(p_out, y_out, st, b"".join(blobs), n, counts, b"".join(flat), s.handle)
    return rc, list(st)[:n] if status else None, p_out.raw[:48 * total] if proofs else None, y_out.raw[:32 * total] if ys else None


def old_route(kz, s, pairs):
    """kzg355_compute_kzg_proof_many on the distinct (blob, z) pairs, the blobs duplicated: {(blob, z): (proof, y)}"""
    distinct = list(dict.fromkeys(pairs))
    n = len(distinct)
    out, ys, st = C.create_string_buffer(48 * n), C.create_string_buffer(32 * n), (C.c_int * n)()
    rc = kz.kzg.lib().kzg355_compute_kzg_proof_many(out, ys, st, b"".join(b for b, _ in distinct), b"".join(z for _, z in distinct), n, s.handle)
    assert rc == 0 and list(st) == [0] * n
    return {p: (out.raw[48 * i:48 * i + 48], ys.raw[32 * i:32 * i + 32]) for i, p in enumerate(distinct)}


def expected(kz, s, blobs, lists):
    want = old_route(kz, s, [(b, z) for b, zs in zip(blobs, lists) for z in zs])
    flat = [want[(b, z)] for b, zs in zip(blobs, lists) for z in zs]
    return b"".join(p for p, _ in flat), b"".join(y for _, y in flat)


# ---- 2. (the call that items 6 and 8 run again) against compute_kzg_proof_many, byte for byte
def shapes_call():
    """the zero blob, a constant, the evaluation forms of X^k, two seeded random blobs; points 0, 1, r - 1, w_m, a repeated point and seeded random
    ones, turned per blob so that the short lists see different ones; ragged counts, 130 above the cell calls' 128"""
    rng = random.Random(4844)
    blobs = [bytes(BLOB), be(5) * 4096] + [b"".join(be(pow(x, k, R)) for x in ROOTS) for k in MONOMIALS] + [random_blob(48440), random_blob(48441)]
    rnd = be(rng.randrange(R))
    special = [be(0), be(1), be(R - 1), be(ROOTS[0]), be(ROOTS[1]), be(ROOTS[2048]), be(ROOTS[4095]), rnd, rnd]
    counts = [9, 9, 1, 2, 9, 0, 2, 9, 1, 9, 130, 9]
    lists = []
    for i, c in enumerate(counts):
        turned = special[i % 9:] + special[:i % 9]
        lists.append((turned + [be(rng.randrange(R)) for _ in range(c)])[:c])
    return blobs, lists


@pytest.fixture(scope="module")
def shapes(kz, handle):
    blobs, lists = shapes_call()
    want_p, want_y = expected(kz, handle, blobs, lists)
    return blobs, lists, want_p, want_y


def test_equals_compute_kzg_proof_many(kz, handle, shapes):
    blobs, lists, want_p, want_y = shapes
    assert [len(zs) for zs in lists] == [9, 9, 1, 2, 9, 0, 2, 9, 1, 9, 130, 9]
    assert c_many(kz, handle, blobs, lists) == (0, [0] * len(blobs), want_p, want_y)
    assert c_many(kz, handle, blobs, lists, proofs=False) == (0, [0] * len(blobs), None, want_y)
    assert c_many(kz, handle, blobs, lists, ys=False, status=False) == (0, None, want_p, None)
    # y = z^k in closed form for the blob of X^k, 0 for the zero blob, the constant for the constant
    off = 0
    for i, zs in enumerate(lists):
        for j, z in enumerate(zs):
            zi, y = int.from_bytes(z, "big"), int.from_bytes(want_y[32 * (off + j):32 * (off + j + 1)], "big")
            if i < 2:
                assert y == (0, 5)[i]
            elif i < 2 + len(MONOMIALS):
                assert y == pow(zi, MONOMIALS[i - 2], R), (i, j)
        off += len(zs)
    # the wrappers: per blob lists, and the single call
    ps, ys, st = kz.Kzg.compute_kzg_proofs_at_many(blobs, lists, handle)
    assert st == [0] * len(blobs)
    assert b"".join(bytes(p) for row in ps for p in row) == want_p and b"".join(bytes(y) for row in ys for y in row) == want_y
    p4, y4 = kz.Kzg.compute_kzg_proofs_at(blobs[4], lists[4], handle)
    at = sum(len(zs) for zs in lists[:4])
    assert b"".join(bytes(p) for p in p4) == want_p[48 * at:48 * (at + 9)] and b"".join(bytes(y) for y in y4) == want_y[32 * at:32 * (at + 9)]
    only = kz.Kzg.compute_kzg_proofs_at(blobs[4], lists[4], handle, proofs=False)
    assert only[0] is None and [bytes(v) for v in only[1]] == [bytes(v) for v in y4]
    # the C entry point of one blob, and no point at all
    lib, out = kz.kzg.lib(), C.create_string_buffer(48 * 9)
    assert lib.kzg355_compute_kzg_proofs_at(out, None, blobs[4], b"".join(lists[4]), 9, handle.handle) == 0 and out.raw == want_p[48 * at:48 * (at + 9)]
    assert lib.kzg355_compute_kzg_proofs_at(out, None, blobs[4], None, 0, handle.handle) == 0
    assert lib.kzg355_compute_kzg_proofs_at(None, None, blobs[4], b"".join(lists[4]), 9, handle.handle) == BADARGS


# ---- 1. the reference's vectors, grouped under their blobs, in one call
def test_reference_vectors_in_one_call(kz, handle, golden_vectors, golden_blobs):
    groups, order = {}, []
    for case in golden_vectors["compute_kzg_proof"]:
        try:
            blob = get_blob(case["input"]["blob"], golden_blobs)
            z = parse_fixed(case["input"]["z"], 32)
        except ParseError:
            assert case["output"] is None                        # (a blob or a z of another length never reaches a call of fixed strides)
            continue
        if blob not in groups:
            groups[blob] = []
            order.append(blob)
        groups[blob].append((z, case))
    # 46 vectors: two blobs and two points of a wrong length stay outside; 36 valid ones, two blobs with an element >= r, four points >= r
    assert sum(len(g) for g in groups.values()) == 42 and len(golden_vectors["compute_kzg_proof"]) == 46
    # a blob with an invalid point is refused as a whole, so its valid vectors go into a group of their own under the same blob
    blobs, lists, cases = [], [], []
    for blob in order:
        good = [(z, c) for z, c in groups[blob] if int.from_bytes(z, "big") < R]
        bad = [(z, c) for z, c in groups[blob] if int.from_bytes(z, "big") >= R]
        for part in ([good] if good else []) + [[zc] for zc in bad]:
            blobs.append(blob), lists.append([z for z, _ in part]), cases.append([c for _, c in part])
    rc, st, p, y = c_many(kz, handle, blobs, lists)
    off, refused = 0, 0
    for i, cs_ in enumerate(cases):
        if any(c["output"] is None for c in cs_):
            assert all(c["output"] is None for c in cs_) and st[i] == BADARGS, cs_[0]["name"]
            refused += 1
        else:
            assert st[i] == 0
            for j, c in enumerate(cs_):
                assert p[48 * (off + j):48 * (off + j + 1)] == bytes.fromhex(c["output"][0][2:]), c["name"]
                assert y[32 * (off + j):32 * (off + j + 1)] == bytes.fromhex(c["output"][1][2:]), c["name"]
        off += len(cs_)
    assert refused == 6 and rc == BADARGS and sum(len(c) for c, t in zip(cases, st) if t == 0) == 36


# ---- 3. the whole domain
def test_whole_domain_ys_are_the_blob(kz, setup_bytes):
    s = _load(kz, setup_bytes, msm_bits=12)
    try:
        blob = random_blob(48442)
        rc, st, _, y = c_many(kz, s, [blob], [[be(x) for x in ROOTS]], proofs=False)
        assert (rc, st) == (0, [0]) and y == blob
        assert s.msm_shape()[0] == 0                             # no table was built: no proof was asked for
    finally:
        s.free()


# ---- 4. round trip
def test_round_trip_through_verify(kz, handle):
    rng = random.Random(44)
    blobs = [random_blob(48443), random_blob(48444)]
    lists = [[be(ROOTS[rng.randrange(4096)]) for _ in range(32)] + [be(rng.randrange(R)) for _ in range(32)] for _ in blobs]
    rc, st, p, y = c_many(kz, handle, blobs, lists)
    assert (rc, st) == (0, [0, 0])
    cms = [bytes(kz.Kzg.blob_to_kzg_commitment(kz.Blob(b), handle)) for b in blobs]
    flat_c, flat_z = [cms[i] for i in range(2) for _ in range(64)], [z for zs in lists for z in zs]
    ys, ps = [y[32 * j:32 * j + 32] for j in range(128)], [p[48 * j:48 * j + 48] for j in range(128)]
    assert kz.Kzg.verify_kzg_proof_many(flat_c, flat_z, ys, ps, handle) == [True] * 128
    ys[70] = be((int.from_bytes(ys[70], "big") + 1) % R)
    assert kz.Kzg.verify_kzg_proof_many(flat_c, flat_z, ys, ps, handle) == [True] * 70 + [False] + [True] * 57


# ---- 5. chunk borders
def launches(kz, s, family):
    total, count = C.c_double(), C.c_long()
    assert kz.kzg.lib().kzg355_kernel_ms_stats(s.handle, family.encode(), C.byref(total), C.byref(count)) == 0
    return count.value


@pytest.mark.parametrize("proofs", [True, False], ids=["proofs", "ys_only"])
def test_a_blob_cut_at_the_chunk_border(kz, s8, proofs):
    rng = random.Random(1153)
    blobs = [random_blob(48450 + i) for i in range(4)]
    pool = [be(rng.randrange(R)) for _ in range(60)] + [be(ROOTS[i]) for i in (0, 1, 77, 4095)]
    lists = [[pool[rng.randrange(len(pool))] for _ in range(1153)], [pool[3]], [], [pool[0], pool[61], pool[5], pool[5], pool[63]]]
    want_p, want_y = expected(kz, s8, blobs, lists)
    s8.set_kernel_timing(True)
    kz.kzg.lib().kzg355_reset_kernel_stats(s8.handle)
    try:
        got = c_many(kz, s8, blobs, lists, proofs=proofs)
        assert launches(kz, s8, "pq_quotient") == chunk_count([len(zs) for zs in lists]) == 2
    finally:
        s8.set_kernel_timing(False)
    assert got == (0, [0] * 4, want_p if proofs else None, want_y)


def test_513_blobs_of_one_point(kz, s8):
    rng = random.Random(513)
    distinct = [random_blob(48460 + i) for i in range(4)]
    blobs = [distinct[i % 4] for i in range(513)]
    lists = [[be(ROOTS[i]) if i % 64 == 0 else be(rng.randrange(R))] for i in range(513)]
    _, want_y = expected(kz, s8, blobs, lists)
    s8.set_kernel_timing(True)
    kz.kzg.lib().kzg355_reset_kernel_stats(s8.handle)
    try:
        got = c_many(kz, s8, blobs, lists, proofs=False)
        assert launches(kz, s8, "pq_quotient") == chunk_count([1] * 513) == 2
    finally:
        s8.set_kernel_timing(False)
    assert got == (0, [0] * 513, None, want_y)


# ---- 6. the device form
GUARD = 64


def test_device_form_between_guards(kz, handle, shapes):
    import torch
    blobs, lists, want_p, want_y = shapes
    n, counts, zs = len(blobs), [len(x) for x in lists], b"".join(z for x in lists for z in x)
    total = sum(counts)

    def guarded(size, fill=None):
        t = torch.full((GUARD + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        if fill is not None:
            t[GUARD:GUARD + size] = torch.frombuffer(bytearray(fill), dtype=torch.uint8).cuda()
        return t

    def inner(t, size):
        raw = bytes(t.cpu().numpy())
        assert raw[:GUARD] == b"\xa5" * GUARD and raw[GUARD + size:] == b"\xa5" * GUARD
        return raw[GUARD:GUARD + size]

    d_blobs = guarded(BLOB * n, b"".join(blobs))
    for proofs, ys in ((True, True), (True, False), (False, True)):
        dp, dy = guarded(48 * total) if proofs else None, guarded(32 * total) if ys else None
        res = kz.Kzg.compute_kzg_proofs_at_many_device(d_blobs[GUARD:GUARD + BLOB * n], n, counts, zs, handle,
                                                       proofs_out=None if dp is None else dp[GUARD:GUARD + 48 * total],
                                                       ys_out=None if dy is None else dy[GUARD:GUARD + 32 * total])
        assert res == [None] * n
        assert dp is None or inner(dp, 48 * total) == want_p
        assert dy is None or inner(dy, 32 * total) == want_y
        assert inner(d_blobs, BLOB * n) == b"".join(blobs)
    # a pointer misaligned by 8 refuses the call as a whole
    dp, dy = guarded(48 * total), guarded(32 * total)
    cn = (C.c_size_t * n)(*counts)
    call = kz.kzg.lib().kzg355_compute_kzg_proofs_at_many_device
    for shift in ((8, 0, 0), (0, 8, 0), (0, 0, 8)):
        st = (C.c_int * n)(*([7] * n))
        assert call(dp.data_ptr() + GUARD + shift[0], dy.data_ptr() + GUARD + shift[1], st, d_blobs.data_ptr() + GUARD + shift[2], n, cn, zs,
                    handle.handle) == BADARGS
        assert list(st) == [BADARGS] * n
    assert inner(dp, 48 * total) == b"\xa5" * (48 * total) and inner(dy, 32 * total) == b"\xa5" * (32 * total)
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at_many_device(d_blobs[GUARD:GUARD + BLOB * n], n, counts, zs, handle)


# ---- 7. statuses by position
def test_status_by_position(kz, handle):
    rng = random.Random(7)
    good = [random_blob(48470 + i) for i in range(3)]
    spoiled = good[1][:32 * 9] + be(R) + good[1][32 * 10:]
    zs = [[be(rng.randrange(R)), be(ROOTS[5])], [be(rng.randrange(R)) for _ in range(3)], [be(ROOTS[9])]]
    want_p, want_y = expected(kz, handle, good, zs)
    cut = [2, 5, 6]                                                  # the slots where blobs 0, 1 and 2 end
    bad_lists = {"element": zs[1], "point_r": [zs[1][0], be(R), zs[1][2]], "point_ff": [zs[1][0], zs[1][1], b"\xff" * 32]}
    for name, mid in bad_lists.items():
        bad_blob = spoiled if name == "element" else good[1]
        for pos in (0, 1, 2):
            others = [good[0], good[2]]
            other_z = [zs[0], zs[2]]
            blobs = others[:pos] + [bad_blob] + others[pos:]
            lists = other_z[:pos] + [mid] + other_z[pos:]
            rc, st, p, y = c_many(kz, handle, blobs, lists)
            assert rc == BADARGS and st == [BADARGS if i == pos else 0 for i in range(3)], (name, pos)
            off = 0
            for i, lst in enumerate(lists):
                if i != pos:
                    src = (0, cut[0]) if lst is zs[0] else (cut[1], cut[2])
                    assert p[48 * off:48 * (off + len(lst))] == want_p[48 * src[0]:48 * src[1]], (name, pos, i)
                    assert y[32 * off:32 * (off + len(lst))] == want_y[32 * src[0]:32 * src[1]], (name, pos, i)
                off += len(lst)
            assert c_many(kz, handle, blobs, lists, status=False)[0] == BADARGS
    with pytest.raises(kz.BadArgs):
        kz.Kzg.compute_kzg_proofs_at(good[1], bad_lists["point_r"], handle)
    ps, ys, st = kz.Kzg.compute_kzg_proofs_at_many([good[0], spoiled, good[2]], zs, handle)
    assert st == [0, BADARGS, 0] and ps[1] is None and ys[1] is None and b"".join(bytes(q) for q in ps[0]) == want_p[:48 * 2]
    # a count of 0 is no error and shifts nothing; its blob is still checked
    assert c_many(kz, handle, good, [zs[0], [], zs[2]]) == (0, [0, 0, 0], want_p[:96] + want_p[240:], want_y[:64] + want_y[160:])
    assert c_many(kz, handle, [good[0], spoiled, good[2]], [zs[0], [], zs[2]])[:2] == (BADARGS, [0, BADARGS, 0])


# ---- 8. replicas on one card
def test_replicas(kz, s8, setup_bytes):
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer")     # no wide table per replica
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s3 = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], devices=[0, 0, 0])
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        assert s3.device_count == 3
        blobs, lists = shapes_call()
        single = c_many(kz, s8, blobs, lists)
        assert single[:2] == (0, [0] * len(blobs))
        before = s3.cell_calls_per_device()
        assert c_many(kz, s3, blobs, lists) == single
        assert [a - b for a, b in zip(s3.cell_calls_per_device(), before)] == [1, 1, 1]      # one set per range of 4 blobs
        # a refusal lands at its own position on its own replica
        lists[6] = [be(R)]
        rc, st, p, y = c_many(kz, s3, blobs, lists)
        assert (rc, st) == (BADARGS, [BADARGS if i == 6 else 0 for i in range(len(blobs))])
        at = sum(len(zs) for zs in lists[:6])
        assert (p[:48 * at], y[:32 * at]) == (single[2][:48 * at], single[3][:32 * at])
        assert (p[48 * (at + 1):], y[32 * (at + 1):]) == (single[2][48 * (at + 2):], single[3][32 * (at + 2):])      # (the list had 2 points)
    finally:
        s3.free()


def test_minimal_preset_handle_refuses(kz, setup_bytes):
    import json
    from kzg_rust_amd import kzg_minimal as km
    here = os.path.dirname(os.path.abspath(__file__))
    mfx = json.load(open(os.path.join(here, "golden", "minimal.json")))
    g2 = setup_bytes[1]
    sm = km.Kzg.load_trusted_setup([bytes.fromhex(x) for x in mfx["setup_g1_lagrange"]], [g2[96 * i:96 * i + 96] for i in range(65)])
    try:
        blob = random_blob(48443)
        assert c_many(kz, sm, [blob, blob], [[be(1)], [be(2)]])[:2] == (BADARGS, [BADARGS, BADARGS])
    finally:
        sm.free()
