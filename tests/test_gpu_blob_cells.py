"""-m gpu: verify_blob_cell_proofs_batch (include/kzg355.h, "blobs against their EIP-7594 cell proofs").  Inputs are the
three fixture blobs of tests/golden/cells.json with their commitments and cell proofs.  Every comparison is byte for byte on the 176 bytes
r | [I(tau)]_1 | LL | RL per group: against the CPU (tests/blob_cell_cases.py) and against the composition a client writes without the call --
compute_cells, then verify_cell_kzg_proof_batch over the cells with the commitments repeated and the indices 0..127 -- which is the call's
definition.  The two interpolation routes, the two transcript routes, the device form and a handle over several devices must all give those bytes."""
import ctypes as C
import os
import subprocess

import pytest

import blob_cell_cases as bcc
import cell_device_cases as dcases
import cell_spec as cs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BADARGS = 1
INF = bcc.INF
ZERO_BLOB = bytes(131072)


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


def _load(kz, setup_bytes, devices):
    g1, g2 = setup_bytes
    env = dict(KZG355_MSM="bucket", KZG355_EXCHANGE="peer")          # no wide table per replica
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], devices=devices)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def s1(kz, setup_bytes):
    s = _load(kz, setup_bytes, None)
    yield s
    s.free()


@pytest.fixture(scope="module")
def s3(kz, setup_bytes):
    s = _load(kz, setup_bytes, [0, 0, 0])
    assert s.device_count == 3
    yield s
    s.free()


@pytest.fixture(scope="module")
def fx():
    return dcases.fixture()


def group(fx, blobs):
    """(blobs, commitments, cell proofs) of the fixture blobs `blobs`"""
    return [fx["blobs"][b] for b in blobs], [fx["C"][b] for b in blobs], [p for b in blobs for p in fx["P"][b]]


def norm(res):
    return ["BadArgs" if type(x).__name__ == "BadArgs" else x for x in res]


def composition(kz, s, groups):
    """what a client writes today: the cells back from compute_cells, then the cell batch check over repeated commitments and indices 0..127"""
    args = []
    for blobs, commitments, proofs in groups:
        cells = kz.Kzg._compute_cells(blobs, s, True, False)
        if any(isinstance(c, kz.BadArgs) for c in cells):
            args.append(None)
            continue
        args.append(bcc.group_args([[x.to_bytes() for x in c[0]] for c in cells], commitments, proofs))
    good = [a for a in args if a is not None]
    res, out = kz.Kzg.debug_cell_batch_intermediates(good, s)
    it = iter(zip(norm(res), out))
    return [next(it) if a is not None else ("BadArgs", None) for a in args]


def call(kz, s, groups, interp_form=0):
    res, out = kz.Kzg.debug_blob_cell_batch_intermediates(groups, s, interp_form)
    return list(zip(norm(res), out))


def same_where_defined(got, want):
    """verdicts everywhere, bytes wherever the group has an answer (a refused group's 176 bytes are unspecified)"""
    assert [g[0] for g in got] == [w[0] for w in want]
    for t, (g, w) in enumerate(zip(got, want)):
        if w[0] != "BadArgs":
            assert g[1] == w[1], t


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("n", [1, 2, 3])
def test_groups_of_n_blobs_equal_the_composition(kz, oracle, s1, fx, n):
    groups = [group(fx, order[:n]) for order in ([0, 1, 2], [2, 0, 1])]
    got = call(kz, s1, groups)
    assert [g[0] for g in got] == [True, True]
    same_where_defined(got, composition(kz, s1, groups))
    assert kz.Kzg.verify_blob_cell_proofs_batch_many(groups, s1) == [True, True]
    if n == 1:                                                    # the CPU's answer
        out, ok = bcc.expected(oracle, [fx["cells"][0]], [fx["C"][0]], fx["P"][0])
        assert (ok, out) == got[0]


def test_the_two_interpolation_routes_give_the_same_bytes(kz, s1, fx):
    groups = [group(fx, [0, 1]), group(fx, [1, 1]), group(fx, [2, 0])]
    one, two = call(kz, s1, groups, 1), call(kz, s1, groups, 2)
    assert one == two == call(kz, s1, groups, 0) and [g[0] for g in one] == [True] * 3
    # a wrong group: the routes agree on its bytes too
    bad = list(groups)
    bad[1] = (groups[1][0], groups[1][1], groups[1][2][::-1])
    one, two = call(kz, s1, bad, 1), call(kz, s1, bad, 2)
    assert one == two and [g[0] for g in one] == [True, False, True]


def test_the_same_blob_twice_and_the_zero_blob(kz, oracle, s1, fx):
    twice = group(fx, [1, 1])
    got = call(kz, s1, [twice, group(fx, [1, 2])])
    same_where_defined(got, composition(kz, s1, [twice, group(fx, [1, 2])]))
    assert got[0][0] is True
    # one unique commitment in the transcript: r is the CPU's over [C, C] deduplicated
    r, uniq, _ = cs.challenge(*bcc.group_args([fx["cells"][1]] * 2, twice[1], twice[2]))
    assert uniq == [fx["C"][1]] and got[0][1][:32] == r.to_bytes(32, "big")
    zero = ([ZERO_BLOB], [INF], [INF] * 128)
    got = call(kz, s1, [zero])
    assert got[0][0] is True and got[0][1][32:] == INF * 3
    assert got[0] == (bcc.expected(oracle, [[bytes(2048)] * 128], [INF], [INF] * 128)[::-1])
    assert kz.Kzg.verify_blob_cell_proofs_batch(*zero, s1) is True


def spoiled(fx, oracle):
    """[(what, group, expected verdict)] on groups of two blobs; every spoil changes bytes"""
    blobs, commitments, proofs = group(fx, [0, 1])
    out = [("good", (blobs, commitments, proofs), True)]
    p = list(proofs); p[5], p[130] = p[130], p[5]
    out.append(("swapped proof", (blobs, commitments, p), False))
    b1 = bytearray(blobs[1]); b1[32 * 100 + 31] ^= 1
    out.append(("blob element changed", ([blobs[0], bytes(b1)], commitments, proofs), False))
    out.append(("another blob's commitment", (blobs, [commitments[0], fx["C"][2]], proofs), False))
    out.append(("good again", group(fx, [2, 1]), True))
    br = blobs[0][:32 * 77] + cs.R.to_bytes(32, "big") + blobs[0][32 * 78:]
    out.append(("blob element = r", ([br, blobs[1]], commitments, proofs), "BadArgs"))
    off = dcases.off_curve(oracle)
    out.append(("off-curve proof", (blobs, commitments, proofs[:200] + [off] + proofs[201:]), "BadArgs"))
    out.append(("good at the end", group(fx, [1, 0]), True))
    base = out[0][1]
    for what, g, _ in out[1:4] + out[5:7]:
        assert g != base and [len(x) for x in g] == [2, 2, 256], what
    return out


def test_one_spoiled_group_leaves_the_others_alone(kz, oracle, s1, fx):
    cases = spoiled(fx, oracle)
    groups = [g for _, g, _ in cases]
    got = call(kz, s1, groups)
    assert [g[0] for g in got] == [want for _, _, want in cases], [what for what, _, _ in cases]
    same_where_defined(got, composition(kz, s1, groups))
    # the good groups alone: their bytes do not depend on their neighbours
    alone = call(kz, s1, [g for _, g, want in cases if want is True])
    assert alone == [g for g, (_, _, want) in zip(got, cases) if want is True]
    # statuses and the return value through the C ABI
    G = len(groups)
    ok, st = (C.c_bool * G)(), (C.c_int * G)(*([7] * G))
    rc = kz.kzg.lib().kzg355_verify_blob_cell_proofs_batch_many(ok, st, b"".join(b"".join(g[0]) for g in groups), b"".join(b"".join(g[1]) for g in groups),
                                                                b"".join(b"".join(g[2]) for g in groups), 2, G, s1.handle)
    assert rc == BADARGS and list(st) == [BADARGS if want == "BadArgs" else 0 for _, _, want in cases]
    assert [bool(x) for x in ok] == [want is True for _, _, want in cases]


def test_edge_counts_and_lengths(kz, s1, fx):
    L = kz.kzg.lib()
    blobs, commitments, proofs = group(fx, [0])
    b, c, p = b"".join(blobs), b"".join(commitments), b"".join(proofs)
    ok, st = (C.c_bool * 2)(False, False), (C.c_int * 2)(7, 7)
    assert L.kzg355_verify_blob_cell_proofs_batch_many(ok, st, None, None, None, 0, 2, s1.handle) == 0          # n_per_group == 0: true
    assert list(ok) == [True, True] and list(st) == [0, 0]
    dbg = C.create_string_buffer(b"\x55" * 352, 352)
    assert L.kzg355_debug_blob_cell_batch_intermediates(dbg, ok, st, None, None, None, 0, 2, 0, s1.handle) == 0 and dbg.raw == bytes(352)
    ok, st = (C.c_bool * 1)(False), (C.c_int * 1)(7)
    assert L.kzg355_verify_blob_cell_proofs_batch_many(ok, st, b, c, p, 1, 0, s1.handle) == 0 and st[0] == 7 and ok[0] is False      # groups == 0: untouched
    assert kz.Kzg.verify_blob_cell_proofs_batch([], [], [], s1) is True
    one = C.c_bool(False)
    for nb, nc, np_ in ((1, 2, 128), (1, 1, 127), (1, 1, 129), (2, 1, 128), (1, 0, 128)):
        assert L.kzg355_verify_blob_cell_proofs_batch(C.byref(one), b, nb, c, nc, p, np_, s1.handle) == BADARGS, (nb, nc, np_)
    assert L.kzg355_verify_blob_cell_proofs_batch(C.byref(one), b, 1, c, 1, p, 128, s1.handle) == 0 and one.value is True
    with pytest.raises(kz.BadArgs):
        kz.Kzg.verify_blob_cell_proofs_batch(blobs, commitments, proofs[:-1], s1)
    # what refuses a call as a whole, with a real handle: every status is marked
    for args in ((b, c, p, 2049, 3, 0), (None, c, p, 1, 3, 0), (b, c, p, 1, 3, 3), (b, c, p, 1, 3, -1)):
        ok, st, dbg = (C.c_bool * 3)(True, True, True), (C.c_int * 3)(7, 7, 7), C.create_string_buffer(176 * 3)
        assert L.kzg355_debug_blob_cell_batch_intermediates(dbg, ok, st, *args, s1.handle) == BADARGS
        assert list(st) == [BADARGS] * 3 and list(ok) == [False] * 3


# ------------------------------------------------------------------------------------------------ device form
def u8(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")


def to_device(groups):
    return (u8(b"".join(b"".join(g[0]) for g in groups)), u8(b"".join(b"".join(g[1]) for g in groups)), u8(b"".join(b"".join(g[2]) for g in groups)))


@pytest.mark.parametrize("prep_form", [1, 2])
def test_device_form_equals_the_host_form(kz, s1, fx, prep_form):
    groups = [group(fx, [0, 1]), (group(fx, [2, 2])[0], group(fx, [2, 2])[1], group(fx, [2, 0])[2])]      # true, false
    host = call(kz, s1, groups)
    assert [h[0] for h in host] == [True, False]
    d = to_device(groups)
    for interp_form in (1, 2):
        res, out = kz.Kzg.debug_blob_cell_batch_intermediates_device(*d, 2, 2, s1, interp_form, prep_form)
        assert list(zip(norm(res), out)) == host, interp_form
    assert kz.Kzg.verify_blob_cell_proofs_batch_many_device(*d, 2, 2, s1) == [True, False]
    # a misaligned device pointer refuses the call as a whole
    ok, st = (C.c_bool * 2)(True, True), (C.c_int * 2)(7, 7)
    rc = kz.kzg.lib().kzg355_verify_blob_cell_proofs_batch_many_device(ok, st, d[0].data_ptr(), d[1].data_ptr() + 8, d[2].data_ptr(), 2, 2, s1.handle)
    assert rc == BADARGS and list(st) == [BADARGS] * 2 and list(ok) == [False] * 2


def test_device_form_above_the_device_hash_cap(kz, s1, fx):
    """129 blobs in one group = 16512 cells, above the 16384 the device hashes: every prep_form takes the host's hash"""
    grp = ([fx["blobs"][0]] * 129, [fx["C"][0]] * 129, fx["P"][0] * 129)
    host = call(kz, s1, [grp])
    assert host[0][0] is True
    d = to_device([grp])
    for prep_form in (0, 1):
        res, out = kz.Kzg.debug_blob_cell_batch_intermediates_device(*d, 129, 1, s1, 0, prep_form)
        assert list(zip(norm(res), out)) == host, prep_form


# ------------------------------------------------------------------------------------------------ several devices
def test_groups_fan_out_over_three_replicas(kz, s1, s3, fx):
    groups = [group(fx, [0]), (group(fx, [1])[0], group(fx, [1])[1], group(fx, [2])[2]), group(fx, [2])]
    moved = lambda before: [a - b for a, b in zip(s3.cell_calls_per_device(), before)]      # noqa: E731
    before, ex = s3.cell_calls_per_device(), s3.exchange_stats()
    got = call(kz, s3, groups)
    assert moved(before) == [1, 1, 1], "one group per replica: every replica runs one launch set"
    assert got == call(kz, s1, groups) and [g[0] for g in got] == [True, False, True]
    before = s3.cell_calls_per_device()
    assert kz.Kzg.verify_blob_cell_proofs_batch_many(groups[:2], s3) == [True, False]
    assert moved(before) == [1, 1, 0], "a call uses as many replicas as it has groups"
    assert kz.Kzg.verify_blob_cell_proofs_batch(*groups[2], s3) is True
    assert moved(before) == [2, 1, 0] and s3.exchange_stats() == ex, "a group is never cut: no exchange"
    # device-resident arrays stay on the first replica
    d = to_device(groups)
    assert kz.Kzg.verify_blob_cell_proofs_batch_many_device(*d, 1, 3, s3) == [True, False, True]
    assert moved(before) == [3, 1, 0]


# ------------------------------------------------------------------------------------------------ the other surfaces
def test_python_c_and_cpp_paths_agree(kz, s1, fx, tmp_path):
    good = group(fx, [0, 2])
    bad = (good[0], good[1][::-1], good[2])
    for g, want in ((good, True), (bad, False)):
        assert kz.Kzg.verify_blob_cell_proofs_batch(*g, s1) is want
        assert kz.Kzg.verify_blob_cell_proofs_batch_many([g], s1) == [want]
    runner = os.path.join(HERE, "native", "cpp_blob_cell_runner")
    inp = str(tmp_path / "groups_in.bin")
    with open(inp, "wb") as f:
        for g in (good, bad):
            f.write(len(g[0]).to_bytes(4, "little") + b"".join(g[0]) + b"".join(g[1]) + b"".join(g[2]))
    out = subprocess.run([runner, os.path.join(HERE, "golden", "trusted_setup_g1.bin"), os.path.join(HERE, "golden", "trusted_setup_g2.bin"), inp],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["true", "false"]
