"""-m gpu: compute_cells_and_kzg_proofs at its data-dependent corners, the device against the oracle byte for byte (cells against
cell_spec.compute_cells, H_0 .. H_62 against fk20_spec.h_points, the 128 proofs against fk20_spec.proofs_from_h), through single calls and one
_many call holding every blob.  The blobs are built from chosen circulant columns (tests/fk20_spec.py), so the fixed-base scalars C_r[i] of
k_cc_msm are known:
  * comb digit corners: k* = 14 16^63 - r, whose last comb addition must double (the lazy addition's fp_maybe_zero_lz fallback), in every lane
    of every bin, in one lane next to 63 other corner scalars, and in one bin of one column;
  * the point at infinity at chosen places: lanes (odd columns zero), bins of Z (columns vanishing there), and H_e (low-degree blobs);
  * the field stage's boundaries: all r-1, r-1 / 0 alternating, and values >= r at the ends of the blob and of its halves;
  * per-blob statuses across the 512-blob chunks of a 1030-blob _many call, for each output form, through the C ABI;
  * the cell verifier (device and CPU restatement) on the special outputs: infinity commitments and proofs, constant and degree < 128 blobs."""
import ctypes as C
import json
import os
import random

import pytest

import cell_spec as cs
import fk20_spec as fk
from synth import random_blob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = cs.R
INF = fk.G1_INF
BADARGS = 1
CELL_BYTES = 128 * cs.BYTES_PER_CELL
PROOF_BYTES = 128 * 48


@pytest.fixture(scope="module")
def kz():
    import kzg_rust_amd
    return kzg_rust_amd


@pytest.fixture(scope="module")
def settings(kz, setup_bytes):
    g1, g2 = setup_bytes
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    yield s
    s.free()


@pytest.fixture(scope="module")
def mono():
    return cs.load_monomial()


def raw(xs):
    return [bytes(x) for x in xs]


def blob_of_values(vals):
    return b"".join((v % R).to_bytes(32, "big") for v in vals)


def random_column(rng):
    return [rng.randrange(R), rng.randrange(R)]


# ---- the edge blobs, by group: (name, blob); their oracle answers are computed once per module
def edge_groups():
    rng = random.Random(0xedce)
    corpus = [k for _, k in fk.comb_corpus()]
    ks = corpus.index(fk.K_STAR)
    g = {}
    g["comb_every_lane"] = [("k* in every column", fk.column_blob([fk.K_STAR] * 64))]
    g["comb_lanes_diverge"] = [("corpus[0:64]", fk.column_blob(corpus[:64])),
                               ("corpus[8:72] reversed", fk.column_blob(corpus[8:72][::-1]))]        # k* in lane 0, then lane 63
    one_bin = []
    for i0, r0 in ((0, 0), (1, 21), (64, 42), (127, 63)):
        cols = [random_column(rng) for _ in range(64)]
        cols[r0] = fk.column_pair(fk.K_STAR, i0, rng.randrange(R))
        one_bin.append((f"k* at bin {i0} of column {r0}", fk.columns_blob(cols)))
    g["comb_one_bin"] = one_bin
    g["inf_lanes"] = [("odd columns zero", fk.columns_blob([random_column(rng) if r % 2 == 0 else [0] for r in range(64)]))]
    g["inf_bins"] = [(f"Z = inf at bins {bins}", fk.columns_blob([fk.column_vanishing(bins, [rng.randrange(1, R) for _ in range(3)]) for _ in range(64)]))
                     for bins in ((0, 5, 64, 127), (63,))]
    g["low_degree"] = [(f"degree < {64 * j}", fk.blob_from_coefficients([rng.randrange(R) for _ in range(64 * j)])) for j in (1, 2, 3, 33)]
    return g


@pytest.fixture(scope="module")
def edges(oracle, mono):
    out = {}
    for group, blobs in edge_groups().items():
        out[group] = []
        for name, blob in blobs:
            H = fk.h_points(oracle, blob, mono)
            out[group].append((name, blob, (cs.compute_cells(blob), H, fk.proofs_from_h(oracle, H))))
    return out


def check_single(kz, settings, name, blob, want):
    cells, H, proofs = want
    c, p = kz.Kzg.compute_cells_and_kzg_proofs(blob, settings)
    assert raw(c) == cells, name
    [h] = kz.Kzg.debug_cell_compute_h([blob], settings)
    assert h[:63] == H, (name, [e for e in range(63) if h[e] != H[e]])
    assert h[63] == INF, name
    assert raw(p) == proofs, (name, [k for k in range(128) if bytes(p[k]) != proofs[k]])


def check_group(kz, settings, edges, group):
    for name, blob, want in edges[group]:
        check_single(kz, settings, name, blob, want)


def test_comb_doubling_in_every_lane_of_every_bin(kz, settings, edges):
    # C_r[i] = k* for all r, i: all 8192 lanes' last additions double
    assert fk.comb_doubling_windows(fk.K_STAR) == [("dbl", 63)]
    check_group(kz, settings, edges, "comb_every_lane")


def test_comb_corner_scalars_across_lanes(kz, settings, edges):
    # 64 different corner scalars per bin, k* among them: the lanes of a wave take different branches, one lane per bin doubles
    for name, k in fk.comb_corpus():
        assert fk.from_digits(fk.comb_digits(k)) == k and fk.comb_digits(k)[63] >= 0, name
    check_group(kz, settings, edges, "comb_lanes_diverge")


def test_comb_doubling_in_one_bin(kz, settings, edges):
    check_group(kz, settings, edges, "comb_one_bin")


def test_infinity_in_half_the_lanes(kz, settings, edges):
    check_group(kz, settings, edges, "inf_lanes")


def test_infinity_in_chosen_bins_of_z(kz, settings, edges):
    check_group(kz, settings, edges, "inf_bins")


def test_low_degree_blobs(kz, settings, edges):
    for (name, blob, (cells, H, proofs)), j in zip(edges["low_degree"], (1, 2, 3, 33)):
        assert H[j - 1:] == [INF] * (64 - j) and INF not in H[:j - 1], name
        if j == 1:
            assert proofs == [INF] * 128
        if j == 2:
            assert proofs == [H[0]] * 128
    check_group(kz, settings, edges, "low_degree")


def test_all_edge_blobs_in_one_many_call(kz, settings, edges):
    flat = [(name, blob, want) for group in edges.values() for name, blob, want in group]
    res = kz.Kzg.compute_cells_and_kzg_proofs_many([b for _, b, _ in flat], settings)
    hs = kz.Kzg.debug_cell_compute_h([b for _, b, _ in flat], settings)
    for (name, _, (cells, H, proofs)), (c, p), h in zip(flat, res, hs):
        assert raw(c) == cells, name
        assert raw(p) == proofs, name
        assert h == H + [INF], name


# ---- field-stage boundaries
def test_constant_r_minus_1(kz, settings):
    blob = blob_of_values([R - 1] * cs.N_FE)
    cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(blob, settings)
    assert raw(cells) == [(R - 1).to_bytes(32, "big") * 64] * 128
    assert raw(proofs) == [INF] * 128
    assert kz.Kzg.debug_cell_compute_h([blob], settings)[0] == [INF] * 64
    [(c, p)] = kz.Kzg.compute_cells_and_kzg_proofs_many([blob], settings)
    assert (raw(c), raw(p)) == (raw(cells), raw(proofs))


def test_alternating_r_minus_1_and_zero(kz, settings, oracle, oracle_settings, mono):
    blob = blob_of_values([R - 1 if i % 2 == 0 else 0 for i in range(cs.N_FE)])
    cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(blob, settings)
    assert raw(cells) == cs.compute_cells(blob)
    com = oracle.blob_to_kzg_commitment(blob, oracle_settings)
    assert cs.verify_cell_kzg_proof_batch(oracle, [com] * 128, list(range(128)), raw(cells), raw(proofs), mono=mono) is True
    assert cs.cell_proofs(oracle, blob, mono, cells=[0, 127]) == [bytes(proofs[0]), bytes(proofs[127])]
    [(c, p)] = kz.Kzg.compute_cells_and_kzg_proofs_many([blob], settings)
    assert (raw(c), raw(p)) == (raw(cells), raw(proofs))


@pytest.mark.parametrize("value", [R, R + 1, 2 ** 255, 2 ** 256 - 1], ids=["r", "r+1", "2^255", "2^256-1"])
def test_non_canonical_values_at_the_edges(kz, settings, value):
    base = random_blob(4242)
    for i in (0, 511, 512, 4095):
        bad = base[:32 * i] + value.to_bytes(32, "big") + base[32 * i + 32:]
        with pytest.raises(kz.BadArgs):
            kz.Kzg.compute_cells(bad, settings)
        with pytest.raises(kz.BadArgs):
            kz.Kzg.compute_kzg_cell_proofs(bad, settings)
        with pytest.raises(kz.BadArgs):
            kz.Kzg.compute_cells_and_kzg_proofs(bad, settings)


# ---- statuses across chunks
@pytest.fixture(scope="module")
def chunked(kz, settings):
    n, bad_at = 1030, (0, 511, 512, 1023, 1029)
    blobs = [random_blob(30000 + i) for i in range(n)]
    values = (R, R + 1, 2 ** 255, 2 ** 256 - 1, R)
    for b, v, e in zip(bad_at, values, (0, 4095, 511, 512, 2000)):
        blobs[b] = blobs[b][:32 * e] + v.to_bytes(32, "big") + blobs[b][32 * e + 32:]
    good = [i for i in range(n) if i not in bad_at]
    # the good blobs alone: a call whose chunks fall elsewhere
    lib = kz.kzg.lib()
    ref_c, ref_p = C.create_string_buffer(CELL_BYTES * len(good)), C.create_string_buffer(PROOF_BYTES * len(good))
    st = (C.c_int * len(good))()
    assert lib.kzg355_compute_cells_and_kzg_proofs_many(ref_c, ref_p, st, b"".join(blobs[i] for i in good), len(good), settings.handle) == 0
    assert list(st) == [0] * len(good)
    return n, bad_at, blobs, good, ref_c.raw, ref_p.raw


@pytest.mark.parametrize("form", ["cells", "proofs", "both"])
def test_statuses_land_on_their_blobs_across_chunks(kz, settings, chunked, form):
    n, bad_at, blobs, good, ref_c, ref_p = chunked
    lib = kz.kzg.lib()
    want_c, want_p = form in ("cells", "both"), form in ("proofs", "both")
    c_out = C.create_string_buffer(CELL_BYTES * n) if want_c else None
    p_out = C.create_string_buffer(PROOF_BYTES * n) if want_p else None
    st = (C.c_int * n)(*([7] * n))
    rc = lib.kzg355_compute_cells_and_kzg_proofs_many(c_out, p_out, st, b"".join(blobs), n, settings.handle)
    assert rc == BADARGS
    assert [i for i in range(n) if st[i] != 0] == list(bad_at)
    assert all(st[i] == BADARGS for i in bad_at)
    craw = c_out.raw if want_c else b""
    praw = p_out.raw if want_p else b""
    for j, i in enumerate(good):
        if want_c:
            assert craw[CELL_BYTES * i:CELL_BYTES * (i + 1)] == ref_c[CELL_BYTES * j:CELL_BYTES * (j + 1)], i
        if want_p:
            assert praw[PROOF_BYTES * i:PROOF_BYTES * (i + 1)] == ref_p[PROOF_BYTES * j:PROOF_BYTES * (j + 1)], i
    # single calls next to the bad blobs and the chunk edges; the CPU cells for six of them
    for i in (1, 510, 513, 1022, 1024, 1028):
        cells, proofs = kz.Kzg.compute_cells_and_kzg_proofs(blobs[i], settings)
        if want_c:
            assert craw[CELL_BYTES * i:CELL_BYTES * (i + 1)] == b"".join(raw(cells)), i
            if form == "cells":
                assert raw(cells) == cs.compute_cells(blobs[i]), i
        if want_p:
            assert praw[PROOF_BYTES * i:PROOF_BYTES * (i + 1)] == b"".join(raw(proofs)), i
    if form == "cells":                                          # cells-only single calls are cheap: every good blob
        for i in good:
            assert craw[CELL_BYTES * i:CELL_BYTES * (i + 1)] == b"".join(raw(kz.Kzg.compute_cells(blobs[i], settings))), i


# ---- the cell verifier on the special outputs
def test_cell_verifier_on_special_outputs(kz, settings, oracle, oracle_settings, mono):
    fx = json.load(open(os.path.join(HERE, "golden", "cells.json")))
    rng = random.Random(0x5eed)
    blobs = [bytes(cs.N_FE * 32),                                        # commitment and proofs at infinity
             blob_of_values([0x1234567] * cs.N_FE),                       # constant: proofs at infinity, commitment finite
             fk.blob_from_coefficients([rng.randrange(R) for _ in range(128)]),   # degree < 128: every proof H_0
             random_blob(fx["blob_seeds"][0])]
    coms = [oracle.blob_to_kzg_commitment(b, oracle_settings) for b in blobs]
    assert coms[0] == INF and coms[1] != INF
    out = [kz.Kzg.compute_cells_and_kzg_proofs(b, settings) for b in blobs]
    assert raw(out[0][1]) == raw(out[1][1]) == [INF] * 128
    assert len(set(raw(out[2][1]))) == 1
    assert raw(out[3][1]) == [bytes.fromhex(p) for p in fx["proofs"][0]]
    com = [coms[b] for b in range(4) for _ in range(128)]
    idx = [k for _ in range(4) for k in range(128)]
    cells = [bytes(c) for b in range(4) for c in out[b][0]]
    proofs = [bytes(p) for b in range(4) for p in out[b][1]]

    def both(cells, proofs):
        dev = kz.Kzg.verify_cell_kzg_proof_batch(com, idx, [kz.Cell(c) for c in cells], [kz.KzgProof(p) for p in proofs], settings)
        cpu = cs.verify_cell_kzg_proof_batch(oracle, com, idx, cells, proofs, mono=mono)
        return dev, cpu

    assert both(cells, proofs) == (True, True)
    bad_cells = list(cells)
    v = bytearray(bad_cells[5]); v[31] ^= 1; bad_cells[5] = bytes(v)          # a cell of the zero blob
    assert both(bad_cells, proofs) == (False, False)
    bad_proofs = list(proofs)
    bad_proofs[128 + 77] = mono[0]                                                # a proof of the constant blob: G1 in place of infinity
    assert both(cells, bad_proofs) == (False, False)
