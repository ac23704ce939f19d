"""Inputs shared by tests/test_gpu_blob_cell_shapes.py (GPU) and tests/test_blob_cell_shape_cases.py (CPU): groups of whole blobs for
verify_blob_cell_proofs_batch at the sizes where its own code takes another path, built from the CPU alone, and the CPU's 176 bytes
r | [I(tau)]_1 | LL | RL and verdict of each (nothing here calls the library under test).

Where the blobs come from:
  * mixtures: for scalars a = (a0, a1, a2) the blob a0 B0 + a1 B1 + a2 B2 (element-wise mod r) of the three fixture blobs; its cells are
    cell_spec.compute_cells of those bytes, its commitment sum a_b C_b and its proof of cell k sum a_b pi_{b,k} (the oracle's lincomb).  Pools.mix(t)
    is the t-th of a seeded sequence; check_claims finds out from the bytes that the commitments a group claims distinct are distinct.
  * low-degree blobs: fk20_spec.blob_from_coefficients of at most 128 coefficients with the commitment and the (one) proof of
    cell_batch_cases.lowdeg_item: degree < 64 a finite commitment with every proof at infinity, X^64 the generator as every proof, the zero blob
    with commitment and proofs at infinity.

A Group carries what it CLAIMS from its plan -- its kind (valid, spoiled, malformed), its number of distinct commitments and their order of first
appearance -- and observed() recomputes the last two from the bytes, as in cell_batch_cases.  Every spoiling asserts that it changed bytes.

The groups, each at the smallest size that crosses the boundary it is named after:
  * dedup positions (k_blob_meta takes slot j < ucount[g] of the deduplicated list, blob b reads pos[g n + b]): A,B,A,C; A,A,B,A,C; A,B,C,D,A; seven
    distinct blobs; and low-degree, zero, mixture, mixture (infinity as a commitment among finite ones)
  * 6 | 7 blobs per launch set (blob_interp_form: the column route up to 6 blobs, the coefficient route above): (n, groups) = (6, 1), (7, 1), (3, 2)
    at the boundary, (2, 4) and (1, 7) above it
  * 256-cell stride: k_cell_sum's 256-thread stride takes a second pass from 257 terms and a group of n blobs has 128 n cells, so n = 2 is the last
    size of one pass and n = 3 the first of two; the (2, 4) and (3, 2) groups above are those sizes
  * 128 | 129 distinct blobs in one group: 16384 cells (CELL_PREP_MAX_CELLS) is the last group the device hashes, 16512 the first the host must; and
    the 129 group with the proofs of cells 127 and 126 of its last blob exchanged
  * spoils at n = 7, all in the LAST blob so that an ignored tail shows: an element changed, the commitments of blobs 5 and 6 exchanged, two proofs
    exchanged (False); an element equal to r, an off-curve proof (BadArgs)

The CPU's answer: expected() is blob_cell_cases.expected, that is cell_spec.verify_cell_kzg_proof_batch over the 128 n cells, after the blobs' own
argument check (a field element >= r is BadArgs, as compute_cells has it).  For the 128- and 129-blob groups alone BigReference computes the same
176 bytes a shorter way (1.7 s a group where the spec's loop, 0.1 s a blob at seven blobs, would take some 13 s): r from cell_spec.challenge,
[I(tau)]_1 from blob_cell_cases.interpolant_from_coefficients over the blobs' coefficients (those of a mixture are the mixtures of the three
cell_spec.blob_coefficients; tests/test_blob_cell_spec.py holds the identity against the definition), LL and RL from cell_spec.lincomb over all
proofs with the spec's scalars, the verdict from the oracle's pairing check, every distinct point validated once.
tests/test_blob_cell_shape_cases.py holds BigReference against expected on small groups."""
import random

import blob_cell_cases as bcc
import cell_batch_cases as bc
import cell_device_cases as dcases
import cell_spec as cs
import fk20_spec as fk

R = cs.R
N = cs.CELLS_PER_EXT_BLOB
INF = bcc.INF
SEED = 0x7594C
BIG = 129                                                        # blobs of the largest group = mixtures a test module may ask the pool for


def fixture():
    """cell_batch_cases' fixture plus the fixture blobs as integers and their monomial coefficients"""
    fx = bc.fixture()
    fx["bvals"] = [blob_values(b) for b in fx["blobs"]]
    fx["coef"] = [cs.blob_coefficients(b) for b in fx["blobs"]]
    return fx


def blob_values(blob):
    """the 4096 field elements; BadArgs on one >= r (compute_cells' argument check)"""
    vals = [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(cs.N_FE)]
    if len(blob) != 32 * cs.N_FE or any(v >= R for v in vals):
        raise cs.BadArgs("non-canonical blob element")
    return vals


# ------------------------------------------------------------------------------------------------ whole blobs
class WholeBlob:
    """a blob with its 128 cells, its commitment and its 128 cell proofs; a: the mixture scalars (None for a low-degree blob)"""

    def __init__(self, tag, blob, cells, c, p, a=None):
        assert len(blob) == 32 * cs.N_FE and len(cells) == N and len(c) == 48 and len(p) == N
        self.tag, self.blob, self.cells, self.c, self.p, self.a = tag, blob, cells, c, p, a


def mixture_blob(o, fx, a, tag="mix"):
    v = fx["bvals"]
    blob = b"".join(((a[0] * v[0][i] + a[1] * v[1][i] + a[2] * v[2][i]) % R).to_bytes(32, "big") for i in range(cs.N_FE))
    return WholeBlob(tag, blob, cs.compute_cells(blob), cs.lincomb(o, fx["C"], a), [cs.lincomb(o, [fx["P"][b][k] for b in range(3)], a) for k in range(N)],
                     list(a))


def lowdeg_blob(o, fx, coeffs, tag="low"):
    """the blob of sum coeffs[t] X^t, at most 128 coefficients: one proof for every cell, by cell_batch_cases.lowdeg_item's rule"""
    blob = fk.blob_from_coefficients(coeffs)
    cells = cs.compute_cells(blob)
    c, _, cell5, proof = bc.lowdeg_item(o, fx, coeffs, 5)
    assert cell5 == cells[5], "Horner on the coset and the extension of the blob disagree"
    return WholeBlob(tag, blob, cells, c, [proof] * N)


class Pools:
    """the seeded blobs, each built on first use and kept (one instance per test module)"""

    def __init__(self, o, fx):
        self.o, self.fx, self._mix, self._low = o, fx, [], {}
        self._rng = random.Random(SEED)

    def mix(self, t):
        while len(self._mix) <= t:
            self._mix.append(mixture_blob(self.o, self.fx, [self._rng.randrange(1, R) for _ in range(3)], f"mix{len(self._mix)}"))
        return self._mix[t]

    def low(self, what):
        """"zero"; "deg63": degree 63, every proof at infinity; "x64": X^64, the generator as every proof; "deg127\""""
        if what not in self._low:
            rng = random.Random(SEED + 1)
            coeffs = {"zero": [0], "deg63": [rng.randrange(1, R) for _ in range(64)], "x64": [0] * 64 + [1],
                      "deg127": [rng.randrange(1, R) for _ in range(128)]}[what]
            wb = lowdeg_blob(self.o, self.fx, coeffs, what)
            if what == "zero":
                assert wb.blob == bytes(32 * cs.N_FE) and wb.c == INF and set(wb.p) == {INF}
            if what == "deg63":
                assert wb.c != INF and set(wb.p) == {INF}
            if what == "x64":
                assert set(wb.p) == {self.fx["mono"][0]} and wb.c == self.fx["mono"][64]
            self._low[what] = wb
        return self._low[what]


# ------------------------------------------------------------------------------------------------ groups
class Group:
    def __init__(self, name, wbs, kind, distinct, first):
        self.name, self.kind = name, kind
        self.blobs = [w.blob for w in wbs]
        self.cells = [list(w.cells) for w in wbs]                 # None for a blob that has no cells (an element >= r)
        self.c = [w.c for w in wbs]
        self.p = [x for w in wbs for x in w.p]
        self.a = [w.a for w in wbs]
        self.distinct, self.first = distinct, first               # the claims, from the builder's plan

    @property
    def n(self):
        return len(self.blobs)

    @property
    def args(self):
        """(blobs, commitments, cell_proofs) as verify_blob_cell_proofs_batch takes them"""
        return self.blobs, self.c, self.p

    def copy(self, name, kind):
        g = Group.__new__(Group)
        g.name, g.kind, g.distinct, g.first = name, kind, self.distinct, list(self.first)
        g.blobs, g.cells, g.c, g.p, g.a = list(self.blobs), [row if row is None else list(row) for row in self.cells], list(self.c), list(self.p), list(self.a)
        return g


def observed(g):
    """(distinct commitments, first-appearance order) from the group's bytes"""
    first = list(dict.fromkeys(g.c))
    return len(first), first


def check_claims(g):
    assert g.kind in ("valid", "spoiled", "malformed") and g.distinct is not None and g.first is not None, g.name
    assert len(g.c) == len(g.blobs) == len(g.cells) == g.n and len(g.p) == N * g.n, g.name
    assert all(len(x) == 48 for x in g.c + g.p) and all(len(b) == 32 * cs.N_FE for b in g.blobs), g.name
    d, first = observed(g)
    assert d == g.distinct, (g.name, d, g.distinct)
    assert first == g.first, g.name


def planned(name, blobs, plan, kind="valid"):
    """the group blobs[plan[0]], blobs[plan[1]], ...: the claims come from the plan; they hold if the commitments of `blobs` are pairwise distinct,
    which check_claims finds out from the bytes"""
    order = list(dict.fromkeys(plan))
    return Group(name, [blobs[t] for t in plan], kind, distinct=len(order), first=[blobs[t].c for t in order])


DEDUP = ("ABAC", "AABAC", "ABCDA", "seven", "kinds")


def dedup_group(pools, which):
    if which == "seven":
        return distinct_group(pools, 7)
    if which == "kinds":                                          # low-degree, zero (infinity as a commitment, in slot 1), two mixtures
        return planned("dedup-kinds", [pools.low("deg63"), pools.low("zero"), pools.mix(1), pools.mix(2)], [0, 1, 2, 3])
    plan = [ord(ch) - ord("A") for ch in which]
    return planned(f"dedup-{which}", [pools.mix(t) for t in range(4)], plan)


def distinct_group(pools, n, start=0):
    """n mixtures, every commitment distinct: pool blobs start .. start + n - 1"""
    g = planned(f"distinct{n}" + (f"@{start}" if start else ""), [pools.mix(start + t) for t in range(n)], list(range(n)))
    assert g.distinct == n
    return g


LAUNCH_SETS = ((6, 1), (7, 1), (3, 2), (2, 4), (1, 7))            # (blobs per group, groups): 6, 7, 6, 8 and 7 blobs in the launch set


def launch_set_groups(pools, n, groups):
    """`groups` groups of n blobs.  One group: all distinct.  Several: all distinct, a repeat, infinity and low-degree blobs among them, so that
    no two groups of a call are alike"""
    if groups == 1:
        return [distinct_group(pools, n)]
    if n == 3:
        return [distinct_group(pools, 3, 4), planned("three-ABA", [pools.mix(7), pools.mix(8)], [0, 1, 0])]
    if n == 2:
        return [distinct_group(pools, 2, 9), planned("two-AA", [pools.mix(11)], [0, 0]), planned("two-x64-mix", [pools.low("x64"), pools.mix(12)], [0, 1]),
                planned("two-mix-zero", [pools.mix(13), pools.low("zero")], [0, 1])]
    assert n == 1 and groups == 7
    return ([distinct_group(pools, 1, 14 + t) for t in range(3)] +
            [planned(f"one-{what}", [pools.low(what)], [0]) for what in ("zero", "deg63", "x64", "deg127")])


def big_group(pools, n):
    assert n in (BIG - 1, BIG)
    return distinct_group(pools, n)


# ---- spoilings: each returns a new group and asserts that bytes changed
def _changed(g, out):
    assert out.args != g.args, "a spoiling that changes nothing"
    return out


def spoil_element(g, b, i):
    """element i of blob b plus one: the blob is no longer the one committed to; False"""
    out = g.copy(f"{g.name}-element{b}.{i}", "spoiled")
    v = int.from_bytes(g.blobs[b][32 * i:32 * i + 32], "big")
    out.blobs[b] = g.blobs[b][:32 * i] + ((v + 1) % R).to_bytes(32, "big") + g.blobs[b][32 * i + 32:]
    out.cells[b] = cs.compute_cells(out.blobs[b])
    out.a[b] = None
    assert out.cells[b] != g.cells[b]
    return _changed(g, out)


def spoil_swap_commitments(g, b1, b2):
    """the commitments of blobs b1 and b2 exchanged (each appears once): False, and the order of first appearance changes with them"""
    assert g.c[b1] != g.c[b2] and g.c.count(g.c[b1]) == 1 and g.c.count(g.c[b2]) == 1
    out = g.copy(f"{g.name}-commitments{b1}x{b2}", "spoiled")
    out.c[b1], out.c[b2] = g.c[b2], g.c[b1]
    i1, i2 = g.first.index(g.c[b1]), g.first.index(g.c[b2])
    out.first[i1], out.first[i2] = g.first[i2], g.first[i1]
    return _changed(g, out)


def spoil_swap_proofs(g, b, k1, k2):
    """the proofs of cells k1 and k2 of blob b exchanged: False"""
    j1, j2 = N * b + k1, N * b + k2
    assert g.p[j1] != g.p[j2], "a spoiling that changes nothing"
    out = g.copy(f"{g.name}-proofs{b}.{k1}x{k2}", "spoiled")
    out.p[j1], out.p[j2] = g.p[j2], g.p[j1]
    return _changed(g, out)


def malformed_element(g, b, i):
    """element i of blob b equal to r: BadArgs; the blob has no cells"""
    out = g.copy(f"{g.name}-element{b}.{i}=r", "malformed")
    out.blobs[b] = g.blobs[b][:32 * i] + R.to_bytes(32, "big") + g.blobs[b][32 * i + 32:]
    out.cells[b], out.a[b] = None, None
    return _changed(g, out)


def malformed_proof(g, b, k, point):
    """`point` (off the curve) as the proof of cell k of blob b: BadArgs"""
    out = g.copy(f"{g.name}-proof{b}.{k}-off-curve", "malformed")
    out.p[N * b + k] = point
    return _changed(g, out)


SPOILS7 = ("element", "commitments", "proofs", "element=r", "off-curve proof")


def spoils_at_seven(pools):
    """{what: group}: the all-distinct group of seven with its LAST blob spoiled"""
    g = distinct_group(pools, 7)
    out = {"element": spoil_element(g, 6, 4095), "commitments": spoil_swap_commitments(g, 5, 6), "proofs": spoil_swap_proofs(g, 6, 127, 3),
           "element=r": malformed_element(g, 6, 2077), "off-curve proof": malformed_proof(g, 6, 127, dcases.off_curve(pools.o))}
    assert tuple(out) == SPOILS7
    for what, s in out.items():                                   # the spoil sits in the last blob and nowhere else
        assert s.blobs[:6] == g.blobs[:6] and s.p[:N * 6] == g.p[:N * 6] and s.c[:5] == g.c[:5], what
    return out


def big_swapped(pools):
    """the 129 group with the proofs of cells 127 and 126 of blob 128 (the last) exchanged"""
    return spoil_swap_proofs(big_group(pools, BIG), BIG - 1, 127, 126)


def small_groups(pools):
    """every group of this module but the 128- and 129-blob ones, once each"""
    out = [dedup_group(pools, which) for which in DEDUP]
    for n, groups in LAUNCH_SETS:
        out += [g for g in launch_set_groups(pools, n, groups) if g.name not in {x.name for x in out}]
    out += list(spoils_at_seven(pools).values())
    assert len({g.name for g in out}) == len(out)
    return out


# ------------------------------------------------------------------------------------------------ the CPU's answer
def expected(o, fx, g):
    """(176 bytes, verdict) by the spec over the group's 128 n cells; cell_spec.BadArgs as the spec, or compute_cells before it, raises it"""
    for blob in g.blobs:
        blob_values(blob)
    return bcc.expected(o, g.cells, g.c, g.p, mono=fx["mono"], g2=fx["g2"])


class BigReference:
    """(176 bytes, verdict) of a group of mixtures, the way the module docstring says; a point is validated once however often and in however many
    groups it appears"""

    def __init__(self, o, fx):
        self.o, self.fx, self._valid, self._coef = o, fx, {}, {}

    def _coefficients(self, a):
        key = tuple(a)
        if key not in self._coef:
            f = self.fx["coef"]
            self._coef[key] = [(a[0] * f[0][i] + a[1] * f[1][i] + a[2] * f[2][i]) % R for i in range(cs.N_FE)]
        return self._coef[key]

    def __call__(self, g):
        assert all(a is not None for a in g.a), "mixtures only"
        for blob in g.blobs:
            blob_values(blob)
        for pt in dict.fromkeys(g.c + g.p):
            if pt not in self._valid:
                self._valid[pt] = self.o.g1_validate(pt) == 0
            if not self._valid[pt]:
                raise cs.BadArgs("validate_kzg_g1")
        args = bcc.group_args(g.cells, g.c, g.p)
        r, uniq, pos = cs.challenge(*args)
        n = N * g.n
        rp = [1] * n
        for k in range(1, n):
            rp[k] = rp[k - 1] * r % R
        I = bcc.interpolant_from_coefficients(r, [self._coefficients(a) for a in g.a])
        mono = self.fx["mono"][:cs.CELL_FE]
        itau = cs.lincomb(self.o, mono, I)
        ll = cs.lincomb(self.o, g.p, rp)
        w = [0] * len(uniq)
        for k in range(n):
            w[pos[k]] = (w[pos[k]] + rp[k]) % R
        h64 = [pow(cs.coset_shift(k), cs.CELL_FE, R) for k in range(N)]
        rl = cs.lincomb(self.o, uniq + mono + g.p, w + [(-x) % R for x in I] + [rp[k] * h64[k % N] % R for k in range(n)])
        return cs._be(r) + itau + ll + rl, self.o.pairings_verify(ll, self.fx["g2"][cs.CELL_FE], rl, self.fx["g2"][0])
