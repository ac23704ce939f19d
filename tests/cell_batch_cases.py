"""Inputs shared by tests/test_gpu_cell_batch_shapes.py (GPU) and tests/test_cell_batch_cases.py (CPU): verify_cell_kzg_proof_batch groups at the shapes
of a PeerDAS column sidecar (one cell index, one distinct commitment per cell) and of a block taken as one batch (up to 128 x 128 cells), built from
the CPU alone, and the CPU function that says what r, [I(tau)]_1, LL, RL and the verdict of such a group are.

Where the items come from (nothing here calls the library under test):
  * mixtures: for scalars a = (a0, a1, a2) the blob a0 B0 + a1 B1 + a2 B2 of the three fixture blobs has commitment sum a_b C_b, cell k equal to
    sum a_b cells_b[k] element-wise mod r and proof sum a_b pi_{b,k}; lam times a valid item is a valid item again (scaled()).
  * low-degree blobs: a polynomial p of degree < 128 has commitment sum_{t<128} p_t [tau^t]_1, the same proof sum_{t<64} p_{t+64} [tau^t]_1 for every
    cell and cells by Horner at h_k w64^rev6(j).  The zero polynomial: commitment, proof, LL, RL and [I(tau)]_1 all at infinity; degree < 64: a
    finite commitment with proof, LL and RL at infinity; X^64: the generator as every proof.
  * setup points: the 4096 Lagrange and 4096 monomial points of the trusted setup are 8192 distinct valid G1 points; as "commitments" over fixture
    cells and proofs they give well-formed groups with any number of distinct commitments whose verdict is False.

Every builder returns a Group that carries what it CLAIMS from its construction plan (kind, number of distinct commitments, first-appearance order,
cells per column); observed() recomputes the same from the bytes, and both test modules assert that the two agree, so that a builder cannot silently
drop or collapse what a test is named after.  spoil() asserts that it changed bytes: a no-op mutation is an error of the test, not a group that
"may still verify"."""
import hashlib
import os
import random
from collections import Counter

import cell_spec as cs
import cell_device_cases as dcases

R = cs.R
INF = b"\xc0" + bytes(47)
SEED = 0x7594B
POOL = 300            # mixture items of the common pool: more than the largest all-distinct mixture group (257)
GOLDEN = cs.GOLDEN


# ------------------------------------------------------------------------------------------------ fixture and items
def fixture():
    """cell_device_cases' fixture plus the cells as integers, 128 monomial points and the G2 points"""
    fx = dcases.fixture()
    fx["vals"] = [[cs.cell_values(c) for c in row] for row in fx["cells"]]
    fx["mono"] = cs.load_monomial(128)
    fx["g2"] = cs.g2_points()
    return fx


def setup_points():
    """the 8192 distinct valid G1 points of the two committed setup files, Lagrange and monomial interleaved"""
    lag = open(os.path.join(GOLDEN, "trusted_setup_g1.bin"), "rb").read()
    mono = open(os.path.join(GOLDEN, "setup_g1_monomial.bin"), "rb").read()
    out = []
    for t in range(4096):
        out += [lag[48 * t:48 * t + 48], mono[48 * t:48 * t + 48]]
    return out


def _cell_bytes(vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def mixture_item(o, fx, a, k):
    """(commitment, cell index, cell, proof) of the blob a0 B0 + a1 B1 + a2 B2 at cell k"""
    v = fx["vals"]
    cell = _cell_bytes([(a[0] * v[0][k][j] + a[1] * v[1][k][j] + a[2] * v[2][k][j]) % R for j in range(cs.CELL_FE)])
    return cs.lincomb(o, fx["C"], a), k, cell, cs.lincomb(o, [fx["P"][b][k] for b in range(3)], a)


def mixture_pool(o, fx, indices, seed):
    rng = random.Random(seed)
    return [mixture_item(o, fx, [rng.randrange(1, R) for _ in range(3)], k) for k in indices]


def scaled(o, item, lam):
    """lam times a valid item: the item of lam times its blob"""
    c, k, cell, p = item
    lam_be = cs._be(lam)
    return o.g1_mul_add(c, lam_be), k, _cell_bytes([lam * x % R for x in cs.cell_values(cell)]), o.g1_mul_add(p, lam_be)


def poly_cell(coeffs, k):
    h = cs.coset_shift(k)
    out = []
    for j in range(cs.CELL_FE):
        x = h * pow(cs.W64, cs.rev(j, 6), R) % R
        y = 0
        for c in reversed(coeffs):
            y = (y * x + c) % R
        out.append(y)
    return _cell_bytes(out)


def lowdeg_item(o, fx, coeffs, k):
    """the item of the polynomial sum coeffs[t] X^t (at most 128 coefficients) at cell k"""
    coeffs = list(coeffs)
    assert len(coeffs) <= 128

    def commit(cf):                                              # over the non-zero coefficients only; none: the point at infinity
        nz = [(fx["mono"][t], c) for t, c in enumerate(cf) if c]
        return cs.lincomb(o, [p for p, _ in nz], [c for _, c in nz]) if nz else INF
    return commit(coeffs), k, poly_cell(coeffs, k), commit(coeffs[64:])


def column_plan(n):
    """cell indices of a group that holds all 128 columns from 128 cells on: a shuffle of 0..127 first, the rest drawn from eight columns only, so
    that from 129 cells on the counts are uneven (at exactly 128 every column holds one cell: there is no other way to fill 128 columns)"""
    rng = random.Random(SEED + 1)
    first = list(range(128)); rng.shuffle(first)
    return (first + [rng.choice((0, 1, 5, 64, 77, 126, 127, 127)) for _ in range(max(0, n - 128))])[:n]


class Pools:
    """the seeded item pools, each built on first use and kept (one instance per test module)"""

    def __init__(self, o, fx):
        self.o, self.fx, self._made = o, fx, {}

    def _get(self, name, make):
        if name not in self._made:
            self._made[name] = make()
        return self._made[name]

    @property
    def mixed(self):          # POOL items, a random cell index each
        rng = random.Random(SEED + 2)
        return self._get("mixed", lambda: mixture_pool(self.o, self.fx, [rng.randrange(128) for _ in range(POOL)], SEED + 3))

    @property
    def sidecar(self):        # 257 items of one cell index
        return self._get("sidecar", lambda: mixture_pool(self.o, self.fx, [93] * 257, SEED + 4))

    @property
    def columns(self):        # 257 items on column_plan's indices
        return self._get("columns", lambda: mixture_pool(self.o, self.fx, column_plan(257), SEED + 5))

    @property
    def spare(self):          # donors of a spoiling: their commitments and proofs appear in no group
        return self._get("spare", lambda: mixture_pool(self.o, self.fx, [7, 8], SEED + 6))

    def many(self, count):
        """count valid items with pairwise distinct commitments: the mixed pool, then its multiples by 2, 3, ..."""
        have = self._made.setdefault("many", list(self.mixed))
        while len(have) < count:
            t = len(have)
            have.append(scaled(self.o, self.mixed[t % POOL], t // POOL + 1))
        return have[:count]

    @property
    def setup(self):
        return self._get("setup", setup_points)


# ------------------------------------------------------------------------------------------------ groups
class Group:
    def __init__(self, name, items, kind, distinct=None, first=None, columns=None):
        self.name, self.kind = name, kind
        self.c = [x[0] for x in items]
        self.i = [x[1] for x in items]
        self.cells = [x[2] for x in items]
        self.p = [x[3] for x in items]
        # the claims, from the builder's plan: None = "as the items say" is never allowed
        self.distinct, self.first, self.columns = distinct, first, columns

    @property
    def n(self):
        return len(self.c)

    @property
    def args(self):
        return self.c, self.i, self.cells, self.p

    def items(self):
        return list(zip(self.c, self.i, self.cells, self.p))


def observed(g):
    """(distinct commitments, first-appearance order, cells per column) from the group's bytes"""
    first = list(dict.fromkeys(g.c))
    return len(first), first, dict(Counter(int(i) for i in g.i))


def check_claims(g):
    assert g.distinct is not None and g.first is not None and g.columns is not None, g.name
    d, first, cols = observed(g)
    assert len(g.c) == len(g.i) == len(g.cells) == len(g.p), g.name
    assert all(len(x) == 48 for x in g.c + g.p) and all(len(x) == cs.BYTES_PER_CELL for x in g.cells), g.name
    assert d == g.distinct, (g.name, d, g.distinct)
    assert first == g.first, g.name
    assert cols == {k: v for k, v in g.columns.items() if v}, g.name


def planned(name, pool, plan, kind="valid"):
    """the group pool[plan[0]], pool[plan[1]], ...: the claims come from the plan (they hold if the pool's commitments are pairwise distinct, which
    check_claims then finds out from the bytes)"""
    order = list(dict.fromkeys(plan))
    return Group(name, [pool[t] for t in plan], kind, distinct=len(order), first=[pool[t][0] for t in order],
                 columns=dict(Counter(pool[t][1] for t in plan)))


def distinct_group(pools, n, layout):
    """n mixture items, every commitment distinct.  layout "mixed": a random cell index each; "sidecar": one cell index, so one segment holds all
    the cells; "columns": all 128 columns (column_plan)"""
    pool = {"mixed": pools.mixed, "sidecar": pools.sidecar, "columns": pools.columns}[layout]
    g = planned(f"{layout}{n}", pool, list(range(n)))
    if layout == "sidecar":
        assert g.columns == {93: n}
    if layout == "columns":
        assert g.columns == dict(Counter(column_plan(n))) and (n < 128 or len(g.columns) == 128)
    return g


SPOILINGS = ("cell", "proof", "index", "commitment")


def spoil(g, what, j, donor=None):
    """g with item j changed in one part; donor: the item whose proof / commitment replaces item j's.  The changed bytes must differ."""
    c, i, cells, p = [list(x) for x in g.args]
    columns, first = dict(g.columns), list(g.first)
    if what == "cell":
        v = cs.cell_values(cells[j])
        v[41] = (v[41] + 1) % R
        new = _cell_bytes(v)
        assert new != cells[j]
        cells[j] = new
    elif what == "proof":
        assert donor[3] != p[j], "a spoiling that changes nothing"
        p[j] = donor[3]
    elif what == "index":
        new = (i[j] + 1) % 128
        assert new != i[j]
        columns[i[j]] -= 1
        columns[new] = columns.get(new, 0) + 1
        i[j] = new
    elif what == "commitment":
        assert donor[0] != c[j], "a spoiling that changes nothing"
        assert c.count(c[j]) == 1 and donor[0] not in c, "the claim below holds for a commitment that appears once, replaced by a new one"
        first[first.index(c[j])] = donor[0]
        c[j] = donor[0]
    else:
        raise ValueError(what)
    out = Group(f"{g.name}-{what}{j}", list(zip(c, i, cells, p)), "spoiled", distinct=g.distinct, first=first, columns=columns)
    assert out.args != g.args, "a spoiling that changes nothing"
    return out


def malformed_index(g, j):
    """g with cell index 128 at item j: BadArgs (the claims speak of the indices below 128)"""
    items = g.items()
    columns = dict(g.columns)
    columns[items[j][1]] -= 1
    columns[128] = 1
    items[j] = (items[j][0], 128, items[j][2], items[j][3])
    return Group(f"{g.name}-malformed{j}", items, "malformed", distinct=g.distinct, first=g.first, columns=columns)


DEDUP_ORDERS = ("one", "two", "half", "descending")


def dedup_group(pools, n, order):
    """n cells that repeat valid items (a repeated item is the same valid cell again, so the group is valid):
      one         one commitment throughout (u = 1)
      two         two commitments alternating
      half        u = n // 2 as A B C ... then all of them again, rotated by 100: every second appearance is far from the first, in another pass of
                  the table insert's 256-thread stride and in another wave; the odd cell out repeats A a third time
      descending  300 commitments whose first appearances descend in bytes, repeated to n"""
    if order == "one":
        pool, plan = pools.mixed, [11] * n
    elif order == "two":
        pool, plan = pools.mixed, [(17, 4)[t & 1] for t in range(n)]
    elif order == "half":
        u = n // 2
        pool = pools.many(u)
        plan = list(range(u)) + [(t + 100) % u for t in range(u)] + [0] * (n - 2 * u)
    elif order == "descending":
        pool = sorted(pools.mixed, key=lambda x: x[0], reverse=True)
        plan = [t % POOL for t in range(n)]
    else:
        raise ValueError(order)
    g = planned(f"dedup-{order}{n}", pool, plan)
    want_u = {"one": 1, "two": min(2, n), "half": n // 2, "descending": min(n, POOL)}[order]
    assert g.distinct == want_u
    return g


def setup_group(pools, n, every=1):
    """n fixture cells and proofs under setup points as commitments: well-formed, False.  every = 1: all commitments distinct; every = 2: every
    second cell brings a new commitment and the others repeat an earlier one (when the 8192 points run out, all further cells repeat)"""
    fx, pts = pools.fx, pools.setup
    rng = random.Random(SEED + 7 + n)
    items, plan = [], []
    new = 0
    for t in range(n):
        if t % every == 0 and new < len(pts):
            plan.append(new); new += 1
        else:
            plan.append(rng.randrange(new))
        b, k = rng.randrange(3), rng.randrange(128)
        items.append((pts[plan[-1]], k, fx["cells"][b][k], fx["P"][b][k]))
    order = list(dict.fromkeys(plan))
    assert order == list(range(new)) and new == min(len(pts), (n + every - 1) // every)
    return Group(f"setup{n}/{every}", items, "spoiled", distinct=new, first=[pts[t] for t in order], columns=dict(Counter(x[1] for x in items)))


def _lowdeg_group(name, pools, polys, kind):
    """one item per polynomial, cell indices from a shuffle of 0..127 repeated; the claims from the polynomials (two polynomials have the same
    commitment exactly when they are equal)"""
    rng = random.Random(SEED + 8)
    ks = list(range(128)); rng.shuffle(ks)
    items = [lowdeg_item(pools.o, pools.fx, p, ks[t % 128]) for t, p in enumerate(polys)]
    order = list(dict.fromkeys(tuple(p) for p in polys))
    first = [items[[tuple(p) for p in polys].index(q)][0] for q in order]
    return Group(name, items, kind, distinct=len(order), first=first, columns=dict(Counter(x[1] for x in items)))


def zero_group(pools, n):
    """only zero-polynomial items: every commitment, proof and sum is the point at infinity; True"""
    g = _lowdeg_group(f"zero{n}", pools, [[0]] * n, "valid")
    assert set(g.c) == {INF} and set(g.p) == {INF} and set(g.cells) == {bytes(cs.BYTES_PER_CELL)}
    return g


def constlin_group(pools, n):
    """only constant and linear polynomials, all different: finite commitments, every proof (so LL and RL) at infinity, [I(tau)]_1 finite; True"""
    rng = random.Random(SEED + 9)
    polys = [[rng.randrange(1, R)] if t % 2 == 0 else [rng.randrange(R), rng.randrange(1, R)] for t in range(n)]
    g = _lowdeg_group(f"constlin{n}", pools, polys, "valid")
    assert set(g.p) == {INF} and INF not in g.c
    return g


def mixed_group(pools, n=129):
    """zero, constant, a X^64, degree-127 and mixture items side by side, every commitment distinct (infinity among them, once)"""
    rng = random.Random(SEED + 10)
    polys = [[0]] + [[rng.randrange(1, R)] for _ in range(20)] + [[0] * 64 + [1]] + [[0] * 64 + [rng.randrange(2, R)] for _ in range(19)]
    polys += [[rng.randrange(R) for _ in range(127)] + [rng.randrange(1, R)] for _ in range(20)]
    low = _lowdeg_group("low", pools, polys, "valid")
    assert low.p[21] == pools.fx["mono"][0], "X^64: the generator as proof"
    mix = pools.mixed[:n - low.n]
    items = []
    lo, mi = low.items(), list(mix)
    while lo or mi:                                              # interleaved, so that infinity is neither first nor last
        if mi:
            items.append(mi.pop())
        if lo:
            items.append(lo.pop())
    assert len(items) == n
    return Group(f"kinds{n}", items, "valid", distinct=n, first=[x[0] for x in items], columns=dict(Counter(x[1] for x in items)))


# ------------------------------------------------------------------------------------------------ the CPU's answer
def challenge(commitments, cell_indices, cells, proofs):
    """cell_spec.challenge with a dictionary where that searches a list (quadratic in the number of distinct commitments)"""
    where, pos = {}, []
    for c in commitments:
        pos.append(where.setdefault(c, len(where)))
    uniq = list(where)
    n = len(commitments)
    parts = [cs.DOMAIN, cs.N_FE.to_bytes(8, "big"), cs.CELL_FE.to_bytes(8, "big"), len(uniq).to_bytes(8, "big"), n.to_bytes(8, "big")] + uniq
    for k in range(n):
        parts += [pos[k].to_bytes(8, "big"), int(cell_indices[k]).to_bytes(8, "big"), bytes(cells[k]), bytes(proofs[k])]
    return int.from_bytes(hashlib.sha256(b"".join(parts)).digest(), "big") % R, uniq, pos


class Reference:
    """verify_cell_kzg_proof_batch on the CPU, the mathematics of cell_spec.verify_cell_kzg_proof_batch: the same argument checks, transcript,
    weights, interpolant and sums.  What differs is bookkeeping that cannot change a result: a point is validated once however often it appears
    (and once per Reference, not per group), cells are parsed once, and the scalars of equal points -- and the weights of equal cells in one
    column -- are added up before the lincomb / the interpolation (both are linear)."""

    def __init__(self, o, fx):
        self.o, self.mono, self.g2 = o, fx["mono"][:cs.CELL_FE], fx["g2"]
        self._valid, self._vals = {}, {}

    def _validate(self, b):
        if b not in self._valid:
            self._valid[b] = self.o.g1_validate(b) == 0
        return self._valid[b]

    def _cell(self, cell):
        if cell not in self._vals:
            try:
                self._vals[cell] = cs.cell_values(cell)
            except cs.BadArgs:
                self._vals[cell] = None
        return self._vals[cell]

    def _lincomb(self, pairs):
        acc = {}
        for pt, s in pairs:
            acc[pt] = (acc.get(pt, 0) + s) % R
        return cs.lincomb(self.o, list(acc), list(acc.values()))

    def __call__(self, commitments, cell_indices, cells, proofs, sums=True):
        """(r as 32 big-endian bytes, [I(tau)]_1, LL, RL, verdict); sums=False stops after [I(tau)]_1 (None for the rest) and leaves the points
        unvalidated: the caller then asks the library's status whether they were well-formed.  BadArgs as cell_spec raises it."""
        n = len(commitments)
        assert n > 0 and len(cell_indices) == len(cells) == len(proofs) == n
        if any(int(i) >= cs.CELLS_PER_EXT_BLOB for i in cell_indices):
            raise cs.BadArgs("cell index")
        if sums and not all(self._validate(b) for b in dict.fromkeys(list(commitments) + list(proofs))):
            raise cs.BadArgs("validate_kzg_g1")
        if any(self._cell(c) is None for c in dict.fromkeys(cells)):
            raise cs.BadArgs("non-canonical cell element")
        r, uniq, pos = challenge(commitments, cell_indices, cells, proofs)
        rp = [1] * n
        for k in range(1, n):
            rp[k] = rp[k - 1] * r % R
        weight = {}                                               # (column, cell) -> sum of r^k
        for k in range(n):
            key = (int(cell_indices[k]), cells[k])
            weight[key] = (weight.get(key, 0) + rp[k]) % R
        cols = {}
        for (c, cell), wt in weight.items():
            acc, v = cols.setdefault(c, [0] * cs.CELL_FE), self._vals[cell]
            for j in range(cs.CELL_FE):
                acc[j] = (acc[j] + wt * v[j]) % R
        I = [0] * cs.CELL_FE
        for c, acc in cols.items():
            for t, v in enumerate(cs.cell_interpolant(acc, c)):
                I[t] = (I[t] + v) % R
        itau = cs.lincomb(self.o, self.mono, I)
        if not sums:
            return cs._be(r), itau, None, None, None
        ll = self._lincomb(zip(proofs, rp))
        h64 = {c: pow(cs.coset_shift(c), cs.CELL_FE, R) for c in cols}
        rl = self._lincomb([(commitments[k], rp[k]) for k in range(n)] + [(self.mono[t], -I[t]) for t in range(cs.CELL_FE)] +
                           [(proofs[k], rp[k] * h64[int(cell_indices[k])]) for k in range(n)])
        return cs._be(r), itau, ll, rl, self.o.pairings_verify(ll, self.g2[cs.CELL_FE], rl, self.g2[0])
