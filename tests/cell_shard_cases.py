"""Inputs shared by tests/test_cell_shard_spec.py (CPU) and tests/test_gpu_cell_multi_device.py (GPU): verify_cell_kzg_proof_batch groups that a
handle over D devices cuts into D contiguous blocks of cells (block d = cells [n d / D, n (d + 1) / D)), and the CPU statement of what each block
contributes to the check.

A cut group must have, for the cut to be able to go wrong: a commitment that appears in two blocks (each block deduplicates on its own, so the
commitment is weighted in both), a column that appears in two blocks (one segment of the interpolant in each) and a block whose cells are not in
column order (each block sorts on its own).  cut_group() builds such groups from mixtures of the fixture blobs (cell_batch_cases.mixture_item) and
check_cut() asserts that the three properties hold, from the bytes."""
import random
from collections import Counter

import cell_batch_cases as bc
import cell_spec as cs

R = cs.R
SEED = 0x7594E


def blocks_of(n, D):
    """[(first cell, cells)] of the D blocks of a group of n cells"""
    return [(n * d // D, n * (d + 1) // D - n * d // D) for d in range(D)]


# (blob, column) per cell; blobs 0..2 are three fixed mixtures of the fixture blobs
PLANS = {
    7: [(0, 9), (1, 5), (0, 3), (2, 9), (1, 100), (2, 2), (0, 64)],      # blocks (2, 2, 3)
    6: [(0, 70), (1, 3), (1, 70), (2, 1), (2, 5), (0, 6)],               # blocks (2, 2, 2)
    8: [(0, 127), (1, 0), (2, 127), (0, 1), (1, 64), (1, 63), (2, 0), (0, 127)],     # blocks (2, 3, 3)
    3: [(0, 9), (1, 50), (0, 9)],                                         # two devices: blocks (1, 2)
}


def cut_group(o, fx, n, variant=0):
    """the group of PLANS[n] as a cell_batch_cases.Group; variant picks other mixtures (a second group of the same shape)"""
    rng = random.Random(SEED + 16 * variant)
    blobs = [[rng.randrange(1, R) for _ in range(3)] for _ in range(3)]
    made = {}
    items = []
    for b, k in PLANS[n]:
        if (b, k) not in made:
            made[b, k] = bc.mixture_item(o, fx, blobs[b], k)
        items.append(made[b, k])
    first = list(dict.fromkeys(x[0] for x in items))
    return bc.Group(f"cut{n}v{variant}", items, "valid", distinct=len(first), first=first, columns=dict(Counter(x[1] for x in items)))


def check_cut(g, D):
    """the three properties of the module docstring, from the group's bytes"""
    bl = blocks_of(g.n, D)
    where_c, where_k = {}, {}
    for d, (off, cnt) in enumerate(bl):
        for t in range(off, off + cnt):
            where_c.setdefault(g.c[t], set()).add(d)
            where_k.setdefault(int(g.i[t]), set()).add(d)
    assert any(len(v) > 1 for v in where_c.values()), f"{g.name}: no commitment in two blocks"
    assert any(len(v) > 1 for v in where_k.values()), f"{g.name}: no column in two blocks"
    assert any(list(g.i[off:off + cnt]) != sorted(g.i[off:off + cnt]) for off, cnt in bl), f"{g.name}: every block is in column order"


def block_sums(o, mono, r, off, commitments, cell_indices, cells, proofs):
    """([I_d(tau)]_1, LL_d, RL_d) of one block: the group's r, exponents from `off`, the block's own dedup and column sums -- what one device
    computes.  Linear in the cells: the blocks' sums add up to the group's."""
    n = len(commitments)
    rp = [pow(r, off + k, R) for k in range(n)]
    uniq, pos = [], []
    for c in commitments:
        if c not in uniq:
            uniq.append(c)
        pos.append(uniq.index(c))
    w = [0] * len(uniq)
    for k in range(n):
        w[pos[k]] = (w[pos[k]] + rp[k]) % R
    cols = {}
    for k in sorted(range(n), key=lambda t: int(cell_indices[t])):       # the block's own column sort (stable)
        acc = cols.setdefault(int(cell_indices[k]), [0] * cs.CELL_FE)
        for j, v in enumerate(cs.cell_values(cells[k])):
            acc[j] = (acc[j] + rp[k] * v) % R
    I = [0] * cs.CELL_FE
    for c, acc in cols.items():
        for t, v in enumerate(cs.cell_interpolant(acc, c)):
            I[t] = (I[t] + v) % R
    itau = cs.lincomb(o, mono[:cs.CELL_FE], I)
    ll = cs.lincomb(o, list(proofs), rp)
    rl = cs.lincomb(o, uniq + list(mono[:cs.CELL_FE]) + list(proofs),
                    w + [(-x) % R for x in I] + [rp[k] * pow(cs.coset_shift(int(cell_indices[k])), cs.CELL_FE, R) % R for k in range(n)])
    return itau, ll, rl


def add_points(o, pts):
    return cs.lincomb(o, list(pts), [1] * len(pts))


def swap_proofs(g, a, b):
    """g with the proofs of cells a and b exchanged (they must differ): well-formed, False"""
    items = g.items()
    assert items[a][3] != items[b][3], "a spoiling that changes nothing"
    pa, pb = items[a][3], items[b][3]
    items[a] = items[a][:3] + (pb,)
    items[b] = items[b][:3] + (pa,)
    return bc.Group(f"{g.name}-swap{a}-{b}", items, "spoiled", distinct=g.distinct, first=g.first, columns=g.columns)


def with_item(g, j, kind, commitment=None, index=None, cell=None, proof=None):
    """g with parts of item j replaced"""
    items = g.items()
    c, i, cl, p = items[j]
    items[j] = (commitment or c, i if index is None else index, cell or cl, proof or p)
    assert items[j] != (c, i, cl, p), "a spoiling that changes nothing"
    return bc.Group(f"{g.name}-{kind}{j}", items, kind, distinct=g.distinct, first=g.first, columns=g.columns)


def noncanonical(cell, j=17):
    """the cell with element j replaced by r (the smallest non-canonical value)"""
    return cell[:32 * j] + R.to_bytes(32, "big") + cell[32 * j + 32:]
