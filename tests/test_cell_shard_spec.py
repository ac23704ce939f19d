"""CPU only: the linearity that lets a handle over several devices cut one verify_cell_kzg_proof_batch group into blocks of cells (DESIGN.md
section 11), pinned against tests/cell_spec.py in Python integers.  Once r is known -- from the transcript of the WHOLE group -- LL, RL and
[I(tau)]_1 are sums over the cells, so block d, with exponents starting at its first cell's position and its own dedup and column sums
(cell_shard_cases.block_sums), yields three points, and the blocks' points add up to the group's.  The shapes are the smallest ragged and equal
cuts over three devices; each group has a commitment in two blocks, a column in two blocks and a block out of column order."""
import pytest

import cell_batch_cases as bc
import cell_shard_cases as sc
import cell_spec as cs


@pytest.fixture(scope="module")
def fx():
    return bc.fixture()


def summed(oracle, fx, g, D):
    r, _, _ = cs.challenge(*g.args)
    per_block = [sc.block_sums(oracle, fx["mono"], r, off, g.c[off:off + cnt], g.i[off:off + cnt], g.cells[off:off + cnt], g.p[off:off + cnt])
                 for off, cnt in sc.blocks_of(g.n, D)]
    return [sc.add_points(oracle, [b[side] for b in per_block]) for side in range(3)], per_block


@pytest.mark.parametrize("n, blocks", [(7, [2, 2, 3]), (6, [2, 2, 2])])
def test_block_sums_add_up_to_the_groups(oracle, fx, n, blocks):
    D = 3
    assert [cnt for _, cnt in sc.blocks_of(n, D)] == blocks
    g = sc.cut_group(oracle, fx, n)
    bc.check_claims(g)
    sc.check_cut(g, D)
    for grp, verdict in ((g, True), (sc.swap_proofs(g, 0, n - 1), False)):        # the swap crosses the first and the last block
        ok, d = cs.verify_cell_kzg_proof_batch(oracle, *grp.args, mono=fx["mono"][:64], g2=fx["g2"], intermediates=True)
        assert ok is verdict, grp.name
        (itau, ll, rl), per_block = summed(oracle, fx, grp, D)
        assert (itau, ll, rl) == (d["itau"], d["ll"], d["rl"]), grp.name
        assert oracle.pairings_verify(ll, fx["g2"][cs.CELL_FE], rl, fx["g2"][0]) is ok, grp.name
        # no block alone is the group: the sums really are made of several parts
        assert all(b != (d["itau"], d["ll"], d["rl"]) for b in per_block), grp.name


def test_exponents_start_at_the_blocks_first_cell(oracle, fx):
    """the same cut with every block's exponents starting at 0 is another group element: the first-exponent argument is not decoration"""
    g = sc.cut_group(oracle, fx, 7)
    r, _, _ = cs.challenge(*g.args)
    _, d = cs.verify_cell_kzg_proof_batch(oracle, *g.args, mono=fx["mono"][:64], g2=fx["g2"], intermediates=True)
    wrong = [sc.block_sums(oracle, fx["mono"], r, 0, g.c[off:off + cnt], g.i[off:off + cnt], g.cells[off:off + cnt], g.p[off:off + cnt])
             for off, cnt in sc.blocks_of(7, 3)]
    assert sc.add_points(oracle, [b[1] for b in wrong]) != d["ll"]
