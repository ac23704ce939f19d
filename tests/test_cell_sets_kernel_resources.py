"""-m "not gpu": what the gfx950 build says about the `_sets` entries of k_cells.hip, the kernels of verify_cell_kzg_proof_batch_many_sets that
share their bodies with the uniform entries (kzg_rust_amd/csrc/group_geo.h).  None of them may use scratch or a dynamic stack, and the ragged forms
of k_cell_rpowers and k_cell_weights use no LDS, as the uniform ones.  Read from the code object the build left behind
(test_cell_kernel_resources.kernel_resources)."""
import re

from test_cell_kernel_resources import kernel_resources

SETS = ("k_cell_rpowers_sets", "k_cell_weights_sets", "k_cell_interp_sets", "k_cell_terms_sets", "k_cell_sum_sets")


def test_the_sets_entries_use_no_scratch(tmp_path):
    res = kernel_resources(tmp_path, "k_cells")
    found = {}
    for short in SETS:
        hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
        assert len(hits) == 1, (short, sorted(res))
        found[short] = res[hits[0]]
        print(short, found[short])
    assert {k for k in res if "_sets" in k} == {k for k in res if any(re.fullmatch(r"_ZN3kzg\d+" + s + r"E.*", k) for s in SETS)}
    for short, r in found.items():
        assert r["scratch"] == 0 and not r["dynamic_stack"], (short, r)
    assert found["k_cell_rpowers_sets"]["lds"] == 0 and found["k_cell_weights_sets"]["lds"] == 0
    # the uniform and the ragged sum are the same tree over the same 256 points of LDS
    uniform = [v for k, v in res.items() if re.fullmatch(r"_ZN3kzg\d+k_cell_sumE.*", k)]
    assert len(uniform) == 1 and uniform[0]["lds"] == found["k_cell_sum_sets"]["lds"] == 256 * 3 * 56
