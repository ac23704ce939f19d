"""-m "not gpu": what the gfx950 build says about the kernels of verify_blob_kzg_proof_batch_many_sets (k_verify.hip, k_g1.hip), read from the code
objects the build left behind (test_cell_kernel_resources.kernel_resources).  Every `_sets` kernel is there exactly once and uses neither
scratch nor a dynamic stack; and the uniform kernels beside them -- two of which now share text with a ragged entry -- report the VGPR / LDS /
scratch figures of the commit before the ragged forms existed.

PARENT: that commit (f215788) built with the same hipcc and flags and read with kernel_resources(), before any line of the ragged forms was
written.  k_rhash_lanes shares its body with k_rhash_lanes_sets through a geometry template and kept its figures; k_rpowers did not (142 -> 149
VGPRs behind the same template), so k_rpowers_sets is a sibling and k_rpowers is the parent's text.  k_lincomb_terms' 48 bytes of scratch are the
parent's too (g1_mul128_w4 indexes its digit words at run time); k_lincomb_terms_sets takes the ladder's form without that index."""
import re

from test_cell_kernel_resources import kernel_resources

SETS = {"k_verify": ("k_rhash_lanes_sets", "k_rpowers_sets", "k_err_fold_sets"),
        "k_g1": ("k_lincomb_terms_sets", "k_lincomb_finish_sets", "k_dump_intermediates_sets")}
PARENT = {"k_verify": {"k_rhash_lanes": {"vgprs": 42, "lds": 0, "scratch": 0}, "k_rpowers": {"vgprs": 142, "lds": 65664, "scratch": 0}},
          "k_g1": {"k_lincomb_terms": {"vgprs": 256, "lds": 0, "scratch": 48}, "k_lincomb_finish": {"vgprs": 183, "lds": 0, "scratch": 0}}}


def one(res, short):
    hits = [k for k in res if re.fullmatch(r"_ZN3kzg\d+" + short + r"E.*", k)]
    assert len(hits) == 1, (short, sorted(res))
    return res[hits[0]]


def test_the_sets_kernels_use_no_scratch_and_the_uniform_ones_keep_their_figures(tmp_path):
    for unit, shorts in SETS.items():
        d = tmp_path / unit
        d.mkdir()
        res = kernel_resources(d, unit)
        found = {short: one(res, short) for short in shorts}
        # every `_sets` kernel of the unit is one of the expected ones
        assert {k for k in res if "_sets" in k} == {k for k in res if any(re.fullmatch(r"_ZN3kzg\d+" + s + r"E.*", k) for s in shorts)}
        for short, r in found.items():
            print(short, r)
            assert r["scratch"] == 0 and not r["dynamic_stack"], (short, r)
        for short, want in PARENT[unit].items():
            r = one(res, short)
            print(short, r)
            assert {k: r[k] for k in want} == want and not r["dynamic_stack"], (short, r, want)
    # the ragged hash and powers kernels keep the uniform kernels' LDS (none; four waves of schedule words)
    res = kernel_resources(tmp_path / "k_verify", "k_verify")
    assert one(res, "k_rhash_lanes_sets")["lds"] == 0 and one(res, "k_rpowers_sets")["lds"] == 65664 and one(res, "k_err_fold_sets")["lds"] == 0
