// Host build (g++) of the lazy G1 chain arithmetic (field.h, g1.h) with RAW limb operands, so that tests/test_lazy_chain_host.py can
// hand the routines lazy values at the very bounds their callers pass -- something the byte-level ABI of hd_probe.cpp cannot express --
// and check the results against Python big integers.  Test infrastructure only: this file is never part of libkzg355.so.
#include "../../kzg_rust_amd/csrc/field.h"
#include "../../kzg_rust_amd/csrc/g1.h"
using namespace kzg;
namespace {
void load(Fp &r, const uint32_t *l) { for (int i = 0; i < NFP; i++) r.l[i] = l[i]; }
void store(uint32_t *l, const Fp &a) { for (int i = 0; i < NFP; i++) l[i] = a.l[i]; }
void load_jac(G1Jac &r, const uint32_t *l) { load(r.x, l); load(r.y, l + NFP); load(r.z, l + 2 * NFP); }
void store_jac(uint32_t *l, const G1Jac &a) { store(l, a.x); store(l + NFP, a.y); store(l + 2 * NFP, a.z); }
}
extern "C" {
// out = (a b + 2 c^2) / R as fp_mulsqr2_lz leaves it (lazy: not reduced below p); 14 limbs each
void lcp_mulsqr2(uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c) {
    Fp x, y, z, r; load(x, a); load(y, b); load(z, c);
    fp_mulsqr2_lz(r, x, y, z);
    store(out, r);
}
// out = (a b + c d) / R as fp_mul2_lz leaves it (the fused Y3 of the lazy additions)
void lcp_mul2(uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d) {
    Fp x, y, z, w, r; load(x, a); load(y, b); load(z, c); load(w, d);
    fp_mul2_lz(r, x, y, z, w);
    store(out, r);
}
// k lazy doublings of the Jacobian point `in` (3 x 14 raw limbs, lazy Montgomery coordinates): raw = the chain's value as it stands (for the
// bound checks), canon = after g1_canon_lazy, ref = the canonical chain g1_add(P, P) from the canonicalised input.  r aliases p, as in the kernels.
void lcp_dbl_chain(uint32_t *raw, uint32_t *canon, uint32_t *ref, const uint32_t *in, int k) {
    G1Jac a; load_jac(a, in);
    G1Jac b; g1_canon_lazy(b, a);
    for (int i = 0; i < k; i++) g1_dbl_lazy(a, a);
    store_jac(raw, a);
    G1Jac c; g1_canon_lazy(c, a); store_jac(canon, c);
    for (int i = 0; i < k; i++) { G1Jac t = b; g1_add(b, t, t); }
    store_jac(ref, b);
}
// a + b through g1_add_lazy (b canonical) / g1_add_lazy2 (both lazy) / g1x_add_lazy2 (XYZZ: 4 x 14 limbs each); out = raw result
void lcp_add_lazy(uint32_t *out, const uint32_t *a, const uint32_t *b, int both_lazy) {
    G1Jac x, y, r; load_jac(x, a); load_jac(y, b);
    if (both_lazy) g1_add_lazy2(r, x, y); else g1_add_lazy(r, x, y);
    store_jac(out, r);
}
void lcp_addx_lazy2(uint32_t *out, const uint32_t *a, const uint32_t *b) {
    G1X x, y; load(x.x, a); load(x.y, a + NFP); load(x.zz, a + 2 * NFP); load(x.zzz, a + 3 * NFP);
    load(y.x, b); load(y.y, b + NFP); load(y.zz, b + 2 * NFP); load(y.zzz, b + 3 * NFP);
    g1x_add_lazy2(x, x, y);                                      // (r aliases a, as in k_lc_wsum)
    store(out, x.x); store(out + NFP, x.y); store(out + 2 * NFP, x.zz); store(out + 3 * NFP, x.zzz);
}
// both subgroup predicates on an affine point given as canonical Montgomery limbs (2 x 14; all zero = infinity); bit 0: endomorphism form, bit 1: [r]P
int lcp_subgroup(const uint32_t *xy) {
    G1Affine p; load(p.x, xy); load(p.y, xy + NFP);
    return (g1_in_subgroup(p) ? 1 : 0) | (g1_in_subgroup_naive(p) ? 2 : 0);
}
// g1_decompress: return code, and the point as canonical Montgomery limbs
int lcp_decompress(uint32_t *xy, const uint8_t *in48) {
    G1Affine p = g1a_inf();
    const int rc = g1_decompress(p, in48);
    if (rc == 0) { store(xy, p.x); store(xy + NFP, p.y); }
    return rc;
}
// fp_sqrt on canonical Montgomery limbs: 1 and the root, or 0
int lcp_sqrt(uint32_t *out, const uint32_t *a) {
    Fp x, r; load(x, a);
    if (!fp_sqrt(r, x)) return 0;
    store(out, r); return 1;
}
}
