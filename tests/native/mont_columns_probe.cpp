// Host build (g++) of the lazy Montgomery products of field.h in BOTH forms -- the row forms (mont_mul_lazy, mont_mul2_lazy, mont_sqr,
// mont_mulsqr2_lazy) and their column forms (mont_*_cols) -- on RAW limbs, for N = 9 (Fr) and N = 14 (Fp), so that
// tests/test_mont_columns_host.py can hand them operands at the very bounds their callers pass (raw limbs up to 2^31, lazy values with the
// excess in the top limb) and compare the two forms limb for limb and against Python big integers.
// With -DMONT_COLUMNS_MAIN the file is a stand-alone program that runs a fixed set of such operands through both forms (for a build under
// -fsanitize=undefined); it exits 0 when every pair of results agrees.  Test infrastructure only: never part of libkzg355.so.
#include "../../kzg_rust_amd/csrc/field.h"
using namespace kzg;
namespace {
const uint32_t FP_M[NFP] = FP_MOD_INIT;
const uint32_t FR_M[NFR] = FR_MOD_INIT;
template <int N> const uint32_t *mod_of() { return N == NFP ? FP_M : FR_M; }
template <int N> uint32_t inv_of() { return N == NFP ? FP_INVW : FR_INVW; }
// form 0: rows; 1: columns; 2: columns with the pin (on the host the same expression as 1)
template <int N> void mul(uint32_t *o, const uint32_t *a, const uint32_t *b, int form) {
    if (form == 0) mont_mul_lazy<N>(o, a, b, mod_of<N>(), inv_of<N>());
    else if (form == 1) mont_mul_lazy_cols<N, false>(o, a, b, mod_of<N>(), inv_of<N>());
    else mont_mul_lazy_cols<N, true>(o, a, b, mod_of<N>(), inv_of<N>());
}
template <int N> void mul2(uint32_t *o, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int form) {
    if (form == 0) mont_mul2_lazy<N>(o, a, b, c, d, mod_of<N>(), inv_of<N>());
    else if (form == 1) mont_mul2_lazy_cols<N, false>(o, a, b, c, d, mod_of<N>(), inv_of<N>());
    else mont_mul2_lazy_cols<N, true>(o, a, b, c, d, mod_of<N>(), inv_of<N>());
}
template <int N> void sqr(uint32_t *o, const uint32_t *a, int form, int lazy) {
    if (form == 0) { if (lazy) mont_sqr<N, true>(o, a, mod_of<N>(), inv_of<N>()); else mont_sqr<N, false>(o, a, mod_of<N>(), inv_of<N>()); }
    else if (form == 1) { if (lazy) mont_sqr_cols<N, true, false>(o, a, mod_of<N>(), inv_of<N>()); else mont_sqr_cols<N, false, false>(o, a, mod_of<N>(), inv_of<N>()); }
    else { if (lazy) mont_sqr_cols<N, true, true>(o, a, mod_of<N>(), inv_of<N>()); else mont_sqr_cols<N, false, true>(o, a, mod_of<N>(), inv_of<N>()); }
}
template <int N> void mulsqr2(uint32_t *o, const uint32_t *a, const uint32_t *b, const uint32_t *c, int form) {
    if (form == 0) mont_mulsqr2_lazy<N>(o, a, b, c, mod_of<N>(), inv_of<N>());
    else if (form == 1) mont_mulsqr2_lazy_cols<N, false>(o, a, b, c, mod_of<N>(), inv_of<N>());
    else mont_mulsqr2_lazy_cols<N, true>(o, a, b, c, mod_of<N>(), inv_of<N>());
}
}  // namespace
extern "C" {
// n: 9 or 14 limbs per operand; every function returns 0, or -1 for another n
int mcp_mul(uint32_t *o, const uint32_t *a, const uint32_t *b, int n, int form) {
    if (n == NFR) mul<NFR>(o, a, b, form); else if (n == NFP) mul<NFP>(o, a, b, form); else return -1;
    return 0;
}
int mcp_mul2(uint32_t *o, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int n, int form) {
    if (n == NFR) mul2<NFR>(o, a, b, c, d, form); else if (n == NFP) mul2<NFP>(o, a, b, c, d, form); else return -1;
    return 0;
}
int mcp_sqr(uint32_t *o, const uint32_t *a, int n, int form, int lazy) {
    if (n == NFR) sqr<NFR>(o, a, form, lazy); else if (n == NFP) sqr<NFP>(o, a, form, lazy); else return -1;
    return 0;
}
int mcp_mulsqr2(uint32_t *o, const uint32_t *a, const uint32_t *b, const uint32_t *c, int n, int form) {
    if (n == NFR) mulsqr2<NFR>(o, a, b, c, form); else if (n == NFP) mulsqr2<NFP>(o, a, b, c, form); else return -1;
    return 0;
}
}

#if defined(MONT_COLUMNS_MAIN)
#include <stdio.h>
namespace {
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
// kind 0: random normalised limbs; 1: every limb at `top` - 1; 2: zero; 3: the modulus itself (a lazy zero); 4: random limbs below `top`;
// 5: random canonical value (below 2^380 / 2^254)
template <int N> void fill(uint32_t *v, int kind, uint32_t top) {
    for (int i = 0; i < N; i++)
        v[i] = kind == 0 ? (rnd() & LMASK) : kind == 1 ? top - 1 : kind == 2 ? 0u : kind == 3 ? mod_of<N>()[i] : kind == 5 ? (rnd() & LMASK) : rnd() % top;
    if (kind == 5) v[N - 1] &= N == NFP ? 0x7u : 0x3fffffu;
    if (kind == 0) v[N - 1] &= N == NFP ? 0x1ffu : 0x7fffffu;      // top limb: the value stays below 2^386 (about 32 p) / 2^255
}
template <int N> bool same(const uint32_t *x, const uint32_t *y) { for (int i = 0; i < N; i++) if (x[i] != y[i]) return false; return true; }
template <int N> int run() {
    int bad = 0;
    uint32_t a[N], b[N], c[N], d[N], r0[N], r1[N], r2[N];
    for (int it = 0; it < 400; it++) {
        const int ka = it % 5, kb = (it / 5) % 4;
        // products of two: one operand may be raw (limbs below 2^31) against a normalised one; two products: raw limbs below 2^30 and 3 * 2^29
        fill<N>(a, ka, ka == 1 || ka == 4 ? (N == NFR ? 0x80000000u : 1u << LB) : 1u << LB); fill<N>(b, kb, 1u << LB);
        mul<N>(r0, a, b, 0); mul<N>(r1, a, b, 1); mul<N>(r2, a, b, 2);
        bad += !same<N>(r0, r1) || !same<N>(r0, r2);
        fill<N>(a, ka, ka == 1 || ka == 4 ? (N == NFR ? 1u << 30 : 1u << LB) : 1u << LB); fill<N>(c, ka, ka == 1 || ka == 4 ? (N == NFR ? 3u << LB : 1u << LB) : 1u << LB);
        fill<N>(d, (kb + 1) % 4, 1u << LB);
        mul2<N>(r0, a, b, c, d, 0); mul2<N>(r1, a, b, c, d, 1); mul2<N>(r2, a, b, c, d, 2);
        bad += !same<N>(r0, r1) || !same<N>(r0, r2);
        // squares and product-plus-doubled-square: normalised operands only (their callers pass lazy values)
        fill<N>(a, kb, 1u << LB); fill<N>(c, (kb + 2) % 4, 1u << LB);
        sqr<N>(r0, a, 0, 1); sqr<N>(r1, a, 1, 1); sqr<N>(r2, a, 2, 1);
        bad += !same<N>(r0, r1) || !same<N>(r0, r2);
        fill<N>(d, kb == 2 ? 2 : 5, 1u << LB);                       // the canonical square takes a canonical operand
        sqr<N>(r0, d, 0, 0); sqr<N>(r1, d, 1, 0); sqr<N>(r2, d, 2, 0);
        bad += !same<N>(r0, r1) || !same<N>(r0, r2);
        mulsqr2<N>(r0, a, b, c, 0); mulsqr2<N>(r1, a, b, c, 1); mulsqr2<N>(r2, a, b, c, 2);
        bad += !same<N>(r0, r1) || !same<N>(r0, r2);
    }
    return bad;
}
}  // namespace
int main() {
    const int bad = run<NFR>() + run<NFP>();
    printf("mont_columns: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
