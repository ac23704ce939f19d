// field.h -- Fp (381-bit) and Fr (255-bit) Montgomery arithmetic for gfx950, unsaturated 29-bit limbs.
//
// Why 29-bit limbs: measured on MI355X (profiles/r01_valu_issue_rates.txt) v_mad_u64_u32 issues at
// the same rate as any other VALU op, so the cost of a field product is its instruction COUNT.
// With limbs < 2^29 every column sum of a Montgomery product (<= 28 terms < 2^58 each; up to 58 such units where two products or a product and a
// doubled square share one reduction: mont_units() below counts them and every body asserts the count) fits a 64-bit
// accumulator, so each limb product is exactly ONE v_mad_u64_u32 with no carry handling: an Fp product
// is 2*14*14 = 392 mads + ~100 shift/mask ops, versus ~1350 instructions for saturated 32-bit limbs
// (288 mads + carry/zero-extension traffic).  Fp: 14 limbs (R = 2^406), Fr: 9 limbs (R = 2^261).
// All products are three bodies (mont_mul, mont_sqr, mont_cols) under one overflow bound; the lazy forms and the column forms are wrappers of
// those (the Montgomery section below).
//
// Every value is kept CANONICAL (limbs < 2^29, value < modulus) so equality is limb equality.
// Reference counterpart: the blst_fp / blst_fr types behind src/utils.rs, src/kzg.rs;
// blst's 64-bit-limb R = 2^384 / 2^256 layout is deliberately not reproduced.
//
// Everything is KZG_HD (host+device): the same source is unit-tested with g++ on the CPU build box
// (tests/native/hd_probe.cpp) before it runs on a GPU.  The product ships only device instantiations.
#pragma once
#include <stdint.h>
#include "consts_gen.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KZG_HD __host__ __device__ __forceinline__
#define KZG_HD_NOINLINE inline __host__ __device__ __attribute__((noinline))
#else
#define KZG_HD inline __attribute__((always_inline))
#define KZG_HD_NOINLINE inline __attribute__((noinline))
#endif

namespace kzg {

constexpr int LB = KZG_LIMB_BITS;                 // 29
constexpr uint32_t LMASK = (1u << LB) - 1u;
constexpr int NFP = KZG_FP_LIMBS;                 // 14
constexpr int NFR = KZG_FR_LIMBS;                 // 9

struct Fp { uint32_t l[NFP]; };
struct Fr { uint32_t l[NFR]; };

// ---------------------------------------------------------------------------------- limb helpers
// r = a - b over N 29-bit limbs (mod 2^(29N)); returns 1 if a < b
template <int N> KZG_HD uint32_t ul_sub(uint32_t *r, const uint32_t *a, const uint32_t *b) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint32_t d = a[i] - b[i] - borrow;
        borrow = d >> 31;
        r[i] = d & LMASK;
    }
    return borrow;
}
template <int N> KZG_HD bool ul_is_zero(const uint32_t *a) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < N; i++) t |= a[i];
    return t == 0;
}
template <int N> KZG_HD bool ul_eq(const uint32_t *a, const uint32_t *b) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < N; i++) t |= a[i] ^ b[i];
    return t == 0;
}
// a + b mod m  (a, b canonical)
template <int N> KZG_HD void mod_add(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *m) {
    // d = a + b - m with a signed carry chain; if it went negative add m back
    uint32_t d[N];
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        int32_t t = (int32_t)(a[i] + b[i] - m[i]) + c;
        c = t >> LB;
        d[i] = (uint32_t)t & LMASK;
    }
    const uint32_t neg = (uint32_t)c;      // 0 or 0xffffffff
    uint32_t cc = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint32_t t = d[i] + (m[i] & neg) + cc;
        cc = t >> LB;
        r[i] = t & LMASK;
    }
}
// a - b mod m
template <int N> KZG_HD void mod_sub(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *m) {
    uint32_t d[N];
    const uint32_t neg = 0u - ul_sub<N>(d, a, b);
    uint32_t cc = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint32_t t = d[i] + (m[i] & neg) + cc;
        cc = t >> LB;
        r[i] = t & LMASK;
    }
}
// ---------------------------------------------------------------------------------- Montgomery products
// r = (a b + c d + 2^SH e^2) / 2^(29N) mod m (whichever of the three terms a routine takes), inv = -m^-1 mod 2^29, reduced word by word: every limb
// product and every q_i m[j] is ONE multiply-add into the 64-bit accumulator of its weight, and carries move only when a weight is finished.  Three
// bodies take the same products in three orders; for the same operands they compute the same quotient digits q_i and the same result limbs, bit
// for bit (tests/test_mont_columns_host.py).
//   mont_mul   N accumulators, operand scanning: round i adds a[j] b[i] (TWO: and c[j] d[i]) and q_i m[j] to acc[j], then shifts the lowest
//              accumulator (now zero mod 2^29) out.  No carries until the final sweep.  TWO: two products share one reduction, 3 N^2 multiply-adds
//              instead of 4 N^2.  Wrappers: mont_mul_lazy, mont_mul2_lazy.
//   mont_sqr   2N accumulators, all limb products first, then the reduction: 2^SH a^2 + (AB ? x y : 0).  The square is taken by its N (N + 1) / 2
//              distinct limb products, a << SH on the diagonal and a << (SH + 1) off it (Fp: 105 + 196 multiply-adds for a square against 392; 497 for
//              x y + 2 a^2 against 693 apart).  The factor 2^SH sits in shifted copies of the limbs (32-bit words: SH <= 2), and the bound below
//              allows SH = 1 at N = 14; the doubling chain, which needs 8 B^2, passes a = 2B normalised, so that the rest of the factor sits in the
//              VALUE and not in every limb product.  Wrapper: mont_mulsqr2_lazy.
//   mont_cols  ONE accumulator, product scanning: column k = sum_{i+j=k} (limb products) + sum_i q_i m[k-i], started from the column below >> 29.
//              The carry is then the addend of the column's first multiply-add (v_mad_u64_u32 has a 64-bit addend, which the row forms feed a
//              literal 0 once per column), and the columns N .. 2N-1 ARE the result limbs: the row forms' N carry additions and their final sweep
//              of N - 1 additions are gone, the multiply-adds are the same in number.  FULL in {0, 1, 2} full products (a b, c d) per column; SH >= 0
//              adds 2^SH e^2 by half products, SH = -1 no square.  Wrappers: mont_mul_lazy_cols, mont_mul2_lazy_cols, mont_sqr_cols,
//              mont_mulsqr2_lazy_cols.  The row forms stay the default: KZG_MONT_COLS_FR selects the lazy Fr pair by columns for a translation
//              unit, fp_mul_lz<COLS> / fp_sqr_lz<COLS> are selected by the point routine (below).
// LAZY leaves out the final conditional subtraction and keeps the top limb unmasked: the result is < m (1 + value / (m 2^(29N))) with every limb below
// the top one normalised (< 2^29), which is all a following product or a bounded number of additions needs; the last operation of a chain is canonical.
// Saves ~45 of ~316 (Fr) instructions per product on the throughput kernels.
//
// Why the canonical names ARE the two row bodies, and why each body spells out its own sweep and tail: every level of forwarding, above or below,
// gives the optimiser one more round over the body while m is still a pointer, and the conditional subtraction then comes out of the compiler in
// another shape once m is the constant modulus (its top limb's borrow as x + (2^29 - m) and x < m, or as one x - m < 0): a few instructions in every
// kernel with a canonical product, registers and spills with them (EXPERIMENTS.md, "Montgomery bodies folded").  The lazy forms do not care.
//
// The overflow bound, once, for all three.  An accumulator of one weight k collects, in units of 2^58 (one product of two limbs below 2^29):
//     FULL N           limb products x[j] y[i], i + j = k, of the FULL full products,
//     N                reduction products q_i m[k-i],
//     2^(SH+1) (N/2)   cross products (2^(SH+1) e_i) e_j of the square -- the pairs i < j with i + j = k, N / 2 of them and not N --
//     2^SH             and its one diagonal (2^SH e_i) e_i,
// and, when its turn comes, the carry of the weight below, < 2^35.  mont_units() is that count and every body asserts mont_units() < 64: at most
// 63 * 2^58 + 2^35 < 2^64.  The largest in use is a b + 2 c^2 at N = 14: 2 * 14 + 4 * 7 + 2 = 58.  (That count was once noted as "not true of 15
// limbs"; it is 60 at N = 15 and first fails, with 66, at N = 16.)  The unit assumes every limb below 2^29; the top limb of a lazy value is smaller still
// (Fp: < 2^10 for a value below 2^6 p), and fp_sub_lz / fp_add_lz / fr_add_lazy / the lazy products leave every other limb normalised.  RAW operands
// (limbs not normalised) are inside the bound only where counted by hand, which is for N = 9 (eval_core.h), in either order of the products:
//     one product, one operand raw with limbs up to 2^31 against a normalised one:  9 * 2^60 + 9 * 2^58 + carry < 2^64;
//     two products, A with limbs < 2^30 and B with limbs < 3 * 2^29 against normalised z^k, s:  9 (2^59 + 3 * 2^58 + 2^58) = 27 * 2^59 < 2^63.8.
//
// Operand contracts (value bounds; "lazy" = every limb below the top one < 2^29).  r may be any of the operands.
//     mont_mul                                    a, b limbs < 2^29, a b < m 2^(29N)                     r canonical (t < m + a b / R, one subtraction)
//     mont_sqr, mont_sqr_cols                     a canonical (LAZY: lazy, as mont_mul_lazy)             r canonical (LAZY: as mont_mul_lazy)
//     mont_mul_lazy, mont_mul_lazy_cols           lazy; N = 9: a, b < ~2.6 m, one may be raw (above);    r < 1.1 m
//                                                 N = 14: a, b < 2^6 m                                   r < m (1 + 2^-13)
//     mont_mul2_lazy, mont_mul2_lazy_cols         lazy; N = 9: a b + c d < ~5 m^2, a, c may be raw       r < 1.1 m
//                                                 (above); N = 14: a b + c d < 2^12 m^2                  r < m (1 + 2^-13)
//     mont_mulsqr2_lazy, mont_mulsqr2_lazy_cols   lazy, a b + 2 c^2 < 2^12 m^2                           r < m (1 + 2^-13)
constexpr int mont_units(int N, int FULL, int SH) { return (FULL + 1) * N + (SH < 0 ? 0 : (2 << SH) * (N / 2) + (1 << SH)); }

// (callers write mont_mul<N>(r, a, b, m, inv); TWO, LAZY and the trailing c, d are for the wrappers mont_mul_lazy / mont_mul2_lazy alone)
template <int N, bool TWO = false, bool LAZY = false> KZG_HD void mont_mul(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *m, const uint32_t inv,
                                                                           const uint32_t *c = nullptr, const uint32_t *d = nullptr) {
    static_assert(mont_units(N, TWO ? 2 : 1, -1) < 64, "an accumulator's limb and reduction products and a carry must stay below 2^64");
    uint64_t acc[N];
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t bi = b[i], di = TWO ? d[i] : 0u;
#pragma unroll
        for (int j = 0; j < N; j++) { acc[j] += (uint64_t)a[j] * bi; if (TWO) acc[j] += (uint64_t)c[j] * di; }
        const uint32_t q = ((uint32_t)acc[0] * inv) & LMASK;
#pragma unroll
        for (int j = 0; j < N; j++) acc[j] += (uint64_t)q * m[j];
        const uint64_t carry = acc[0] >> LB;
#pragma unroll
        for (int j = 0; j < N - 1; j++) acc[j] = acc[j + 1];
        acc[N - 1] = 0;
        acc[0] += carry;
    }
    uint32_t t[N];
    uint32_t *o = LAZY ? r : t;                                    // (every operand has been read by now)
    uint64_t cy = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        cy += acc[j];
        o[j] = (LAZY && j == N - 1) ? (uint32_t)cy : ((uint32_t)cy & LMASK);     // LAZY: the top limb keeps any excess
        cy >>= LB;
    }
    if (LAZY) return;
    uint32_t s[N];
    const uint32_t br = ul_sub<N>(s, t, m);
#pragma unroll
    for (int j = 0; j < N; j++) r[j] = br ? t[j] : s[j];
}
// (callers write mont_sqr<N, LAZY>(r, a, m, inv); AB, SH and the trailing x, y are for the wrapper mont_mulsqr2_lazy alone, whose (a, b, c) arrive
// here as (x, y, a): the squared operand is a in this body)
template <int N, bool LAZY = false, bool AB = false, int SH = 0> KZG_HD void mont_sqr(uint32_t *r, const uint32_t *a, const uint32_t *m, const uint32_t inv,
                                                                                     const uint32_t *x = nullptr, const uint32_t *y = nullptr) {
    static_assert(SH >= 0 && LB + SH + 1 <= 32 && mont_units(N, AB ? 1 : 0, SH) < 64,
                  "an accumulator's limb and reduction products and a carry must stay below 2^64");
    uint64_t acc[2 * N];
    uint32_t a1[N], a2[N];
#pragma unroll
    for (int j = 0; j < N; j++) { a1[j] = a[j] << SH; a2[j] = a[j] << (SH + 1); }
#pragma unroll
    for (int k = 0; k < 2 * N; k++) acc[k] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (AB) {
            const uint32_t yi = y[i];
#pragma unroll
            for (int j = 0; j < N; j++) acc[i + j] += (uint64_t)x[j] * yi;
        }
        acc[2 * i] += (uint64_t)a1[i] * a[i];
#pragma unroll
        for (int j = i + 1; j < N; j++) acc[i + j] += (uint64_t)a2[i] * a[j];
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t q = ((uint32_t)acc[i] * inv) & LMASK;
#pragma unroll
        for (int j = 0; j < N; j++) acc[i + j] += (uint64_t)q * m[j];
        acc[i + 1] += acc[i] >> LB;
    }
    uint32_t t[N];
    uint32_t *o = LAZY ? r : t;
    uint64_t cy = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        cy += acc[N + j];
        o[j] = (LAZY && j == N - 1) ? (uint32_t)cy : ((uint32_t)cy & LMASK);
        cy >>= LB;
    }
    if (LAZY) return;
    uint32_t s[N];
    const uint32_t br = ul_sub<N>(s, t, m);
#pragma unroll
    for (int j = 0; j < N; j++) r[j] = br ? t[j] : s[j];
}
// PIN: left alone the compiler re-associates a column into (products summed from 0) + carry -- its reassociation adds the value computed last
// at the end -- which puts the 64-bit addition back (and for N = 14 gives the row forms' code again).  With PIN the device build passes the
// accumulator through __builtin_annotation after every multiply-add: the intrinsic returns its argument and generates no instruction, but the
// optimiser does not look through it, so each sum keeps the shape it is written in and the accumulator stays the addend.  (An empty asm
// statement pins as well, but the hazard recogniser then puts an s_nop before every multiply-add that reads the asm's result; an assumption
// such as acc != 2^64 - 1 is dropped wherever the limbs' ranges are known, which is after every fp_sub_lz.)  The host build, and PIN = false,
// are the plain expression.
template <bool PIN> KZG_HD void col_mad(uint64_t &acc, const uint32_t x, const uint32_t y) {
    acc += (uint64_t)x * y;
#if defined(__HIP_DEVICE_COMPILE__)
    if (PIN) acc = __builtin_annotation(acc, "col");
#endif
}
// the reduction half of column k: the q_i m[k-i] of the quotient digits known so far, then for k < N the new digit q_k (which clears the column's
// low 29 bits), for k >= N the result limb k - N.  Leaves the accumulator shifted for column k + 1.
template <int N, bool PIN> KZG_HD void col_reduce(uint64_t &acc, uint32_t *q, uint32_t *r, const int k, const uint32_t *m, const uint32_t inv) {
    if (k < N) {
#pragma unroll
        for (int i = 0; i < N; i++) if (i < k) col_mad<PIN>(acc, q[i], m[k - i]);
        q[k] = ((uint32_t)acc * inv) & LMASK;
        acc += (uint64_t)q[k] * m[0];
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) if (i > k - N) col_mad<PIN>(acc, q[i], m[k - i]);
        r[k - N] = (uint32_t)acc & LMASK;
    }
    acc >>= LB;
}
// Within a column: the full products, interleaved per i; the diagonal (k / 2, k / 2); the cross pairs (i, k - i) with i < k - i < N; the reduction.
template <int N, bool PIN, int FULL, int SH, bool LAZY> KZG_HD void mont_cols(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *c,
                                                                              const uint32_t *d, const uint32_t *e, const uint32_t *m, const uint32_t inv) {
    static_assert(FULL >= 0 && FULL <= 2 && SH >= -1 && LB + SH + 1 <= 32 && mont_units(N, FULL, SH) < 64,
                  "a column's limb and reduction products and a carry must stay below 2^64");
    constexpr int S = SH < 0 ? 0 : SH;
    uint32_t q[N], t[N], e1[N], e2[N];
    if (SH >= 0) {
#pragma unroll
        for (int j = 0; j < N; j++) { e1[j] = e[j] << S; e2[j] = e[j] << (S + 1); }
    }
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * N - 1; k++) {
        if (FULL >= 1) {
#pragma unroll
            for (int i = 0; i < N; i++) if (i <= k && k - i < N) { col_mad<PIN>(acc, a[k - i], b[i]); if (FULL == 2) col_mad<PIN>(acc, c[k - i], d[i]); }
        }
        if (SH >= 0) {
            if (!(k & 1)) col_mad<PIN>(acc, e1[k / 2], e[k / 2]);
#pragma unroll
            for (int i = 0; i < N; i++) if (2 * i < k && k - i < N) col_mad<PIN>(acc, e2[i], e[k - i]);
        }
        col_reduce<N, PIN>(acc, q, t, k, m, inv);                  // (into t: the operands are still being read)
    }
    t[N - 1] = (uint32_t)acc;      // column 2N - 1: the carry alone; LAZY: the top limb keeps any excess (canonical: t < 2m, it needs no mask)
    if (LAZY) {
#pragma unroll
        for (int j = 0; j < N; j++) r[j] = t[j];
        return;
    }
    uint32_t s[N];
    const uint32_t br = ul_sub<N>(s, t, m);
#pragma unroll
    for (int j = 0; j < N; j++) r[j] = br ? t[j] : s[j];
}
// The other seven names.  (mont_mul has no column sibling: no canonical product sits on a throughput path.)
template <int N> KZG_HD void mont_mul_lazy(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *m, const uint32_t inv) {
    mont_mul<N, false, true>(r, a, b, m, inv);
}
template <int N> KZG_HD void mont_mul2_lazy(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                                            const uint32_t *m, const uint32_t inv) {
    mont_mul<N, true, true>(r, a, b, m, inv, c, d);
}
template <int N> KZG_HD void mont_mulsqr2_lazy(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *m, const uint32_t inv) {
    mont_sqr<N, true, true, 1>(r, c, m, inv, a, b);
}
template <int N, bool PIN = false> KZG_HD void mont_mul_lazy_cols(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *m, const uint32_t inv) {
    mont_cols<N, PIN, 1, -1, true>(r, a, b, nullptr, nullptr, nullptr, m, inv);
}
template <int N, bool PIN = false> KZG_HD void mont_mul2_lazy_cols(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                                                                   const uint32_t *m, const uint32_t inv) {
    mont_cols<N, PIN, 2, -1, true>(r, a, b, c, d, nullptr, m, inv);
}
template <int N, bool LAZY = false, bool PIN = false> KZG_HD void mont_sqr_cols(uint32_t *r, const uint32_t *a, const uint32_t *m, const uint32_t inv) {
    mont_cols<N, PIN, 0, 0, LAZY>(r, nullptr, nullptr, nullptr, nullptr, a, m, inv);
}
template <int N, bool PIN = false> KZG_HD void mont_mulsqr2_lazy_cols(uint32_t *r, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *m,
                                                                      const uint32_t inv) {
    mont_cols<N, PIN, 1, 1, true>(r, a, b, nullptr, nullptr, c, m, inv);
}
// 32-bit word array (little-endian words, NW of them) -> N 29-bit limbs
template <int N, int NW> KZG_HD void words_to_limbs(uint32_t *l, const uint32_t *w) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int bit = LB * k, wi = bit >> 5, sh = bit & 31;
        uint32_t lo = wi < NW ? w[wi] : 0u;
        uint32_t hi = (wi + 1) < NW ? w[wi + 1] : 0u;
        uint32_t v = sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
        l[k] = v & LMASK;
    }
}
// N 29-bit limbs -> NW 32-bit words (value must fit)
template <int N, int NW> KZG_HD void limbs_to_words(uint32_t *w, const uint32_t *l) {
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int bit = 32 * i, k = bit / LB, sh = bit % LB;     // word i starts inside limb k at offset sh
        uint32_t v = k < N ? (l[k] >> sh) : 0u;
        if ((k + 1) < N) v |= l[k + 1] << (LB - sh);             // LB - sh in [1,29]
        if ((k + 2) < N && (2 * LB - sh) < 32) v |= l[k + 2] << (2 * LB - sh);
        w[i] = v;
    }
}

// ---------------------------------------------------------------------------------- Fp
#define KZG_FP_CONSTS const uint32_t FP_MOD[NFP] = FP_MOD_INIT;
KZG_HD Fp fp_zero() { Fp r; for (int i = 0; i < NFP; i++) r.l[i] = 0; return r; }
KZG_HD Fp fp_one() { const uint32_t c[NFP] = FP_ONE_INIT; Fp r; for (int i = 0; i < NFP; i++) r.l[i] = c[i]; return r; }
KZG_HD void fp_add(Fp &r, const Fp &a, const Fp &b) { KZG_FP_CONSTS mod_add<NFP>(r.l, a.l, b.l, FP_MOD); }
KZG_HD void fp_sub(Fp &r, const Fp &a, const Fp &b) { KZG_FP_CONSTS mod_sub<NFP>(r.l, a.l, b.l, FP_MOD); }
KZG_HD void fp_dbl(Fp &r, const Fp &a) { KZG_FP_CONSTS mod_add<NFP>(r.l, a.l, a.l, FP_MOD); }
KZG_HD void fp_neg(Fp &r, const Fp &a) { Fp z = fp_zero(); fp_sub(r, z, a); }
KZG_HD bool fp_is_zero(const Fp &a) { return ul_is_zero<NFP>(a.l); }
KZG_HD bool fp_eq(const Fp &a, const Fp &b) { return ul_eq<NFP>(a.l, b.l); }
// (a translation unit that defines KZG_FP_MUL_NOINLINE before this header calls the two canonical products out of line)
#if defined(KZG_FP_MUL_NOINLINE)
#define KZG_FP_MUL_ATTR KZG_HD_NOINLINE
#else
#define KZG_FP_MUL_ATTR KZG_HD
#endif
KZG_FP_MUL_ATTR void fp_mul(Fp &r, const Fp &a, const Fp &b) { KZG_FP_CONSTS mont_mul<NFP>(r.l, a.l, b.l, FP_MOD, FP_INVW); }
KZG_FP_MUL_ATTR void fp_sqr(Fp &r, const Fp &a) { KZG_FP_CONSTS mont_sqr<NFP>(r.l, a.l, FP_MOD, FP_INVW); }
// ---- lazy (unreduced) Fp: R = 2^406 leaves 25 bits above p, so values may run up to a few dozen p between reductions.
// Products of operands a < 2^6 p, b < 2^6 p come out below p (1 + 2^-13) without the final conditional subtraction; sums are
// plain limb additions with carry normalisation; differences add a multiple of p first.  Used by the accumulation loops of the
// MSM / bucket kernels (g1x_add_mixed_lazy), which spend ~15 % of a canonical addition in those subtractions and selects.
KZG_HD void fp_mul_lz(Fp &r, const Fp &a, const Fp &b) { KZG_FP_CONSTS mont_mul_lazy<NFP>(r.l, a.l, b.l, FP_MOD, FP_INVW); }
KZG_HD void fp_sqr_lz(Fp &r, const Fp &a) { KZG_FP_CONSTS mont_sqr<NFP, true>(r.l, a.l, FP_MOD, FP_INVW); }
// The same two with the form as a template flag, for the point routines that carry one (g1.h: g1x_add_mixed_lazy<COLS>): COLS takes the column forms,
// same limbs out.  The kernels of one translation unit disagree about them (EXPERIMENTS.md, "Montgomery products by columns"): the bucket kernel of the
// batch linear combination gains 2.5-3.9 %, the point validation and the tail of the linear combination spill more registers and lose, so there is no
// unit-wide switch for Fp, and fp_mul2_lz / fp_mulsqr2_lz -- which only those kernels run -- stay in their row forms.
template <bool COLS> KZG_HD void fp_mul_lz(Fp &r, const Fp &a, const Fp &b) {
    KZG_FP_CONSTS
    if (COLS) mont_mul_lazy_cols<NFP, true>(r.l, a.l, b.l, FP_MOD, FP_INVW); else mont_mul_lazy<NFP>(r.l, a.l, b.l, FP_MOD, FP_INVW);
}
template <bool COLS> KZG_HD void fp_sqr_lz(Fp &r, const Fp &a) {
    KZG_FP_CONSTS
    if (COLS) mont_sqr_cols<NFP, true, true>(r.l, a.l, FP_MOD, FP_INVW); else mont_sqr<NFP, true>(r.l, a.l, FP_MOD, FP_INVW);
}
// r = (a b + c d) / R, lazily, ONE Montgomery reduction for the two products (588 limb products instead of 784).  Operands normalised lazy values
// with a b + c d < 2^12 p^2 (e.g. a < 6p, b < 10p, c < 4p, d < 2p in the point additions); result < p (1 + 2^-13).
KZG_HD void fp_mul2_lz(Fp &r, const Fp &a, const Fp &b, const Fp &c, const Fp &d) { KZG_FP_CONSTS mont_mul2_lazy<NFP>(r.l, a.l, b.l, c.l, d.l, FP_MOD,
        FP_INVW); }
// r = (a b + 2 c^2) / R, lazily, ONE Montgomery reduction for a product and a doubled square (497 limb products instead of 693).  Operands normalised
// lazy values with a b + 2 c^2 < 2^12 p^2 (the doubling: a = E < 4p, b < 16p, c = 2B < 4p); result < p (1 + 2^-13).
KZG_HD void fp_mulsqr2_lz(Fp &r, const Fp &a, const Fp &b, const Fp &c) { KZG_FP_CONSTS mont_mulsqr2_lazy<NFP>(r.l, a.l, b.l, c.l, FP_MOD, FP_INVW); }
// r = a + kp - b, kp a multiple of p with a + kp - b >= 0 (kp >= b is enough; g1_dbl_lazy passes a smaller kp where a's own bias covers the
// rest): limbs normalised (signed carries), the top limb keeps the excess
KZG_HD void fp_sub_lz(Fp &r, const Fp &a, const Fp &b, const uint32_t *kp) {
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < NFP; i++) {
        const int32_t t = (int32_t)a.l[i] + (int32_t)kp[i] - (int32_t)b.l[i] + c;
        if (i < NFP - 1) { c = t >> LB; r.l[i] = (uint32_t)t & LMASK; }
        else r.l[i] = (uint32_t)t;
    }
}
// r = a + b + b2 (b2 optional second addend), normalised
KZG_HD void fp_add_lz(Fp &r, const Fp &a, const Fp &b) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < NFP; i++) { const uint32_t t = a.l[i] + b.l[i] + c; if (i < NFP - 1) { c = t >> LB; r.l[i] = t & LMASK; } else r.l[i] = t; }
}
// value < 64 p -> canonical
KZG_HD void fp_canon64(Fp &r, const Fp &a) {
    const uint32_t m32[NFP] = FP_MOD32_INIT, m16[NFP] = FP_MOD16_INIT, m8[NFP] = FP_MOD8_INIT, m4[NFP] = FP_MOD4_INIT, m2[NFP] = FP_MOD2_INIT,
            m1[NFP] = FP_MOD_INIT;
    uint32_t v[NFP], s[NFP];
#pragma unroll
    for (int i = 0; i < NFP; i++) v[i] = a.l[i];
    const uint32_t *ms[6] = {m32, m16, m8, m4, m2, m1};
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint32_t br = ul_sub<NFP>(s, v, ms[k]);
#pragma unroll
        for (int i = 0; i < NFP; i++) v[i] = br ? v[i] : s[i];
    }
#pragma unroll
    for (int i = 0; i < NFP; i++) r.l[i] = v[i];
}
KZG_HD void fp_canon16(Fp &r, const Fp &a) { fp_canon64(r, a); }
// could the lazy value v in [0, 64p) be a multiple of p?  exact filter on the low limb: v = j p  =>  j = v0 * p^-1 mod 2^29
KZG_HD bool fp_maybe_zero_lz(const Fp &v) { return ((v.l[0] * FP_PINVW) & LMASK) < 64u; }
KZG_HD void fp_select(Fp &r, bool take_b, const Fp &a, const Fp &b) {
#pragma unroll
    for (int i = 0; i < NFP; i++) r.l[i] = take_b ? b.l[i] : a.l[i];
}
// canonical integer value (not Montgomery) as limbs
KZG_HD void fp_from_mont(uint32_t out[NFP], const Fp &a) {
    KZG_FP_CONSTS
    uint32_t one[NFP];
#pragma unroll
    for (int i = 0; i < NFP; i++) one[i] = i == 0 ? 1u : 0u;
    mont_mul<NFP>(out, a.l, one, FP_MOD, FP_INVW);
}
KZG_HD void fp_to_mont(Fp &r, const uint32_t in[NFP]) {
    KZG_FP_CONSTS
    const uint32_t R2[NFP] = FP_R2_INIT;
    mont_mul<NFP>(r.l, in, R2, FP_MOD, FP_INVW);
}
// a^e, e given as 12 plain 32-bit words (<= 384 bits), square-and-multiply MSB first.
// Rolled loop on purpose: a single fp_mul body in the instruction stream.
KZG_HD void fp_pow(Fp &r, const Fp &a, const uint32_t *e) {
    Fp acc = fp_one();
    bool started = false;
    for (int i = 383; i >= 0; i--) {
        if (started) fp_sqr(acc, acc);
        if ((e[i >> 5] >> (i & 31)) & 1) {
            if (started) fp_mul(acc, acc, a); else { acc = a; started = true; }
        }
    }
    r = acc;
}
// a^(p-2): kept as the independent cross-check of the divstep inversion (modinv.h) that fp_inv uses
KZG_HD void fp_inv_fermat(Fp &r, const Fp &a) { const uint32_t e[12] = FP_EXP_INV_INIT; fp_pow(r, a, e); }
// sqrt for p = 3 mod 4: a^((p+1)/4); false if a is not a square
KZG_HD bool fp_sqrt(Fp &r, const Fp &a) {
    // a^((p+1)/4), p = 3 mod 4.  Left-to-right over the 379-bit exponent with a sliding window of four bits over the odd powers
    // a, a^3, .., a^15: 375 squarings + 78 + 8 products (two-bit window: 377 + 142 + 2; bit by bit: 378 + 228), on lazy products (no
    // reduction below p until the end).  The exponent is a constant: every branch below is uniform across a wave.
    const uint32_t e[12] = FP_EXP_SQRT_INIT;
    Fp tab[8], a2, acc;
    fp_sqr_lz(a2, a);
    tab[0] = a;
#pragma unroll
    for (int k = 1; k < 8; k++) fp_mul_lz(tab[k], tab[k - 1], a2);
    auto bit = [&](int i) -> uint32_t { return (e[i >> 5] >> (i & 31)) & 1u; };
    bool started = false;
    int i = 383;
    while (i >= 0 && !bit(i)) i--;
    while (i >= 0) {
        if (!bit(i)) { fp_sqr_lz(acc, acc); i--; continue; }
        int l = i + 1 < 4 ? i + 1 : 4;
        while (!bit(i - l + 1)) l--;                              // the window ends in a set bit
        uint32_t v = 0;
        for (int k = 0; k < l; k++) v = (v << 1) | bit(i - k);
        if (started) for (int k = 0; k < l; k++) fp_sqr_lz(acc, acc);
        switch (v >> 1) {                                         // constant table index in every arm: the table stays in registers
            case 0: if (started) fp_mul_lz(acc, acc, tab[0]); else acc = tab[0]; break;
            case 1: if (started) fp_mul_lz(acc, acc, tab[1]); else acc = tab[1]; break;
            case 2: if (started) fp_mul_lz(acc, acc, tab[2]); else acc = tab[2]; break;
            case 3: if (started) fp_mul_lz(acc, acc, tab[3]); else acc = tab[3]; break;
            case 4: if (started) fp_mul_lz(acc, acc, tab[4]); else acc = tab[4]; break;
            case 5: if (started) fp_mul_lz(acc, acc, tab[5]); else acc = tab[5]; break;
            case 6: if (started) fp_mul_lz(acc, acc, tab[6]); else acc = tab[6]; break;
            default: if (started) fp_mul_lz(acc, acc, tab[7]); else acc = tab[7]; break;
        }
        started = true;
        i -= l;
    }
    Fp s, chk; fp_canon64(s, acc); fp_sqr(chk, s);
    r = s;
    return fp_eq(chk, a);
}
// ZCash sign bit: canonical value > (p-1)/2
KZG_HD bool fp_is_lex_largest(const Fp &a) {
    const uint32_t half[NFP] = FP_HALF_INIT;
    uint32_t v[NFP], t[NFP];
    fp_from_mont(v, a);
    return ul_sub<NFP>(t, half, v) != 0;    // half - v borrows  <=>  v > half
}
// 48 big-endian bytes -> Fp.  Returns false if the integer is >= p.  mask_top3 clears the 3 flag bits.
KZG_HD bool fp_from_be48(Fp &r, const uint8_t *in, bool mask_top3) {
    KZG_FP_CONSTS
    uint32_t w[12], v[NFP], t[NFP];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint8_t *p = in + 4 * (11 - i);
        w[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    if (mask_top3) w[11] &= 0x1fffffffu;
    words_to_limbs<NFP, 12>(v, w);
    bool ok = ul_sub<NFP>(t, v, FP_MOD) != 0;     // v < p
    fp_to_mont(r, v);
    return ok;
}
KZG_HD void fp_to_be48(uint8_t *out, const Fp &a) {
    uint32_t v[NFP], w[12];
    fp_from_mont(v, a);
    limbs_to_words<NFP, 12>(w, v);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        uint8_t *p = out + 4 * (11 - i);
        p[0] = (uint8_t)(w[i] >> 24); p[1] = (uint8_t)(w[i] >> 16); p[2] = (uint8_t)(w[i] >> 8); p[3] = (uint8_t)w[i];
    }
}

// ---------------------------------------------------------------------------------- Fr
#define KZG_FR_CONSTS const uint32_t FR_MOD[NFR] = FR_MOD_INIT;
KZG_HD Fr fr_zero() { Fr r; for (int i = 0; i < NFR; i++) r.l[i] = 0; return r; }
KZG_HD Fr fr_one() { const uint32_t c[NFR] = FR_ONE_INIT; Fr r; for (int i = 0; i < NFR; i++) r.l[i] = c[i]; return r; }
KZG_HD void fr_add(Fr &r, const Fr &a, const Fr &b) { KZG_FR_CONSTS mod_add<NFR>(r.l, a.l, b.l, FR_MOD); }
KZG_HD void fr_sub(Fr &r, const Fr &a, const Fr &b) { KZG_FR_CONSTS mod_sub<NFR>(r.l, a.l, b.l, FR_MOD); }
KZG_HD void fr_mul(Fr &r, const Fr &a, const Fr &b) { KZG_FR_CONSTS mont_mul<NFR>(r.l, a.l, b.l, FR_MOD, FR_INVW); }
// (a squaring of its own like Fp's: 45 + 81 limb products instead of 162 -- the twelve z powers per blob of the challenge kernel, the r-power ladders)
KZG_HD void fr_sqr(Fr &r, const Fr &a) { KZG_FR_CONSTS mont_sqr<NFR>(r.l, a.l, FR_MOD, FR_INVW); }
// lazy product: operands < ~2.6 r, result < 1.1 r, not canonical (see mont_mul_lazy)
// (a translation unit that defines KZG_MONT_COLS_FR before this header takes the two lazy Fr products in their column forms: same limbs out)
#if defined(KZG_MONT_COLS_FR)
constexpr bool FR_LAZY_COLS = true;
#else
constexpr bool FR_LAZY_COLS = false;
#endif
KZG_HD void fr_mul_lazy(Fr &r, const Fr &a, const Fr &b) {
    KZG_FR_CONSTS
    if (FR_LAZY_COLS) mont_mul_lazy_cols<NFR, true>(r.l, a.l, b.l, FR_MOD, FR_INVW); else mont_mul_lazy<NFR>(r.l, a.l, b.l, FR_MOD, FR_INVW);
}
// r = a*b + c*d with one reduction (lazy; result < 1.1 r for a*b + c*d < ~5 r^2)
KZG_HD void fr_mul2_lazy(Fr &r, const Fr &a, const Fr &b, const Fr &c, const Fr &d) {
    KZG_FR_CONSTS
    if (FR_LAZY_COLS) mont_mul2_lazy_cols<NFR, true>(r.l, a.l, b.l, c.l, d.l, FR_MOD, FR_INVW);
    else mont_mul2_lazy<NFR>(r.l, a.l, b.l, c.l, d.l, FR_MOD, FR_INVW);
}
// lazy sum: plain limb addition with carry normalisation, no reduction (value grows; keep chains short)
KZG_HD void fr_add_lazy(Fr &r, const Fr &a, const Fr &b) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < NFR; i++) { uint32_t t = a.l[i] + b.l[i] + c; c = i < NFR - 1 ? t >> LB : 0u; r.l[i] = i < NFR - 1 ? (t & LMASK) : t; }
}
KZG_HD bool fr_is_zero(const Fr &a) { return ul_is_zero<NFR>(a.l); }
KZG_HD bool fr_eq(const Fr &a, const Fr &b) { return ul_eq<NFR>(a.l, b.l); }
KZG_HD void fr_select(Fr &r, bool take_b, const Fr &a, const Fr &b) {
#pragma unroll
    for (int i = 0; i < NFR; i++) r.l[i] = take_b ? b.l[i] : a.l[i];
}
// canonical integer as 8 plain 32-bit words
KZG_HD void fr_to_words(uint32_t w[8], const Fr &a) {
    KZG_FR_CONSTS
    uint32_t one[NFR], v[NFR];
#pragma unroll
    for (int i = 0; i < NFR; i++) one[i] = i == 0 ? 1u : 0u;
    mont_mul<NFR>(v, a.l, one, FR_MOD, FR_INVW);
    limbs_to_words<NFR, 8>(w, v);
}
// any 256-bit integer (8 words) -> Montgomery residue mod r.  The product by R^2 reduces it:
// v < 2^256 < 2^261 and R2 < r  =>  v*R2 < r*2^261, within mont_mul's contract.
// (hash_to_bls_field, utils.rs:250-258, relies on exactly this reduction in blst_fr_from_scalar.)
KZG_HD void fr_from_words(Fr &r, const uint32_t w[8]) {
    KZG_FR_CONSTS
    const uint32_t R2[NFR] = FR_R2_INIT;
    uint32_t v[NFR];
    words_to_limbs<NFR, 8>(v, w);
    mont_mul<NFR>(r.l, v, R2, FR_MOD, FR_INVW);
}
// value (8 words) < r ?
KZG_HD bool fr_words_canonical(const uint32_t w[8]) {
    KZG_FR_CONSTS
    uint32_t v[NFR], t[NFR];
    words_to_limbs<NFR, 8>(v, w);
    return ul_sub<NFR>(t, v, FR_MOD) != 0;
}
KZG_HD void fr_inv_fermat(Fr &r, const Fr &a) {
    const uint32_t e[8] = FR_EXP_INV_INIT;
    Fr acc = a;   // bit 254 of r-2 is set
    for (int i = 253; i >= 0; i--) {
        fr_sqr(acc, acc);
        if ((e[i >> 5] >> (i & 31)) & 1) fr_mul(acc, acc, a);
    }
    r = acc;
}
// 32 big-endian bytes <-> 8 little-endian words
KZG_HD void be32_to_words(uint32_t w[8], const uint8_t *in) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t *p = in + 4 * (7 - i);
        w[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
}
KZG_HD void words_to_be32(uint8_t *out, const uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint8_t *p = out + 4 * (7 - i);
        p[0] = (uint8_t)(w[i] >> 24); p[1] = (uint8_t)(w[i] >> 16); p[2] = (uint8_t)(w[i] >> 8); p[3] = (uint8_t)w[i];
    }
}
// bytes_to_bls_field (utils.rs:262-275): false if the value is >= r
KZG_HD bool fr_from_be32_checked(Fr &r, const uint8_t *in) {
    uint32_t w[8]; be32_to_words(w, in);
    bool ok = fr_words_canonical(w);
    fr_from_words(r, w);
    return ok;
}
KZG_HD void fr_to_be32(uint8_t *out, const Fr &a) { uint32_t w[8]; fr_to_words(w, a); words_to_be32(out, w); }

}  // namespace kzg

#include "modinv.h"   // fp_inv / fr_inv: batched-divstep inversion (defined after the arithmetic it builds on)
