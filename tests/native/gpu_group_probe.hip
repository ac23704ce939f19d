// GPU unit test of the layers ABOVE the field arithmetic under kzg_rust_amd/csrc -- g1.h, tower.h, pairing.h, pairing_coop.h, pairing_lanes.h --
// compiled for gfx950 and run routine by routine, so that tests/test_gpu_group_ops.py can compare the DEVICE results with Python big integers
// (oracle/pyref.py).  The host build of the same headers is tests/native/hd_probe.cpp; what differs on the device is what this file is for: COOP_LANES /
// COOP_SYNC are one real lane and a wave fence over LDS, coop_combine_all passes its carry by a DPP row shift, L12_LANES are twelve real lanes per check
// and five checks per wave, g1_mul128_w4 shares one [entry][word][lane] table among the 64 lanes of a wave, and the mid-level routines are device calls.
// Test infrastructure only: never part of libkzg355.so.
//
// Macros: one translation unit can hold ONE inlining policy, and this one takes the set that k_pairing.hip (the cooperative and twelve-lane pairing),
// k_setup.hip (the lane routines of tower.h / pairing.h) and k_verify.hip / k_small.hip (g1.h) are compiled with:
//     KZG_FP_MUL_NOINLINE defined;  KZG_MID_INLINE NOT defined (KZG_MID / KZG_G1_MID routines are noinline device calls);
//     KZG_G1_ADD_MUL2 NOT defined: g1x_add_mixed_lazy in the form of the batch linear combination's bucket kernel (k_g1.hip) -- the host probe
//     holds the other form, the fixed-base MSM's.
// Not reproduced: k_g1.hip's KZG_MID_INLINE (the same source with the group formulas force-inlined) and the Makefile's scheduler flag on k_pairing.hip
// (-mllvm -amdgpu-sched-strategy=max-ilp): the probe is built with the flags of gpu_probe.hip.
//
// C ABI as gpu_probe.hip: byte buffers in, byte buffers plus an int rc[] out, 0 / negative return for the HIP status.
#define KZG_FP_MUL_NOINLINE 1
#include <hip/hip_runtime.h>
#include "../../kzg_rust_amd/csrc/field.h"
#include "../../kzg_rust_amd/csrc/tower.h"
#include "../../kzg_rust_amd/csrc/g1.h"
#include "../../kzg_rust_amd/csrc/pairing.h"
#include "../../kzg_rust_amd/csrc/pairing_coop.h"
#include "../../kzg_rust_amd/csrc/pairing_lanes.h"
#include <vector>
using namespace kzg;

// ------------------------------------------------------------------------------------------------ G1, one operand per lane
// (x, y, 1) -> (x l^2, y l^3, l): a Jacobian operand with a non-trivial z, as hd_g1_add_jac makes it (a: l = 3, b: l = 5)
__device__ static void lift_jac(G1Jac &r, const G1Affine &p, int l) {
    g1_from_affine(r, p);
    if (g1_is_inf(r)) return;
    Fp z = fp_one(), z2, z3;
    for (int k = 1; k < l; k++) fp_add(z, z, fp_one());
    fp_sqr(z2, z); fp_mul(z3, z2, z); fp_mul(r.x, r.x, z2); fp_mul(r.y, r.y, z3); r.z = z;
}
// the same for the extended-Jacobian form: (x l^2, y l^3, l^2, l^3)
__device__ static void lift_xyzz(G1X &r, const G1Affine &p, int l) {
    if (g1a_is_inf(p)) { r = g1x_inf(); return; }
    Fp z = fp_one(), z2, z3;
    for (int k = 1; k < l; k++) fp_add(z, z, fp_one());
    fp_sqr(z2, z); fp_mul(z3, z2, z); fp_mul(r.x, p.x, z2); fp_mul(r.y, p.y, z3); r.zz = z2; r.zzz = z3;
}
enum { G1_VALIDATE = 0, G1_ADD, G1_ADD_MIXED, G1_DBL, G1X_ADD_MIXED, G1X_ADD_MIXED_LAZY, G1X_ADD_LAZY2, G1_DBL_LAZY, G1_ADD_LAZY, G1_ADD_LAZY2, G1_MUL_WORDS,
       G1_GLV_SPLITS, G1_GLV_MUL, G1_MUL128_W4, G1_PAIRPT, G1_N_OPS };
constexpr int G1_OUT_STRIDE = 64;                     // 48 bytes of a compressed point, or the 64 of the two GLV splits
// a, b: 48-byte compressed points; k: 32-byte big-endian scalars; pre: the count of lazy steps in front of the routine under test (each operation
// says below what it computes with it), the subgroup switch of G1_VALIDATE, the sign of G1_PAIRPT.  rc: G1_VALIDATE as hd_g1_validate (0 ok, 1 bad
// encoding, 2 not on the curve, 3 outside the subgroup, 99 the two subgroup tests disagree); the others 0, or 1 for an operand that does not decode.
// tab: one g1_mul128_w4 table per workgroup.
template <int OP> __global__ void __launch_bounds__(64) k_g1_op(int n, const uint8_t *a, const uint8_t *b, const uint8_t *k, int pre, uint8_t *out, int *rc,
        uint32_t *tab) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint8_t *o = out + (size_t)G1_OUT_STRIDE * i;
    uint32_t kw[8];
    be32_to_words(kw, k + 32 * (size_t)i);
    if constexpr (OP == G1_GLV_SPLITS) {              // a (16 bytes, little-endian words) | b | a_fast | b_fast
        uint32_t s[16];
        glv_split(s, s + 4, kw);
        glv_split_fast(s + 8, s + 12, kw);
        for (int w = 0; w < 16; w++) for (int j = 0; j < 4; j++) o[4 * w + j] = (uint8_t)(s[w] >> (8 * j));
        rc[i] = 0;
        return;
    }
    G1Affine pa, pb, ra;
    int code = g1_decompress(pa, a + 48 * (size_t)i);
    if constexpr (OP == G1_VALIDATE) {
        if (code == 0 && pre && !g1a_is_inf(pa)) {
            const bool s = g1_in_subgroup(pa), t = g1_in_subgroup_naive(pa);
            code = s != t ? 99 : s ? 0 : 3;
        }
        rc[i] = code;
        if (code == 0) g1_compress_affine(o, pa);
        return;
    }
    if (code || g1_decompress(pb, b + 48 * (size_t)i)) { rc[i] = 1; return; }
    G1Jac r = g1_inf();
    if constexpr (OP == G1_ADD) { G1Jac x, y; lift_jac(x, pa, 3); lift_jac(y, pb, 5); g1_add(r, x, y); }
    if constexpr (OP == G1_ADD_MIXED) { G1Jac x; lift_jac(x, pa, 3); g1_add_mixed(r, x, pb); }
    if constexpr (OP == G1_DBL) { G1Jac x; lift_jac(x, pa, 3); g1_dbl(r, x); }
    if constexpr (OP == G1X_ADD_MIXED) { G1X x; lift_xyzz(x, pa, 3); g1x_add_mixed(x, x, pb); g1x_to_jac(r, x); }
    if constexpr (OP == G1X_ADD_MIXED_LAZY) {         // a + (pre + 1) b: the accumulator started with a, then b added pre + 1 times
        G1X acc = g1x_inf(), c; bool started = false;
        g1x_add_mixed_lazy(acc, started, pa);
        for (int s = 0; s <= pre; s++) g1x_add_mixed_lazy(acc, started, pb);
        g1x_from_lazy(c, acc, started); g1x_to_jac(r, c);
    }
    if constexpr (OP == G1X_ADD_LAZY2) {              // (a + pre b) + (b + pre a), both operands raw lazy accumulators as the bucket kernel parks them
        G1X x = g1x_inf(), y = g1x_inf(), s, c; bool sx = false, sy = false;
        g1x_add_mixed_lazy(x, sx, pa); for (int t = 0; t < pre; t++) g1x_add_mixed_lazy(x, sx, pb);
        g1x_add_mixed_lazy(y, sy, pb); for (int t = 0; t < pre; t++) g1x_add_mixed_lazy(y, sy, pa);
        if (!sx) x = g1x_inf();
        if (!sy) y = g1x_inf();
        g1x_add_lazy2(s, x, y);
        g1x_from_lazy(c, s, true); g1x_to_jac(r, c);
    }
    if constexpr (OP == G1_DBL_LAZY) {                // [2^(pre + 1)] a
        G1Jac x; lift_jac(x, pa, 3);
        for (int s = 0; s <= pre; s++) g1_dbl_lazy(x, x);
        g1_canon_lazy(r, x);
    }
    if constexpr (OP == G1_ADD_LAZY) {                // [2^pre] a + b, b canonical
        G1Jac x, y; lift_jac(x, pa, 3); lift_jac(y, pb, 5);
        for (int s = 0; s < pre; s++) g1_dbl_lazy(x, x);
        g1_add_lazy(x, x, y);
        g1_canon_lazy(r, x);
    }
    if constexpr (OP == G1_ADD_LAZY2) {               // pre = 0: a + b; else [2^pre] a + [2^pre + 1] b, the second operand as a lazy addition leaves it
        G1Jac x, y; lift_jac(x, pa, 3); lift_jac(y, pb, 5);
        if (pre > 0) {
            G1Jac t = y;
            for (int s = 0; s < pre; s++) { g1_dbl_lazy(x, x); g1_dbl_lazy(t, t); }
            g1_add_lazy(y, t, y);
        }
        g1_add_lazy2(x, x, y);
        g1_canon_lazy(r, x);
    }
    if constexpr (OP == G1_MUL_WORDS) g1_mul_words(r, pa, kw, 8);
    if constexpr (OP == G1_GLV_MUL) {                 // as hd_glv_mul: [k mod x^2] P + [k div x^2] (-phi P)
        uint32_t s[4], t[4]; G1Affine qa; G1Jac r2;
        glv_split(s, t, kw);
        g1a_neg_phi(qa, pa);
        g1_mul_words(r, pa, s, 4); g1_mul_words(r2, qa, t, 4);
        g1_add(r, r, r2);
    }
    if constexpr (OP == G1_MUL128_W4)                 // the low 128 bits of k; the table of this workgroup, one column per lane
        g1_mul128_w4(r, pa, kw, tab + (size_t)blockIdx.x * (W4_ENTRIES * 3 * NFP * 64), (int)threadIdx.x);
    if constexpr (OP == G1_PAIRPT) {
        G1Jac x; lift_jac(x, pa, 3);
        PairPt pp; pairpt_from_jac(pp, x, (pre & 1) != 0);
        pairpt_to_affine(ra, pp);
    } else g1_to_affine(ra, r);
    g1_compress_affine(o, ra);
    rc[i] = 0;
}

// ------------------------------------------------------------------------------------------------ Fp12 in the w basis
// An element crosses the ABI as twelve canonical 48-byte coefficients of w^0 .. w^11 plus, per coefficient, a multiple of p to add before the call.
__device__ static void add_kp(Fp &r, uint32_t k) {    // r + k p, limbs normalised below the top one
    const uint32_t pm[NFP] = FP_MOD_INIT;
    uint64_t c = 0;
    for (int i = 0; i < NFP; i++) {
        const uint64_t t = (uint64_t)r.l[i] + (uint64_t)k * pm[i] + c;
        if (i < NFP - 1) { r.l[i] = (uint32_t)t & LMASK; c = t >> LB; } else r.l[i] = (uint32_t)t;
    }
}
__device__ static void load_coeff(Fp &r, const uint8_t *v, const uint8_t *kp, size_t e, int k) {
    fp_from_be48(r, v + 48 * (12 * e + k), false);
    add_kp(r, kp[12 * e + k]);
}
__device__ static void store_coeff(uint8_t *out, size_t e, int k, const Fp &v) {
    Fp c; fp_norm_lz(c, v); fp_canon64(c, c);
    fp_to_be48(out + 48 * (12 * e + k), c);
}
enum { CO_MUL = 0, CO_SQR, CO_LINE_W, CO_LINE_BS, CO_CYC_SQR, CO_CONJ, CO_FROB, CO_FROB2, CO_FP6INV, CO_IS_ONE, CO_N_OPS };
// one wave per element, CoopMem in LDS as k_pairing_coop holds it.  rc: 0, CO_IS_ONE: 100 / 101
template <int OP> __global__ void __launch_bounds__(64) k_coop_op(int n, const uint8_t *a, const uint8_t *ka, const uint8_t *b, const uint8_t *kb,
        uint8_t *out, int *rc, const CoopScheds *scheds, const FrobTables *frob) {
    __shared__ CoopMem mem;
    const size_t e = blockIdx.x;
    if ((int)e >= n) return;
    PairPt none; none.ax = fp_zero(); none.ay = fp_zero(); none.az = fp_zero();
    coop_init(mem, scheds, none, none);
    COOP_LANES(lane) { if (lane < 12) { load_coeff(mem.t1.c[lane], a, ka, e, lane); load_coeff(mem.t2.c[lane], b, kb, e, lane); } }
    COOP_SYNC();
    const Fp12W *res = &mem.t0;
    int code = 0;
    if constexpr (OP == CO_MUL) coop_mul(mem, mem.t0, mem.t1, mem.t2, FULL_MASK);
    if constexpr (OP == CO_SQR) coop_sqr(mem, mem.t0, mem.t1);
    if constexpr (OP == CO_LINE_W) coop_product(mem, mem.sc.line, mem.t0, mem.t1, mem.t2, LINE_MASK);
    if constexpr (OP == CO_LINE_BS) {                 // the line as l0, l6, l2, l8, l3, l9 in a row (coop_eval_lines_item's layout); the slot operand unused
        COOP_LANES(lane) { if (lane < 6) { const int j = 2 * (lane >> 1) + 6 * (lane & 1) - (lane >= 4 ? 1 : 0); mem.t3.c[lane] = mem.t2.c[j]; } }
        COOP_SYNC();
        coop_product(mem, mem.sc.line, mem.t0, mem.t1, mem.t4, LINE_MASK, mem.t3.c);
    }
    if constexpr (OP == CO_CYC_SQR) coop_cyc_sqr(mem, mem.t0, mem.t1);
    if constexpr (OP == CO_CONJ) coop_conj(mem.t0, mem.t1);
    if constexpr (OP == CO_FROB) coop_frob(mem.t0, mem.t1, frob->a1, frob->b1);
    if constexpr (OP == CO_FROB2) coop_frob2(mem.t0, mem.t1, frob->a2);
    if constexpr (OP == CO_FP6INV) { coop_fp6_inv(mem, mem.t1, mem.t2.c); res = &mem.t1; }      // in place; t2, t3: the 24 scratch values
    if constexpr (OP == CO_IS_ONE) { code = coop_is_one(mem, mem.t1) ? 101 : 100; res = &mem.t1; }
    COOP_LANES(lane) {
        if (lane < 12) store_coeff(out, e, lane, res->c[lane]);
        if (lane == 0) rc[e] = code;
    }
}
enum { L12_CYC_SQR = 0, L12_MULF, L12_CONJ, L12_FROB, L12_FROB2, L12_IS_ONE, L12_N_OPS };
// five elements per wave, twelve lanes each, as k_pairing_hard12 deals them (a tail group redoes the last element and reports nothing)
template <int OP> __global__ void __launch_bounds__(64) k_l12_op(int n, const uint8_t *a, const uint8_t *ka, const uint8_t *b, const uint8_t *kb,
        uint32_t jmask, uint8_t *out, int *rc, const FrobTables *frob) {
    __shared__ L12Mem mems[L12_BATCHES];
    __shared__ int is_one[L12_BATCHES][12];
    const int grp = (int)threadIdx.x / 12, g = grp < L12_BATCHES ? grp : 0;      // (lanes 60 .. 63 idle: L12_LANES leaves them out)
    const int e_raw = blockIdx.x * L12_BATCHES + grp;
    const size_t e = e_raw < n ? e_raw : n - 1;
    L12Mem &m = mems[g];
    L12_LANES(k) { load_coeff(m.s[1].c[k], a, ka, e, k); load_coeff(m.s[2].c[k], b, kb, e, k); }
    L12_SYNC();
    const Fp12W *res = &m.s[0];
    int code = 0;
    if constexpr (OP == L12_CYC_SQR) l12_cyc_sqr(m.s[0], m.s[1]);
    if constexpr (OP == L12_MULF) l12_mulf(m.s[0], m.s[1], m.s[2], jmask);
    if constexpr (OP == L12_CONJ) l12_conj(m.s[0], m.s[1]);
    if constexpr (OP == L12_FROB) l12_frob(m.s[0], m.s[1], frob->a1, frob->b1);
    if constexpr (OP == L12_FROB2) l12_frob(m.s[0], m.s[1], frob->a2, nullptr);
    if constexpr (OP == L12_IS_ONE) {                 // the twelve answers of a check, combined by its first lane
        L12_LANES(k) { is_one[g][k] = l12_coeff_is_one(m.s[1], k) ? 1 : 0; }
        L12_SYNC();
        code = 101;
        for (int k = 0; k < 12; k++) if (!is_one[g][k]) code = 100;
        res = &m.s[1];
    }
    L12_LANES(k) {
        if (e_raw < n) {
            store_coeff(out, e, k, res->c[k]);
            if (k == 0) rc[e] = code;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the whole pairing check, one wave per check
// ok_coop: the verdict of coop_pairing_check, as hd_pairings_verify_coop calls it.  ok_l12: the verdict with the hard part of the final exponentiation
// through l12_run behind the cooperative Miller loops and easy part, as hd_pairings_verify_lanes12 (all five groups of the wave run the same check).
// rc: 0; 1 a G1 argument does not decode; 4 a coefficient of the twelve-lane result differs from the cooperative run's; 5 the two forms of the
// "== 1" test disagree on the same value.
__global__ void __launch_bounds__(64) k_pairing_check(int n, const uint8_t *p1, const uint8_t *p2, const LineW *lines1, const LineW *lines2, const int *q_inf,
        const CoopInsn *prog, int n_insn, int hard, const CoopScheds *scheds, const FrobTables *frob, int *ok_coop, int *ok_l12, int *rc) {
    __shared__ CoopMem mem;
    __shared__ L12Mem lmems[L12_BATCHES];
    __shared__ int same[L12_BATCHES][12], is_one[L12_BATCHES][12];
    const int grp = (int)threadIdx.x / 12, g = grp < L12_BATCHES ? grp : 0;
    const size_t e = blockIdx.x;
    if ((int)e >= n) return;
    G1Affine a, b;
    if (g1_decompress(a, p1 + 48 * e) || g1_decompress(b, p2 + 48 * e)) { if (threadIdx.x == 0) rc[e] = 1; return; }      // (uniform: every lane decodes the same bytes)
    const LineW *w1 = lines1 + N_LINES * e, *w2 = lines2 + N_LINES * e;
    const bool q1_inf = q_inf[2 * e] != 0, q2_inf = q_inf[2 * e + 1] != 0;
    {
        G1Affine an = a, bn = b;
        if (!g1a_is_inf(a)) g1a_neg(an, a);
        if (q1_inf) an = g1a_inf();
        if (q2_inf) bn = g1a_inf();
        const bool r = coop_pairing_check(mem, prog, n_insn, scheds, w1, an, w2, bn, *frob);
        if (threadIdx.x == 0) ok_coop[e] = r ? 1 : 0;
    }
    PairPt pa, pb; pairpt_from_affine(pa, a); pairpt_from_affine(pb, b);
    { Fp ny; fp_neg(ny, pa.ay); pa.ay = ny; }
    const bool use1 = !fp_is_zero(pa.az) && !q1_inf, use2 = !fp_is_zero(pb.az) && !q2_inf;
    L12Mem &lm = lmems[g];
    coop_init(mem, scheds, pa, pb);
    COOP_LANES(lane) { if (lane < 12 * L12_BATCHES) { same[lane / 12][lane % 12] = 1; is_one[lane / 12][lane % 12] = 1; } }
    coop_run(mem, prog, 0, hard, w1, w2, use1, use2, *frob);
    L12_LANES(k) { Fp c; fp_norm_lz(c, mem.f.c[k]); fp_canon64(c, c); lm.s[S_F].c[k] = c; }      // the hand-over: canonical coefficients
    L12_SYNC();
    l12_run(lm, prog, hard, n_insn, *frob);
    coop_run(mem, prog, hard, n_insn, w1, w2, use1, use2, *frob);
    L12_LANES(k) {
        Fp x, y; fp_norm_lz(x, mem.t0.c[k]); fp_canon64(x, x); fp_norm_lz(y, lm.s[S_T0].c[k]); fp_canon64(y, y);
        same[g][k] = fp_eq(x, y) ? 1 : 0;
        is_one[g][k] = l12_coeff_is_one(lm.s[S_T0], k) ? 1 : 0;
    }
    L12_SYNC();
    const bool coop_one = coop_is_one(mem, mem.t0);
    if (threadIdx.x == 0) {                           // the verdict of the first group; every group's coefficients compared
        bool all_same = true, all_one = true;
        for (int q = 0; q < L12_BATCHES; q++) for (int k = 0; k < 12; k++) all_same = all_same && same[q][k] != 0;
        for (int k = 0; k < 12; k++) all_one = all_one && is_one[0][k] != 0;
        ok_l12[e] = all_one ? 1 : 0; rc[e] = !all_same ? 4 : all_one != coop_one ? 5 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ lane routines of tower.h / pairing.h
// One element per lane.  An element is twelve 48-byte canonical values, the tower coefficients in the order c[i].c[j].c[k] -> 6 i + 2 j + k (an Fp2
// or Fp6 operand fills the first two or six); TW_G2_DECOMPRESS reads the first 96 bytes of a as the encoding and returns x.c0, x.c1, y.c0, y.c1.
// rc: 0; TW_FP2_SQRT 2 no square root; TW_FP2_LEX 100 / 101; TW_G2_DECOMPRESS as g2_decompress.
enum { TW_FP2_MUL = 0, TW_FP2_SQR, TW_FP2_INV, TW_FP2_SQRT, TW_FP2_LEX, TW_FP6_MUL, TW_FP6_INV, TW_FP12_MUL, TW_FP12_SQR, TW_FP12_INV, TW_FP12_FROB,
       TW_FP12_MUL_BY_014, TW_G2_DECOMPRESS, TW_N_OPS };
__device__ static void load_fp12(Fp12 &r, const uint8_t *v, size_t i) {
    Fp *c = &r.c0.c0.c0;                                 // Fp12 is twelve Fp in a row in exactly that order
    for (int k = 0; k < 12; k++) fp_from_be48(c[k], v + 48 * (12 * i + k), false);
}
template <int OP> __global__ void __launch_bounds__(64) k_tower_op(int n, const uint8_t *a, const uint8_t *b, uint8_t *out, int *rc) {
    static_assert(sizeof(Fp12) == 12 * sizeof(Fp), "the coefficients are addressed as an array");
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Fp12 x, y, r;
    Fp *rc12 = &r.c0.c0.c0;
    for (int k = 0; k < 12; k++) rc12[k] = fp_zero();
    int code = 0;
    if constexpr (OP == TW_G2_DECOMPRESS) {
        G2Affine q;
        code = g2_decompress(q, a + 48 * 12 * (size_t)i);
        if (code == 0) { r.c0.c0 = q.x; r.c0.c1 = q.y; }
    } else {
        load_fp12(x, a, i); load_fp12(y, b, i);
    }
    if constexpr (OP == TW_FP2_MUL) fp2_mul(r.c0.c0, x.c0.c0, y.c0.c0);
    if constexpr (OP == TW_FP2_SQR) fp2_sqr(r.c0.c0, x.c0.c0);
    if constexpr (OP == TW_FP2_INV) fp2_inv(r.c0.c0, x.c0.c0);
    if constexpr (OP == TW_FP2_SQRT) { if (!fp2_sqrt(r.c0.c0, x.c0.c0)) code = 2; }
    if constexpr (OP == TW_FP2_LEX) code = fp2_is_lex_largest(x.c0.c0) ? 101 : 100;
    if constexpr (OP == TW_FP6_MUL) fp6_mul(r.c0, x.c0, y.c0);
    if constexpr (OP == TW_FP6_INV) fp6_inv(r.c0, x.c0);
    if constexpr (OP == TW_FP12_MUL) fp12_mul(r, x, y);
    if constexpr (OP == TW_FP12_SQR) fp12_sqr(r, x);
    if constexpr (OP == TW_FP12_INV) fp12_inv(r, x);
    if constexpr (OP == TW_FP12_FROB) fp12_frob(r, x);
    if constexpr (OP == TW_FP12_MUL_BY_014) { r = x; fp12_mul_by_014(r, y.c0.c0, y.c0.c1, y.c0.c2); }      // l0, l1, l4: the first six values of b
    for (int k = 0; k < 12; k++) fp_to_be48(out + 48 * (12 * (size_t)i + k), rc12[k]);
    rc[i] = code;
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
struct DevBufs {                                         // device buffers of one call, freed together
    std::vector<void *> all;
    bool ok = true;
    template <typename T> T *zeroed(size_t count, int fill = 0) {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(T) * (count ? count : 1)) != hipSuccess) { ok = false; return nullptr; }
        all.push_back(p);
        if (hipMemset(p, fill, sizeof(T) * (count ? count : 1)) != hipSuccess) ok = false;
        return static_cast<T *>(p);
    }
    template <typename T> T *upload(const T *h, size_t count) {
        T *p = zeroed<T>(count);
        if (p && count && hipMemcpy(p, h, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return p;
    }
    template <typename T> void download(T *h, const T *d, size_t count) {
        if (count && hipMemcpy(h, d, sizeof(T) * count, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
    }
    ~DevBufs() { for (void *p : all) (void)hipFree(p); }
};
int finish(DevBufs &d) {
    if (hipGetLastError() != hipSuccess) return -3;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    return d.ok ? 0 : -1;
}
FrobTables frob_tables() {
    static const uint32_t A1[12][NFP] = FROBW_A1_INIT, B1[12][NFP] = FROBW_B1_INIT, A2[12][NFP] = FROBW_A2_INIT;
    FrobTables ft;
    for (int k = 0; k < 12; k++) for (int i = 0; i < NFP; i++) { ft.a1[k].l[i] = A1[k][i]; ft.b1[k].l[i] = B1[k][i]; ft.a2[k].l[i] = A2[k][i]; }
    return ft;
}
}  // namespace

#define PROBE_LAUNCH(kernel, OPV, grid, ...) case OPV: hipLaunchKernelGGL((kernel<OPV>), grid, dim3(64), 0, 0, __VA_ARGS__); break;

extern "C" {
// out: 64 bytes per operand (G1_OUT_STRIDE), the compressed point in the first 48
int gpu_g1_ops(int op, int n, const uint8_t *a, const uint8_t *b, const uint8_t *k, int pre, uint8_t *out, int *rc) {
    if (n <= 0 || op < 0 || op >= G1_N_OPS || pre < 0 || pre > 64) return -4;
    DevBufs d;
    const int blocks = (n + 63) / 64;
    uint8_t *da = d.upload(a, 48 * (size_t)n), *db = d.upload(b, 48 * (size_t)n), *dk = d.upload(k, 32 * (size_t)n);
    uint8_t *dout = d.zeroed<uint8_t>(G1_OUT_STRIDE * (size_t)n);
    int *drc = d.zeroed<int>(n, 0xff);
    uint32_t *tab = d.zeroed<uint32_t>(op == G1_MUL128_W4 ? (size_t)blocks * W4_ENTRIES * 3 * NFP * 64 : 1);
    if (!d.ok) return -1;
    const dim3 grid(blocks);
    switch (op) {
        PROBE_LAUNCH(k_g1_op, G1_VALIDATE, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_ADD, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_ADD_MIXED, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_DBL, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1X_ADD_MIXED, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1X_ADD_MIXED_LAZY, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1X_ADD_LAZY2, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_DBL_LAZY, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_ADD_LAZY, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_ADD_LAZY2, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_MUL_WORDS, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_GLV_SPLITS, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_GLV_MUL, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_MUL128_W4, grid, n, da, db, dk, pre, dout, drc, tab)
        PROBE_LAUNCH(k_g1_op, G1_PAIRPT, grid, n, da, db, dk, pre, dout, drc, tab)
        default: return -4;
    }
    const int st = finish(d);
    d.download(out, dout, G1_OUT_STRIDE * (size_t)n); d.download(rc, drc, n);
    return st ? st : d.ok ? 0 : -1;
}
// a, b: n x 12 x 48 bytes; ka, kb: n x 12 multiples of p (at most 31)
int gpu_coop_ops(int op, int n, const uint8_t *a, const uint8_t *ka, const uint8_t *b, const uint8_t *kb, uint8_t *out, int *rc) {
    if (n <= 0 || op < 0 || op >= CO_N_OPS) return -4;
    for (size_t i = 0; i < 12 * (size_t)n; i++) if (ka[i] > 31 || kb[i] > 31) return -4;
    static CoopScheds sc;
    if (!build_coop_schedules(sc)) return -5;
    const FrobTables ft = frob_tables();
    DevBufs d;
    uint8_t *da = d.upload(a, 576 * (size_t)n), *db = d.upload(b, 576 * (size_t)n), *dka = d.upload(ka, 12 * (size_t)n), *dkb = d.upload(kb, 12 * (size_t)n);
    uint8_t *dout = d.zeroed<uint8_t>(576 * (size_t)n);
    int *drc = d.zeroed<int>(n, 0xff);
    const CoopScheds *dsc = d.upload(&sc, 1);
    const FrobTables *dft = d.upload(&ft, 1);
    if (!d.ok) return -1;
    const dim3 grid(n);
    switch (op) {
        PROBE_LAUNCH(k_coop_op, CO_MUL, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_SQR, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_LINE_W, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_LINE_BS, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_CYC_SQR, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_CONJ, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_FROB, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_FROB2, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_FP6INV, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        PROBE_LAUNCH(k_coop_op, CO_IS_ONE, grid, n, da, dka, db, dkb, dout, drc, dsc, dft)
        default: return -4;
    }
    const int st = finish(d);
    d.download(out, dout, 576 * (size_t)n); d.download(rc, drc, n);
    return st ? st : d.ok ? 0 : -1;
}
// the same ABI, five elements per wave; the multiples of p are at most 1 here; jmask: the coefficients of b that L12_MULF reads
int gpu_l12_ops(int op, int n, const uint8_t *a, const uint8_t *ka, const uint8_t *b, const uint8_t *kb, uint32_t jmask, uint8_t *out, int *rc) {
    if (n <= 0 || op < 0 || op >= L12_N_OPS || (jmask & ~FULL_MASK)) return -4;
    for (size_t i = 0; i < 12 * (size_t)n; i++) if (ka[i] > 1 || kb[i] > 1) return -4;
    const FrobTables ft = frob_tables();
    DevBufs d;
    uint8_t *da = d.upload(a, 576 * (size_t)n), *db = d.upload(b, 576 * (size_t)n), *dka = d.upload(ka, 12 * (size_t)n), *dkb = d.upload(kb, 12 * (size_t)n);
    uint8_t *dout = d.zeroed<uint8_t>(576 * (size_t)n);
    int *drc = d.zeroed<int>(n, 0xff);
    const FrobTables *dft = d.upload(&ft, 1);
    if (!d.ok) return -1;
    const dim3 grid((n + L12_BATCHES - 1) / L12_BATCHES);
    switch (op) {
        PROBE_LAUNCH(k_l12_op, L12_CYC_SQR, grid, n, da, dka, db, dkb, jmask, dout, drc, dft)
        PROBE_LAUNCH(k_l12_op, L12_MULF, grid, n, da, dka, db, dkb, jmask, dout, drc, dft)
        PROBE_LAUNCH(k_l12_op, L12_CONJ, grid, n, da, dka, db, dkb, jmask, dout, drc, dft)
        PROBE_LAUNCH(k_l12_op, L12_FROB, grid, n, da, dka, db, dkb, jmask, dout, drc, dft)
        PROBE_LAUNCH(k_l12_op, L12_FROB2, grid, n, da, dka, db, dkb, jmask, dout, drc, dft)
        PROBE_LAUNCH(k_l12_op, L12_IS_ONE, grid, n, da, dka, db, dkb, jmask, dout, drc, dft)
        default: return -4;
    }
    const int st = finish(d);
    d.download(out, dout, 576 * (size_t)n); d.download(rc, drc, n);
    return st ? st : d.ok ? 0 : -1;
}
// a, b, out: n x 12 x 48 bytes
int gpu_tower_ops(int op, int n, const uint8_t *a, const uint8_t *b, uint8_t *out, int *rc) {
    if (n <= 0 || op < 0 || op >= TW_N_OPS) return -4;
    DevBufs d;
    uint8_t *da = d.upload(a, 576 * (size_t)n), *db = d.upload(b, 576 * (size_t)n);
    uint8_t *dout = d.zeroed<uint8_t>(576 * (size_t)n);
    int *drc = d.zeroed<int>(n, 0xff);
    if (!d.ok) return -1;
    const dim3 grid((n + 63) / 64);
    switch (op) {
        PROBE_LAUNCH(k_tower_op, TW_FP2_MUL, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP2_SQR, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP2_INV, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP2_SQRT, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP2_LEX, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP6_MUL, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP6_INV, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP12_MUL, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP12_SQR, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP12_INV, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP12_FROB, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_FP12_MUL_BY_014, grid, n, da, db, dout, drc)
        PROBE_LAUNCH(k_tower_op, TW_G2_DECOMPRESS, grid, n, da, db, dout, drc)
        default: return -4;
    }
    const int st = finish(d);
    d.download(out, dout, 576 * (size_t)n); d.download(rc, drc, n);
    return st ? st : d.ok ? 0 : -1;
}
// e(p1[i], q1[i]) == e(p2[i], q2[i]) for n checks: 48-byte G1 and 96-byte G2 encodings.  The lines of the G2 arguments, the pairing program and the
// schedules are built here on the host with the headers' own builders, as hd_probe.cpp does.  6: a G2 argument does not decode.
int gpu_pairing_checks(int n, const uint8_t *p1, const uint8_t *q1, const uint8_t *p2, const uint8_t *q2, int *ok_coop, int *ok_l12, int *rc) {
    if (n <= 0 || n > 64) return -4;
    std::vector<LineW> w1((size_t)n * N_LINES), w2((size_t)n * N_LINES);
    std::vector<int> q_inf(2 * (size_t)n);
    std::vector<LineCoeff> l(N_LINES);
    for (int i = 0; i < n; i++)
        for (int s = 0; s < 2; s++) {
            G2Affine q;
            if (g2_decompress(q, (s ? q2 : q1) + 96 * (size_t)i)) return 6;
            q_inf[2 * i + s] = g2a_is_inf(q) ? 1 : 0;
            LineW *w = (s ? w2 : w1).data() + (size_t)i * N_LINES;
            if (q_inf[2 * i + s]) { for (int j = 0; j < N_LINES; j++) { LineW z; z.l0 = z.l6 = z.l2 = z.l8 = z.l3 = z.l9 = fp_zero(); w[j] = z; } continue; }
            precompute_lines(l.data(), q);
            for (int j = 0; j < N_LINES; j++) line_to_w(w[j], l[j]);
        }
    static CoopInsn prog[COOP_PROGRAM_MAX];
    int hard = 0;
    const int n_insn = build_pairing_program(prog, &hard);
    static CoopScheds sc;
    if (n_insn > COOP_PROGRAM_MAX || !build_coop_schedules(sc) || hard <= 0 || hard >= n_insn) return -5;
    const FrobTables ft = frob_tables();
    DevBufs d;
    uint8_t *dp1 = d.upload(p1, 48 * (size_t)n), *dp2 = d.upload(p2, 48 * (size_t)n);
    const LineW *dw1 = d.upload(w1.data(), w1.size()), *dw2 = d.upload(w2.data(), w2.size());
    const int *dinf = d.upload(q_inf.data(), q_inf.size());
    const CoopInsn *dprog = d.upload(prog, (size_t)n_insn);
    const CoopScheds *dsc = d.upload(&sc, 1);
    const FrobTables *dft = d.upload(&ft, 1);
    int *dok1 = d.zeroed<int>(n, 0xff), *dok2 = d.zeroed<int>(n, 0xff), *drc = d.zeroed<int>(n, 0xff);
    if (!d.ok) return -1;
    hipLaunchKernelGGL(k_pairing_check, dim3(n), dim3(64), 0, 0, n, dp1, dp2, dw1, dw2, dinf, dprog, n_insn, hard, dsc, dft, dok1, dok2, drc);
    const int st = finish(d);
    d.download(ok_coop, dok1, n); d.download(ok_l12, dok2, n); d.download(rc, drc, n);
    return st ? st : d.ok ? 0 : -1;
}
}
