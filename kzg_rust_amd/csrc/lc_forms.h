// lc_forms.h -- the shapes the bucket form of the batch linear combination runs at (k_g1.hip): how a term's scalar is cut, how wide a window is,
// and which (window, class, part of the buckets) tasks each of the bucket kernel's four waves takes.  Host+device, so that the recoding and the
// dealing are checked on the CPU (tests/native/lc_forms_probe.cpp).
//   LcHalves    today's GLV form: two 128-bit halves per term, 25 signed 5-bit digits and a top digit
//   LcQuarters  four 64-bit quarters per term (quarter_split, g1.h: it needs Q = [|x|]P, which the subgroup test leaves), 10 signed 6-bit digits
//               and a top digit: half the windows, so the window can grow by a bit without growing the tail
#pragma once
#include "g1.h"

namespace kzg {

constexpr int LC_TB = 16;                        // buckets of one task: a task is (window, class, part) with part < NB / 16
constexpr int LC_MAXT = 13;                      // tasks one wave may be dealt (16 x 13 = 208 lists <= 255: the list ranks are uint8_t)

template <int BITS_, int PER_TERM_> struct LcCfg {
    static constexpr int BITS = BITS_, PER_TERM = PER_TERM_;
    static constexpr int SCALAR_BITS = 256 / PER_TERM;                       // 128 or 64: what one item's scalar may fill
    static constexpr int WINDOWS = (SCALAR_BITS - 1) / BITS + 1;             // signed digits below, one unsigned top digit (halves: 26; quarters: 11 at 6 bits)
    static constexpr int NB = 1 << (BITS - 1);                               // |digit| in 1 .. NB
    static constexpr int PARTS = NB / LC_TB;
    static constexpr int DIG_STRIDE = PER_TERM == 2 ? 28 : 16;               // bytes of digits per item
    static_assert(NB % LC_TB == 0 && WINDOWS <= DIG_STRIDE && WINDOWS < 32, "task words hold the window in 5 bits");
    // the top digit takes the bits from BITS (WINDOWS - 1) up and the carry of the bias: it must fit the BITS-bit mask of the recoding
    static_assert(SCALAR_BITS + 1 - BITS * (WINDOWS - 1) <= BITS, "top digit");
    static_assert(4 * LC_MAXT >= 2 * WINDOWS * PARTS, "four waves hold every task");
};
using LcHalves = LcCfg<5, 2>;
#if !defined(KZG_LC_QUARTER_BITS)
#define KZG_LC_QUARTER_BITS 6
#endif
using LcQuarters = LcCfg<KZG_LC_QUARTER_BITS, 4>;

template <class CFG> KZG_HD int lc_items_of(int n) { return CFG::PER_TERM * (3 * n + 1); }
// items of a class per window: class 0 is the terms t < n, class 1 the other 2n + 1
template <class CFG> KZG_HD int lc_class_items(int cls, int n) { return CFG::PER_TERM * (cls ? 2 * n + 1 : n); }
// item indices travel as uint16_t with the sign of the digit in bit 15
template <class CFG> KZG_HD bool lc_items_fit(int n) { return n >= 8 && lc_items_of<CFG>(n) <= 0x7fff; }       // halves: n <= 5461; quarters: n <= 2730

// k = sum_w d_w 2^(BITS w) with d_w = chunk_w(k + BIAS) - NB for w < WINDOWS - 1 and d_top = the remaining top bits (unsigned): BIAS has the top
// bit of every chunk below the top one set.  v: SCALAR_BITS / 32 words.
template <class CFG> constexpr KZG_HD uint32_t lc_bias_word(int i) {
    uint32_t r = 0;
    for (int w = 0; w < CFG::WINDOWS - 1; w++) { const int bit = CFG::BITS * w + CFG::BITS - 1; if ((bit >> 5) == i) r |= 1u << (bit & 31); }
    return r;
}
template <class CFG> KZG_HD void lc_recode(int8_t *d, const uint32_t *v) {
    constexpr int NW = CFG::SCALAR_BITS / 32;
    uint32_t e[NW + 2]; uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) { c += (uint64_t)v[i] + lc_bias_word<CFG>(i); e[i] = (uint32_t)c; c >>= 32; }
    e[NW] = (uint32_t)c; e[NW + 1] = 0;
    for (int w = 0; w < CFG::WINDOWS; w++) {
        const int bit = CFG::BITS * w;
        const uint64_t two = (uint64_t)e[bit >> 5] | ((uint64_t)e[(bit >> 5) + 1] << 32);
        const int chunk = (int)((two >> (bit & 31)) & (uint32_t)(2 * CFG::NB - 1));
        d[w] = (int8_t)(w < CFG::WINDOWS - 1 ? chunk - CFG::NB : chunk);
    }
}

// ---- the dealing of the tasks to the four waves of k_lc_buckets.  A wave runs as long as its busiest lane and a workgroup as long as its busiest
// wave, so the waves want the same number of additions.
//   halves    whole windows: class 1 (2 (2n + 1) items a window) 7, 7, 6, 6 windows and class 0 (2n items) 6, 6, 7, 7 -- within 5 % of each other
//   quarters  11 windows of 4 (2n + 1) and 11 of 4n items do not split evenly by whole windows (best: one wave 9 % over the mean), so the unit is
//             (window, class, HALF of the buckets) and the units go, heaviest first, to the wave with the least so far.  Expected additions of a
//             unit, in 64ths of the class's items: a signed digit is uniform in [-NB, NB), so |d| in 1 .. 16 takes 32 and |d| in 17 .. 32
//             takes 31; the top digit is 0 with probability ~0.04 and never above 13: 62 and 0.  (At 5 bits a unit is a whole window: 62.)
//             Result at n = 64 (tests/test_lc_quarters_host.py): every wave within 3 % of the mean.
struct LcDeal {
    uint8_t ntasks[4];
    uint8_t task[4][LC_MAXT];                    // window | class << 5 | part << 6
    uint8_t nwin[4][2];                          // distinct windows per class: what bounds the wave's list entries
};
KZG_HD int lc_task_window(int t) { return t & 31; }
KZG_HD int lc_task_class(int t) { return (t >> 5) & 1; }
KZG_HD int lc_task_part(int t) { return t >> 6; }
template <class CFG> constexpr int lc_unit_weight(int w, int cls, int part) {
    const int items = cls ? 129 : 64;            // the classes' sizes at n = 64, up to the common factor
    const bool top = w == CFG::WINDOWS - 1;
    const int f = CFG::PARTS == 1 ? 62 : top ? (part == 0 ? 62 : 0) : (part == 0 ? 32 : 31);
    return items * f;
}
template <class CFG> constexpr LcDeal lc_make_deal() {
    LcDeal d{};
    if (CFG::PER_TERM == 2) {
        for (int wid = 0; wid < 4; wid++) {
            const int n1 = wid < 2 ? 7 : 6, c1w0 = wid < 2 ? 7 * wid : 14 + 6 * (wid - 2), c0w0 = wid < 2 ? 6 * wid : 12 + 7 * (wid - 2);
            d.ntasks[wid] = LC_MAXT;
            for (int tk = 0; tk < LC_MAXT; tk++) d.task[wid][tk] = (uint8_t)(tk < n1 ? (c1w0 + tk) | 32 : c0w0 + (tk - n1));
        }
    } else {
        constexpr int NU = 2 * CFG::WINDOWS * CFG::PARTS;
        bool used[NU] = {};
        int load[4] = {0, 0, 0, 0};
        for (int round = 0; round < NU; round++) {
            int best = -1, bw = -1;
            for (int u = 0; u < NU; u++) {       // u = (window * 2 + class) * PARTS + part
                const int wt = lc_unit_weight<CFG>(u / (2 * CFG::PARTS), (u / CFG::PARTS) & 1, u % CFG::PARTS);
                if (!used[u] && wt > bw) { best = u; bw = wt; }
            }
            int wv = -1;
            for (int k = 0; k < 4; k++) if (d.ntasks[k] < LC_MAXT && (wv < 0 || load[k] < load[wv])) wv = k;
            used[best] = true; load[wv] += bw;
            d.task[wv][d.ntasks[wv]++] = (uint8_t)((best / (2 * CFG::PARTS)) | (((best / CFG::PARTS) & 1) << 5) | ((best % CFG::PARTS) << 6));
        }
        // ... then two waves trade tasks (a move or a swap) while that lowers the larger of their two loads: at 6 bits the busiest wave goes from
        // 2.8 % to 1.5 % over the mean
        auto wt = [](int t) { return lc_unit_weight<CFG>(t & 31, (t >> 5) & 1, t >> 6); };
        for (bool moved = true; moved;) {
            moved = false;
            for (int a = 0; a < 4 && !moved; a++)
                for (int b = 0; b < 4 && !moved; b++) {
                    if (a == b || load[a] <= load[b]) continue;
                    for (int i = 0; i < d.ntasks[a] && !moved; i++)
                        for (int j = -1; j < d.ntasks[b] && !moved; j++) {        // j = -1: a plain move
                            if (j < 0 && d.ntasks[b] >= LC_MAXT) continue;
                            const int delta = wt(d.task[a][i]) - (j < 0 ? 0 : wt(d.task[b][j]));
                            if (delta <= 0 || load[b] + delta >= load[a]) continue;
                            load[a] -= delta; load[b] += delta;
                            const uint8_t t = d.task[a][i];
                            if (j < 0) { d.task[a][i] = d.task[a][--d.ntasks[a]]; d.task[b][d.ntasks[b]++] = t; }
                            else { d.task[a][i] = d.task[b][j]; d.task[b][j] = t; }
                            moved = true;
                        }
                }
        }
    }
    for (int wid = 0; wid < 4; wid++)
        for (int tk = 0; tk < d.ntasks[wid]; tk++) {
            bool seen = false;
            for (int q = 0; q < tk; q++) seen = seen || (d.task[wid][q] & 63) == (d.task[wid][tk] & 63);
            if (!seen) d.nwin[wid][(d.task[wid][tk] >> 5) & 1]++;
        }
    return d;
}
template <class CFG> struct LcDealOf { static constexpr LcDeal value = lc_make_deal<CFG>(); };
// List entries a wave may have to hold: every item of a class lands in at most one list per window, whatever parts of that window the wave holds.
//   halves    7 x 2 (2n + 1) + 6 x 2n = 40 n + 14, as ever
template <class CFG> KZG_HD int lc_wave_entries(int wid, int n) {
    return LcDealOf<CFG>::value.nwin[wid][1] * lc_class_items<CFG>(1, n) + LcDealOf<CFG>::value.nwin[wid][0] * lc_class_items<CFG>(0, n);
}
template <class CFG> KZG_HD int lc_max_entries(int n) {
    int m = 0;
    for (int wid = 0; wid < 4; wid++) { const int e = lc_wave_entries<CFG>(wid, n); m = e > m ? e : m; }
    return m;
}
// The lists live in LDS while the busiest wave's fit LC_MAXT x LC_LDS_LIST entries, beyond that in a global slab with room for LC_MAXT whole
// classes (+ 2: the two entries read ahead) per wave.
constexpr int LC_LDS_LIST = 400;                 // halves: 40 n + 14 <= 5200 for n <= 129
template <class CFG> KZG_HD bool lc_lists_in_lds(int n) { return lc_max_entries<CFG>(n) <= LC_MAXT * LC_LDS_LIST; }
template <class CFG> KZG_HD int lc_list_stride_of(int n) { return lc_class_items<CFG>(1, n) + 2; }

}  // namespace kzg
