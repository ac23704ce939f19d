// Host build (g++) of the shapes of the bucket-form linear combination (kzg_rust_amd/csrc/lc_forms.h) and of the fourth-of-a-scalar split
// (g1.h), behind a tiny C ABI for tests/test_lc_quarters_host.py.  With -DLC_PROBE_MAIN the same checks run as a stand-alone program, which is
// what the test builds under AddressSanitizer + UndefinedBehaviorSanitizer.  Test infrastructure only: never part of libkzg355.so.
#include "../../kzg_rust_amd/csrc/field.h"
#include "../../kzg_rust_amd/csrc/g1.h"
#include "../../kzg_rust_amd/csrc/lc_forms.h"
#include <cstdio>
#include <cstring>
using namespace kzg;

extern "C" {
// out: a0 .. a3, two 32-bit words each
void lcp_quarter_split(uint32_t out[8], const uint32_t k[8]) {
    uint32_t a[4][2];
    quarter_split(a, k);
    for (int j = 0; j < 4; j++) { out[2 * j] = a[j][0]; out[2 * j + 1] = a[j][1]; }
}
// digits of one quarter (2 words) / one half (4 words); returns the number of windows
int lcp_recode_quarter(int8_t *d, const uint32_t v[2]) { lc_recode<LcQuarters>(d, v); return LcQuarters::WINDOWS; }
int lcp_recode_half(int8_t *d, const uint32_t v[4]) { lc_recode<LcHalves>(d, v); return LcHalves::WINDOWS; }
// form 0: halves, 1: quarters.  out: BITS, WINDOWS, PER_TERM, NB, DIG_STRIDE, LC_TB, LC_MAXT, LC_MAXT * LC_LDS_LIST
void lcp_params(int form, int out[8]) {
    const int h[8] = {LcHalves::BITS, LcHalves::WINDOWS, LcHalves::PER_TERM, LcHalves::NB, LcHalves::DIG_STRIDE, LC_TB, LC_MAXT, LC_MAXT * LC_LDS_LIST};
    const int q[8] = {LcQuarters::BITS, LcQuarters::WINDOWS, LcQuarters::PER_TERM, LcQuarters::NB, LcQuarters::DIG_STRIDE, LC_TB, LC_MAXT, LC_MAXT * LC_LDS_LIST};
    memcpy(out, form ? q : h, sizeof h);
}
// the tasks of the four waves: ntasks[4], task[4][LC_MAXT] (window | class << 5 | part << 6)
void lcp_deal(int form, uint8_t ntasks[4], uint8_t *task) {
    const LcDeal d = form ? LcDealOf<LcQuarters>::value : LcDealOf<LcHalves>::value;
    memcpy(ntasks, d.ntasks, 4); memcpy(task, d.task, 4 * LC_MAXT);
}
int lcp_max_entries(int form, int n) { return form ? lc_max_entries<LcQuarters>(n) : lc_max_entries<LcHalves>(n); }
int lcp_lists_in_lds(int form, int n) { return form ? lc_lists_in_lds<LcQuarters>(n) : lc_lists_in_lds<LcHalves>(n); }
int lcp_items_fit(int form, int n) { return form ? lc_items_fit<LcQuarters>(n) : lc_items_fit<LcHalves>(n); }
// the constant [|x|](-G), affine: x | y, 48 big-endian bytes each
void lcp_neg_gen_x_abs(uint8_t out[96]) { const G1Affine p = g1a_neg_gen_x_abs(); fp_to_be48(out, p.x); fp_to_be48(out + 48, p.y); }
}

#if defined(LC_PROBE_MAIN)
// k = a0 + a1 m + a2 m^2 + a3 m^3 checked in 64-bit pieces: with the quarters below m the sum is rebuilt by schoolbook products on 32-bit words
static bool recombines(const uint32_t k[8]) {
    uint32_t out[8]; lcp_quarter_split(out, k);
    const uint64_t m = BLS_X_ABS;
    uint32_t acc[10] = {0};
    for (int j = 3; j >= 0; j--) {                                // Horner: acc = acc * m + a_j
        const uint32_t mw[2] = {(uint32_t)m, (uint32_t)(m >> 32)};
        uint32_t nxt[10] = {0};
        for (int i = 0; i < 8; i++) { uint64_t c = 0; for (int q = 0; q < 2; q++) { c += (uint64_t)acc[i] * mw[q] + nxt[i + q]; nxt[i + q] = (uint32_t)c; c >>= 32; }
                nxt[i + 2] += (uint32_t)c; }
        uint64_t c = 0;
        for (int i = 0; i < 10; i++) { c += (uint64_t)nxt[i] + (i < 2 ? out[2 * j + i] : 0u); acc[i] = (uint32_t)c; c >>= 32; }
        const uint64_t a = (uint64_t)out[2 * j] | ((uint64_t)out[2 * j + 1] << 32);
        if (a >= m) return false;
        int8_t d[16]; const int nw = lcp_recode_quarter(d, out + 2 * j);
        // the digits give the quarter back (signed arithmetic on 128 bits), the top digit is at most 13
        __int128 v = 0;
        for (int w = nw - 1; w >= 0; w--) v = v * (1 << LcQuarters::BITS) + d[w];
        if (v != (__int128)a || d[nw - 1] < 0 || d[nw - 1] > 13) return false;
        for (int w = 0; w < nw - 1; w++) if (d[w] < -LcQuarters::NB || d[w] >= LcQuarters::NB) return false;
    }
    for (int i = 0; i < 8; i++) if (acc[i] != k[i]) return false;
    return acc[8] == 0 && acc[9] == 0;
}
int main() {
    const uint32_t rw[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};      // r
    uint64_t s = 0x9e3779b97f4a7c15ull;
    int bad = 0;
    for (int it = 0; it < 20000; it++) {
        uint32_t k[8];
        for (int i = 0; i < 8; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; k[i] = (uint32_t)(s >> 16); }
        k[7] &= 0x3fffffffu;                                      // below 2^254 < r
        if (it == 0) memset(k, 0, sizeof k);
        if (it == 1) { memcpy(k, rw, sizeof k); k[0] -= 1; }      // r - 1
        if (it >= 2 && it < 10) { memset(k, 0, sizeof k); k[it - 2] = 0xffffffffu; k[7] &= 0x3fffffffu; }
        if (!recombines(k)) bad++;
    }
    for (int form = 0; form < 2; form++) {
        uint8_t nt[4], task[4 * LC_MAXT];
        lcp_deal(form, nt, task);
        for (int n = 8; n <= 4096; n += 97) if (lcp_max_entries(form, n) <= 0) bad++;
    }
    printf("lc_forms_probe: %d failures\n", bad);
    return bad ? 1 : 0;
}
#endif
