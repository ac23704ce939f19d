// cell_plan_probe -- runs the chunk plan of the chosen-cell calls (kzg_rust_amd/csrc/cell_plan.h) on the CPU for tests/test_cell_plan_host.py, which
// builds it with -fsanitize=address,undefined.  Nothing of HIP: the header is all it includes of the library.
//   stdin, numbers separated by white space:
//     0 <device> <units> <max_units> <max_pairs>  then per unit: <want count> <want indices>                     compute_cell_kzg_proofs_at
//     1 <device> <units> <max_units> <max_pairs>  then per unit: <known count> <known indices> <want count> <want indices>   recover_..._at
//     2 <n> <indices>                 rc_mask: prints {"ok", "mask"}
//     3 <m> <counts>                  sum_counts: prints {"ok", "total"}
//   stdout for 0 and 1: one JSON object per launch set, in order.
#include "../../kzg_rust_amd/csrc/cell_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace kzg;

struct FakeTables { uint64_t words[320]; };   // stands in for RecoverTables (kernels.h): only its size enters the offsets

static size_t next() {
    unsigned long long v;
    if (scanf("%llu", &v) != 1) { fprintf(stderr, "cell_plan_probe: short input\n"); exit(2); }
    return (size_t)v;
}
static std::vector<size_t> list(size_t n) {
    std::vector<size_t> v(n);
    for (size_t &x : v) x = next();
    return v;
}
template <class T, class F> static void arr(const char *name, const std::vector<T> &v, F item, const char *end = ", ") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) { if (i) printf(", "); item(v[i], i); }
    printf("]%s", end);
}

int main() {
    const size_t mode = next();
    if (mode == 2) {
        const std::vector<size_t> idx = list(next());
        uint64_t mask[2];
        const bool ok = rc_mask(mask, idx.data(), idx.size());
        printf("{\"ok\": %d, \"mask\": [%llu, %llu]}\n", (int)ok, (unsigned long long)mask[0], (unsigned long long)mask[1]);
        return 0;
    }
    if (mode == 3) {
        const std::vector<size_t> counts = list(next());
        size_t total;
        const bool ok = sum_counts(total, counts.data(), counts.size());
        printf("{\"ok\": %d, \"total\": %llu}\n", (int)ok, (unsigned long long)total);
        return 0;
    }
    const bool recover = mode == 1, device = next() != 0;
    const size_t m = next(), max_units = next(), max_pairs = next();
    std::vector<size_t> kcounts, kidx, wcounts, widx;
    for (size_t i = 0; i < m; i++) {
        if (recover) {
            kcounts.push_back(next());
            for (size_t x : list(kcounts.back())) kidx.push_back(x);
        }
        wcounts.push_back(next());
        for (size_t x : list(wcounts.back())) widx.push_back(x);
    }
    const std::vector<size_t> wfirst = prefix_sums(wcounts.data(), m);
    CellChunk ch(max_units, max_pairs);
    size_t koff = 0, woff = 0;
    for (size_t c0 = 0; c0 < m; c0 += ch.m, woff += ch.slots) {
        const size_t cap = m - c0 < max_units ? m - c0 : max_units;
        RecoverStage rs(cap, cap);
        rs.reset(koff);
        const size_t *wx = widx.empty() ? nullptr : widx.data() + woff;
        if (recover) plan_recover_chunk(ch, rs, kcounts.data() + c0, kidx.data() + koff, wcounts.data() + c0, wx, m - c0, device);
        else plan_compute_chunk(ch, wcounts.data() + c0, wx, m - c0, device);
        if (!ch.m || woff != wfirst[c0]) { fprintf(stderr, "cell_plan_probe: a chunk without blobs, or slots that do not follow the counts\n"); return 3; }
        printf("{\"c0\": %zu, \"m\": %zu, \"pairs\": %zu, \"slots\": %zu, \"any_refused\": %d, ", c0, ch.m, ch.pairs.size(), ch.slots, (int)ch.any_refused);
        arr("pair_list", ch.pairs, [](const CqPair &p, size_t) { printf("[%u, %u, %llu]", p.blob, p.cell, (unsigned long long)p.slot); });
        arr("runs", ch.runs, [](const PlanRun &r, size_t) { printf("[%zu, %zu, %zu]", r.pair, r.slot, r.len); });
        arr("first_pair", ch.first_pair, [](size_t v, size_t) { printf("%zu", v); });
        arr("refused", ch.refused, [](int v, size_t) { printf("%d", v); }, recover ? ", " : "}\n");
        if (recover) {
            arr("set", ch.refused, [&](int, size_t i) { printf("%d", rs.blob(i).set); });
            arr("first", ch.refused, [&](int, size_t i) { printf("%llu", (unsigned long long)rs.blob(i).first); });
            arr("copies", rs.copies, [](const std::pair<size_t, size_t> &c, size_t) { printf("[%zu, %zu]", c.first, c.second); });
            arr("masks", ch.refused, [&](int, size_t i) {
                const int set = rs.blob(i).set;
                if (set < 0) printf("null");
                else printf("[%llu, %llu]", (unsigned long long)rs.up[2 * set], (unsigned long long)rs.up[2 * set + 1]);
            });
            printf("\"n_sets\": %zu, \"blobs\": %zu, \"known\": %zu, \"staged\": %zu, \"up_bytes\": %zu, \"offsets\": [%zu, %zu, %zu]}\n", rs.sets.size(), rs.blobs,
                   rs.known, rs.staged, rs.up_bytes(), rs.masks_off<FakeTables>(), rs.desc_off<FakeTables>(), rs.end_off<FakeTables>());
            koff += rs.known;
        }
    }
    return 0;
}
