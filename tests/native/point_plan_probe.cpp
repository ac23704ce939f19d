// point_plan_probe -- runs the chunk plan of compute_kzg_proofs_at (kzg_rust_amd/csrc/point_plan.h) on the CPU for tests/test_point_plan_host.py,
// which builds it plain and with -fsanitize=address,undefined.  Nothing of HIP: the header is all it includes of the library.
//   stdin, numbers separated by white space:
//     0 <device> <blobs> <max_units> <max_pairs>  then per blob: <count> <bad>      the chunks of a call.  Point j of blob i is the number
//                                       65536 i + j + 1 as 32 big-endian bytes; bad = 0: none, 1 + j: point j is r, 5000 + j: point j is 32 x 0xff
//                                       (a count above 4096 gets an exact allocation of 32 bytes per point and no bad point: nothing of it may be read
//                                       beyond that)
//     1 <m> <counts>                    sum_point_counts: prints {"ok", "total"}
//     2 <which>                         point_list_ok of one point: 0: r - 1, 1: r, 2: r + 1, 3: 0, 4: 32 x 0xff; prints {"ok"}
//   stdout for 0: one JSON object per launch set, in order.
#include "../../kzg_rust_amd/csrc/point_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace kzg;

static size_t next() {
    unsigned long long v;
    if (scanf("%llu", &v) != 1) { fprintf(stderr, "point_plan_probe: short input\n"); exit(2); }
    return (size_t)v;
}
template <class T, class F> static void arr(const char *name, const std::vector<T> &v, F item, const char *end = ", ") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) { if (i) printf(", "); item(v[i], i); }
    printf("]%s", end);
}
static void put_number(uint8_t *p, uint64_t v) {
    memset(p, 0, 32);
    for (int i = 0; i < 8; i++) p[31 - i] = (uint8_t)(v >> (8 * i));
}

int main() {
    const size_t mode = next();
    if (mode == 1) {
        std::vector<size_t> counts(next());
        for (size_t &c : counts) c = next();
        size_t total = 0;
        const bool ok = sum_point_counts(total, counts.data(), counts.size());
        printf("{\"ok\": %d, \"total\": %llu}\n", (int)ok, (unsigned long long)(ok ? total : 0));
        return 0;
    }
    if (mode == 2) {
        const size_t which = next();
        uint8_t z[32];
        memcpy(z, PLAN_R_BE, 32);
        if (which == 0) z[31] = 0x00;
        if (which == 2) z[31] = 0x02;
        if (which == 3) memset(z, 0, 32);
        if (which == 4) memset(z, 0xff, 32);
        printf("{\"ok\": %d}\n", (int)point_list_ok(z, 1));
        return 0;
    }
    const bool device = next() != 0;
    const size_t n = next(), max_units = next(), max_pairs = next();
    std::vector<size_t> counts(n), bad(n);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) { counts[i] = next(); bad[i] = next(); total += counts[i]; }
    uint8_t *zs = total ? (uint8_t *)malloc(32 * total) : nullptr;    // exactly the call's bytes: the sanitizer sees a read past them
    for (size_t i = 0, at = 0; i < n; at += counts[i], i++)
        for (size_t j = 0; j < counts[i]; j++) {
            uint8_t *p = zs + 32 * (at + j);
            put_number(p, 65536 * i + j + 1);
            if (bad[i] == 1 + j) memcpy(p, PLAN_R_BE, 32);
            if (bad[i] == 5000 + j) memset(p, 0xff, 32);
        }
    PointPlan plan(max_units, max_pairs, counts.data(), zs, n);
    PointChunk ch;
    while (plan.next(ch, device)) {
        printf("{\"m\": %zu, \"pairs\": %zu, \"any_refused\": %d, ", ch.m(), ch.pairs.size(), (int)ch.any_refused);
        arr("pieces", ch.pieces, [](const PointPiece &p, size_t) { printf("[%zu, %zu, %zu, %zu, %zu]", p.blob, p.skip, p.len, p.first_pair, p.slot); });
        arr("pair_list", ch.pairs, [](const PqPair &p, size_t) { printf("[%u, %llu]", p.blob, (unsigned long long)p.slot); });
        arr("runs", ch.runs, [](const PointRun &r, size_t) { printf("[%zu, %zu, %zu]", r.pair, r.slot, r.len); });
        arr("refused", ch.refused, [](int r, size_t) { printf("%d", r); });
        if (ch.zs.size() != 32 * ch.pairs.size()) {
            fprintf(stderr, "point_plan_probe: %zu bytes of points for %zu pairs\n", ch.zs.size(), ch.pairs.size());
            return 3;
        }
        arr("points", ch.pairs, [&](const PqPair &, size_t p) {
            uint64_t v = 0;
            for (int i = 0; i < 8; i++) v = v << 8 | ch.zs[32 * p + 24 + i];
            printf("%llu", (unsigned long long)v);
        }, "}\n");
    }
    free(zs);
    return 0;
}
