// point_plan.h -- the host arithmetic of compute_kzg_proofs_at (openings of blobs at chosen points; include/kzg355.h) that lays out its launch
// sets, free of HIP (standard headers only; it compiles with a plain g++ -std=c++17 and runs under the sanitizers in
// tests/native/point_plan_probe.cpp): the struct the host hands to k_pq_quotient, the check of a blob's points, the sum of a call's counts and
// the chunks of a call.  Unlike a blob of cells a blob of points can want more pairs than a chunk holds, so a blob may be cut at a chunk
// border.  The driver (point_proofs_at.hip) queues what this header planned and decides nothing more about a chunk's layout.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace kzg {

// ---- k_point_quotient.hip
// a (blob, point) pair of a chunk: the blob's place in the chunk, and the slot its y is written to (host form: the pair's own number, the host
// copies piece by piece; device form: the call's slot)
struct PqPair { uint32_t blob, pad; uint64_t slot; };

// what kernels.h calls N_FE and ERR_NONCANONICAL_FR (engine.h asserts that they agree); any err word of a blob is that blob's KZG355_BADARGS
constexpr size_t PLAN_POINTS = 4096;
constexpr int PLAN_POINT_REFUSED = 2;

// the order r of the scalar field, big-endian: a point is canonical when its 32 bytes are below it
constexpr uint8_t PLAN_R_BE[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                   0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
// a point list of a blob: at most 4096 points, each below r; any order, repeats allowed
inline bool point_list_ok(const uint8_t *zs, size_t k) {
    bool good = k <= PLAN_POINTS;
    for (size_t j = 0; good && j < k; j++) good = memcmp(zs + 32 * j, PLAN_R_BE, 32) < 0;
    return good;
}
// the sum of m counts, refused when it or its 48-fold (the sum in bytes of proofs) leaves size_t
inline bool sum_point_counts(size_t &total, const size_t *counts, size_t m) {
    total = 0;
    for (size_t i = 0; i < m; i++) {
        if (counts[i] > SIZE_MAX / 48 - total) return false;
        total += counts[i];
    }
    return true;
}

// ---- a chunk of the call: pieces of blobs in blob order, at most max_units of them (CC_CHUNK) and max_pairs pairs (CQ_CHUNK).  A piece is a
// whole blob while its points fit; the blob at the border is cut there, and the next chunk starts with the rest of its points (its field stage
// runs again).  A blob the host refused, or one that wants nothing, takes a piece without pairs; a refused one keeps its slots.
// a chunk's output runs: `len` pairs from the chunk's pair `pair` on land in the call's slots `slot` onwards
struct PointRun { size_t pair, slot, len; };
// blob `blob` of the call, its points skip .. skip + len - 1 (pairs first_pair onwards; refused: none), which fill the call's slots from `slot`
struct PointPiece { size_t blob, skip, len, first_pair, slot; };
struct PointChunk {
    std::vector<PqPair> pairs;
    std::vector<uint8_t> zs;                                      // the pairs' points, 32 bytes each, in pair order
    std::vector<PointRun> runs;
    std::vector<PointPiece> pieces;
    std::vector<int> refused;                                     // the chunk's err words, when the host refuses one of its blobs
    bool any_refused = false;
    size_t m() const { return pieces.size(); }
    void clear() {
        pairs.clear(); zs.clear(); runs.clear(); pieces.clear(); refused.clear();
        any_refused = false;
    }
};

// the chunks of a call over n blobs, one after the other: which blobs are good is decided before the first of them
struct PointPlan {
    const size_t max_units, max_pairs;
    const size_t *counts;
    const uint8_t *zs;
    const size_t n;
    std::vector<size_t> first;                                    // first[i] = counts[0] + .. + counts[i - 1], i <= n
    std::vector<uint8_t> good;
    size_t b = 0, done = 0;                                       // the next blob, and how many of its points earlier chunks took
    // (the sum of the counts fits: sum_point_counts; zs may be null when it is 0)
    PointPlan(size_t units, size_t pairs_, const size_t *counts_, const uint8_t *zs_, size_t n_)
        : max_units(units), max_pairs(pairs_), counts(counts_), zs(zs_), n(n_), first(n_ + 1, 0), good(n_, 0) {
        for (size_t i = 0; i < n; i++) {
            first[i + 1] = first[i] + counts[i];
            good[i] = counts[i] <= PLAN_POINTS && point_list_ok(counts[i] ? zs + 32 * first[i] : nullptr, counts[i]);
        }
    }
    // The next chunk; false when the call is through.  The host form writes pair after pair and copies piece by piece; the device form writes
    // ys into the caller's slots and copies proofs run by run.
    bool next(PointChunk &ch, bool device) {
        ch.clear();
        while (b < n && ch.m() < max_units) {
            const bool ok = good[b] != 0;
            const size_t left = ok ? counts[b] - done : 0, room = max_pairs - ch.pairs.size();
            if (left && !room) break;
            const size_t len = left < room ? left : room, slot = first[b] + done;
            ch.pieces.push_back(PointPiece{b, done, len, ch.pairs.size(), slot});
            ch.refused.push_back(ok ? 0 : PLAN_POINT_REFUSED);
            ch.any_refused |= !ok;
            if (len) {
                if (ch.runs.empty() || ch.runs.back().slot + ch.runs.back().len != slot) ch.runs.push_back(PointRun{ch.pairs.size(), slot, 0});
                ch.runs.back().len += len;
                const uint32_t at = (uint32_t)(ch.m() - 1);
                for (size_t j = 0; j < len; j++) ch.pairs.push_back(PqPair{at, 0, device ? slot + j : (uint64_t)ch.pairs.size()});
                ch.zs.insert(ch.zs.end(), zs + 32 * slot, zs + 32 * (slot + len));
            }
            if (len == left) { b++; done = 0; }
            else { done += len; break; }                            // cut: the chunk is full
        }
        return ch.m() != 0;
    }
};

}  // namespace kzg
