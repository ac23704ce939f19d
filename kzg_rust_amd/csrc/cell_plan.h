// cell_plan.h -- the host arithmetic of the EIP-7594 cell calls that lay out launch sets, free of HIP (standard headers only; it compiles with a
// plain g++ -std=c++17 and runs under the sanitizers in tests/native/cell_plan_probe.cpp): the two structs the host hands to the kernels, the
// index-set mask of a recovery, the sums of a call's counts, the chunk of the chosen-cell calls (pairs, output runs, refused words) and the
// sets, descriptors and copy runs of a recover chunk.  The drivers (cell_recover.hip, cell_proofs_at.hip, cell_recover_at.hip) queue what
// this header planned and decide nothing more about a chunk's layout.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace kzg {

// ---- k_cell_quotient.hip
// a (blob, cell) pair of a chunk: the blob's place in the chunk, the cell index (< 128), and the slot its cell is gathered into
struct CqPair { uint32_t blob, cell; uint64_t slot; };
// ---- k_cell_recover.hip
// a blob of the chunk: its index set (the tables are d_rt[set]; set < 0: refused by the host, no transform runs for it) and where its known cells
// start, in cells from d_cells
struct RecoverBlob {
    uint64_t first;
    int set, pad;
};

// what kernels.h calls CELLS_PER_EXT_BLOB, CELL_BYTES and ERR_NONCANONICAL_FR (engine.h asserts that they agree); any err word of a blob is
// that blob's KZG355_BADARGS (status_from_err)
constexpr size_t PLAN_CELLS = 128, PLAN_CELL_BYTES = 2048;
constexpr int PLAN_REFUSED = 2;

// The 128-bit mask of an index list (mask[0] bits 0..63, mask[1] bits 64..127); false unless it has 64..128 strictly ascending indices < 128.
inline bool rc_mask(uint64_t mask[2], const size_t *idx, size_t n) {
    mask[0] = mask[1] = 0;
    if (n < PLAN_CELLS / 2 || n > PLAN_CELLS) return false;
    for (size_t i = 0; i < n; i++) {
        if (idx[i] >= PLAN_CELLS || (i && idx[i] <= idx[i - 1])) return false;
        mask[idx[i] >> 6] |= (uint64_t)1 << (idx[i] & 63);
    }
    return true;
}
// a want list of the chosen-cell calls: at most 128 indices < 128, any order, repeats allowed
inline bool want_list_ok(const size_t *wx, size_t wc) {
    bool good = wc <= PLAN_CELLS;
    for (size_t j = 0; good && j < wc; j++) good = wx[j] < PLAN_CELLS;
    return good;
}
// the sum of m counts, refused when it or its 2048-fold (the sum in bytes of cells) leaves size_t
inline bool sum_counts(size_t &total, const size_t *counts, size_t m) {
    total = 0;
    for (size_t i = 0; i < m; i++) {
        if (counts[i] > SIZE_MAX / PLAN_CELL_BYTES - total) return false;
        total += counts[i];
    }
    return true;
}
// first[i] = counts[0] + .. + counts[i - 1], i <= m: where a range of blobs that goes to a replica starts in the call's flat lists
inline std::vector<size_t> prefix_sums(const size_t *counts, size_t m) {
    std::vector<size_t> first(m + 1, 0);
    for (size_t i = 0; i < m; i++) first[i + 1] = first[i] + counts[i];
    return first;
}

// ---- a chunk of a chosen-cell call: whole blobs while their pairs fit max_pairs (CQ_CHUNK; a blob has at most 128) and there are at most
// max_units of them (CC_CHUNK).  A blob the host refused fills no pair and still takes its slots, so that the pairs of a chunk are not
// always one run of slots.
// a chunk's output runs: `len` pairs from the chunk's pair `pair` on land in the call's slots `slot` onwards, counted from the chunk's first slot
struct PlanRun { size_t pair, slot, len; };
struct CellChunk {
    const size_t max_units, max_pairs;
    std::vector<CqPair> pairs;
    std::vector<PlanRun> runs;
    std::vector<int> refused;                                     // the chunk's err words, when the host refuses one of its blobs
    std::vector<size_t> first_pair;                               // of each blob of the chunk (refused: none)
    bool any_refused = false;
    size_t m = 0, slots = 0;                                      // blobs taken, and their slots
    CellChunk(size_t units, size_t pairs_) : max_units(units), max_pairs(pairs_) {}
    void clear() {
        pairs.clear(); runs.clear(); refused.clear(); first_pair.clear();
        any_refused = false;
        m = slots = 0;
    }
    // The next blob, wanting the wc cells wx (good: the caller accepts it, and then every wx[j] < 128).  False, and nothing of the blob is
    // taken, when the chunk is full or the blob's pairs would pass max_pairs: it opens the next chunk.  The host form writes pair after pair
    // and copies run by run; the device form writes into the caller's slots.
    bool add(bool good, const size_t *wx, size_t wc, bool device) {
        if (m == max_units || (good && pairs.size() + wc > max_pairs)) return false;
        first_pair.push_back(pairs.size());
        refused.push_back(good ? 0 : PLAN_REFUSED);
        any_refused |= !good;
        if (good && wc) {
            if (runs.empty() || runs.back().slot + runs.back().len != slots) runs.push_back(PlanRun{pairs.size(), slots, 0});
            runs.back().len += wc;
            for (size_t j = 0; j < wc; j++) pairs.push_back(CqPair{(uint32_t)m, (uint32_t)wx[j], device ? slots + j : (uint64_t)pairs.size()});
        }
        slots += wc;
        m++;
        return true;
    }
};

// ---- the sets, descriptors and known cells of a recover chunk of up to `cap` blobs.  The distinct masks are numbered as they come (blobs with
// the same set share one RecoverTables wherever they sit; max_sets tables: 1 for the calls with one set for all blobs, else cap).  The host form
// packs the accepted blobs' cells into the workspace (at most 128 each, whatever a refused blob's count says), run of neighbours by run; the
// device form reads them where they are, from the chunk's first cell on.
struct RecoverStage {
    static constexpr size_t DESC_WORDS = sizeof(RecoverBlob) / sizeof(uint64_t);
    const size_t cap, max_sets;
    std::vector<uint64_t> up;                                     // what a chunk uploads: 2 * max_sets mask words, then RecoverBlob per blob
    std::map<std::pair<uint64_t, uint64_t>, int> sets;
    std::vector<std::pair<size_t, size_t>> copies;                // the host form's runs of known cells: (first cell of the call, cells)
    size_t base = 0, blobs = 0, known = 0, staged = 0;            // the call's cells before the chunk; blobs added, their cells, those staged
    bool in_run = false;
    RecoverStage(size_t cap_, size_t max_sets_) : cap(cap_), max_sets(max_sets_), up(2 * max_sets_ + DESC_WORDS * cap_, 0) {}
    void reset(size_t first_cell) {
        sets.clear(); copies.clear();
        base = first_cell;
        blobs = known = staged = 0;
        in_run = false;
    }
    // the next blob of the chunk (fewer than cap so far), known at known_count cells with this mask; a refused blob ends the current copy run
    void add(bool good, const uint64_t mask[2], size_t known_count, bool device) {
        RecoverBlob d{0, -1, 0};
        if (!good) {
            in_run = false;
        } else {
            d.set = sets.emplace(std::make_pair(mask[0], mask[1]), (int)sets.size()).first->second;
            up[2 * d.set] = mask[0];
            up[2 * d.set + 1] = mask[1];
            d.first = device ? known : staged;
            if (!device) {
                if (!in_run) copies.push_back({base + known, 0});
                copies.back().second += known_count;
                in_run = true;
                staged += known_count;
            }
        }
        memcpy(&up[2 * max_sets + DESC_WORDS * blobs++], &d, sizeof d);
        known += known_count;
    }
    RecoverBlob blob(size_t i) const {
        RecoverBlob d;
        memcpy(&d, &up[2 * max_sets + DESC_WORDS * i], sizeof d);
        return d;
    }
    size_t up_bytes() const { return sizeof(uint64_t) * up.size(); }
    // where the upload lies in the workspace's z buffer: the masks behind Tables[max_sets], the descriptors behind the masks, and the first
    // byte behind the descriptors (the pair list of recover_cells_and_kzg_proofs_at)
    template <class Tables> size_t masks_off() const {
        static_assert(sizeof(Tables) % alignof(RecoverBlob) == 0 && sizeof(RecoverBlob) % alignof(CqPair) == 0 && alignof(CqPair) <= sizeof(uint64_t) &&
                          alignof(RecoverBlob) <= sizeof(uint64_t),
                      "masks, descriptors and pairs behind the tables are aligned");
        return sizeof(Tables) * max_sets;
    }
    template <class Tables> size_t desc_off() const { return masks_off<Tables>() + 2 * sizeof(uint64_t) * max_sets; }
    template <class Tables> size_t end_off() const { return masks_off<Tables>() + up_bytes(); }
};

// one chunk of compute_cell_kzg_proofs_at: the next of `units` blobs, counts[i] wanted cells each, their indices one after the other in idx
// (both from the chunk's first blob on; idx may be null when no cell is wanted)
inline void plan_compute_chunk(CellChunk &ch, const size_t *counts, const size_t *idx, size_t units, bool device) {
    ch.clear();
    while (ch.m < units) {
        const size_t wc = counts[ch.m], *wx = wc ? idx + ch.slots : nullptr;
        if (!ch.add(want_list_ok(wx, wc), wx, wc, device)) break;
    }
}
// one chunk of recover_cells_and_kzg_proofs_at: a blob is good when both of its lists are; rs (reset by the caller) takes what ch took
inline void plan_recover_chunk(CellChunk &ch, RecoverStage &rs, const size_t *kcounts, const size_t *kidx, const size_t *wcounts, const size_t *widx,
                               size_t units, bool device) {
    ch.clear();
    while (ch.m < units) {
        const size_t kc = kcounts[ch.m], wc = wcounts[ch.m], *wx = wc ? widx + ch.slots : nullptr;
        uint64_t mask[2] = {0, 0};
        const bool good = want_list_ok(wx, wc) && rc_mask(mask, kidx + rs.known, kc);
        if (!ch.add(good, wx, wc, device)) break;
        rs.add(good, mask, kc, device);
    }
}

}  // namespace kzg
