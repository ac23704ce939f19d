// cell_recover_at.hip -- the C entry points of recover_cells_and_kzg_proofs_at (chosen EIP-7594 cells of recovered blobs and their proofs;
// include/kzg355.h) (host side of libkzg355.so; see engine.h).  recover_cells_and_kzg_proofs pays the whole FK20 chain whatever is wanted of its
// 128 proofs.  Here the erasure decoding of that call (k_cell_recover.hip: k_rc_vanish, k_rc_interp, k_rc_columns) is joined to the per-pair
// chain of compute_cell_kzg_proofs_at (k_cq_quotient on the recovered coefficients, then the fixed-base MSM of the commitment path), and the
// cells asked for are written by k_rc_cells_at (k_cell_recover_at.hip).  One set of launches per chunk of whole blobs; the host checks both
// lists of every blob, lays out the chunk's sets, descriptors and pairs, copies known cells in and cells / proofs out and sets the statuses.
#include "engine.h"

namespace kzg355_impl {

// a chunk's output runs: `len` pairs from the chunk's pair `pair` on land in the call's slots `slot` onwards, counted from the chunk's first
// slot (a blob the host refused fills no pair and may still take slots, so that the pairs of a chunk are not always one run)
struct RaRun { size_t pair, slot, len; };

// m > 0 blobs on the device of cs (a replica, for a handle over several devices); the arguments are checked, and both sums of counts fit.
// Blob i is known at kcounts[i] cells (indices kidx[koff_i ..], cells at cells + 2048 koff_i) and asks for wcounts[i] cells, the indices
// widx[woff_i ..]; slot woff_i + j of cells_out / proofs_out receives cell widx[woff_i + j] of its recovered extension and that cell's proof.
// device: cells, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where they are.
// The workspace's buffers by role: blobs = the chunk's known cells (host form); z = the chunk's recover tables, the masks of its sets, the
// descriptors of its blobs and, behind them, its pair list; scal_b = u; y = coefficients; scal_a = MSM scalars; records = the pairs' cells (host
// form); partials, digits, out48 and h_out are the MSM's, as on the commitment path.
static_assert(sizeof(RecoverTables) % alignof(RecoverBlob) == 0 && sizeof(RecoverBlob) % alignof(CqPair) == 0 && alignof(CqPair) <= sizeof(uint64_t),
              "masks, descriptors and pairs behind the tables in w->z are aligned");
static int ra_run(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *kcounts, const size_t *kidx, const uint8_t *cells,
                  const size_t *wcounts, const size_t *widx, size_t m, const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, m, code); };
    if (m > ((size_t)1 << 32) || is_small(cs)) return refuse(KZG355_BADARGS);    // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    if ((rc = ensure_cc_consts(s, w))) return refuse(rc);
    if (proofs_out && (rc = ensure_wide_table(s))) return refuse(rc);             // the first call that wants proofs builds the table, as a commitment does
    s->n_cell_sets.fetch_add(1);
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    const size_t desc_words = sizeof(RecoverBlob) / sizeof(uint64_t);
    std::vector<CqPair> pairs;
    std::vector<RaRun> runs;
    std::vector<int> refused;                                     // the chunk's err words, when the host refuses one of its blobs
    std::vector<size_t> first_pair;                               // of each blob of the chunk (refused: none)
    std::vector<uint64_t> up;                                     // what a chunk uploads: 2 * mc mask words, then RecoverBlob per blob
    std::vector<std::pair<size_t, size_t>> copies;                // the host form's runs of known cells: (first cell of the call, cells)
    Timed tm(s, w);
    int first = KZG355_OK;
    size_t koff = 0, woff = 0;                                    // the call's known cells and slots before the chunk
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    for (size_t c0 = 0; c0 < m;) {
        // the chunk: whole blobs while their pairs fit CQ_CHUNK (a blob has at most 128) and there are at most CC_CHUNK of them.  Blobs with the
        // same set share one RecoverTables wherever they sit; the host form packs the accepted blobs' cells into w->blobs, run of neighbours by run.
        pairs.clear(); runs.clear(); refused.clear(); first_pair.clear(); copies.clear();
        const size_t cap = m - c0 < CC_CHUNK ? m - c0 : CC_CHUNK;
        up.assign((2 + desc_words) * cap, 0);
        RecoverBlob *desc = reinterpret_cast<RecoverBlob *>(up.data() + 2 * cap);
        std::map<std::pair<uint64_t, uint64_t>, int> sets;
        bool any_refused = false, in_run = false;
        size_t mc = 0, known = 0, slots = 0, staged = 0;
        for (; mc < cap; mc++) {
            const size_t kc = kcounts[c0 + mc], wc = wcounts[c0 + mc], *wx = wc ? widx + woff + slots : nullptr;
            uint64_t mask[2];
            bool good = wc <= (size_t)CELLS_PER_EXT_BLOB;
            for (size_t j = 0; good && j < wc; j++) good = wx[j] < (size_t)CELLS_PER_EXT_BLOB;
            good = good && rc_mask(mask, kidx + koff + known, kc);
            if (good && pairs.size() + wc > CQ_CHUNK) break;
            first_pair.push_back(pairs.size());
            refused.push_back(good ? 0 : ERR_NONCANONICAL_FR);   // any err word is this blob's KZG355_BADARGS (status_from_err)
            if (!good) {
                desc[mc] = RecoverBlob{0, -1, 0};
                any_refused = true;
                in_run = false;
            } else {
                const int set = sets.emplace(std::make_pair(mask[0], mask[1]), (int)sets.size()).first->second;
                up[2 * set] = mask[0];
                up[2 * set + 1] = mask[1];
                desc[mc] = RecoverBlob{device ? known : staged, set, 0};
                if (!device) {
                    if (!in_run) copies.push_back({koff + known, 0});
                    copies.back().second += kc;
                    in_run = true;
                    staged += kc;
                }
                if (wc) {
                    if (runs.empty() || runs.back().slot + runs.back().len != slots) runs.push_back(RaRun{pairs.size(), slots, 0});
                    runs.back().len += wc;
                    // (the host form writes pair after pair and copies run by run; the device form writes into the caller's slots)
                    for (size_t j = 0; j < wc; j++) pairs.push_back(CqPair{(uint32_t)mc, (uint32_t)wx[j], device ? slots + j : (uint64_t)pairs.size()});
                }
            }
            known += kc;
            slots += wc;
        }
        const size_t P = pairs.size();
        const size_t up_bytes = sizeof(uint64_t) * (2 + desc_words) * cap;
        int crc;
        if ((!device && (crc = w->blobs.ensure((size_t)CELL_BYTES * (staged ? staged : 1)))) ||
            (crc = w->z.ensure(sizeof(RecoverTables) * cap + up_bytes + sizeof(CqPair) * (P ? P : 1))) ||
            (crc = w->scal_b.ensure(sizeof(Fr) * CELLS_PER_EXT_BLOB * CELL_FE * mc)) ||
            (proofs_out && ((crc = w->y.ensure(sizeof(Fr) * N_FE * mc)) || (P && (crc = w->scal_a.ensure(sizeof(Fr) * N_FE * P))) ||
                            (P && !device && (crc = w->h_out.ensure(48 * P))))) ||
            (cells_out && P && !device && (crc = w->records.ensure((size_t)CELL_BYTES * P))))
            return crc;
        if ((crc = launch_set_begin(w, mc))) return crc;
        hipStream_t st = w->stream;
        RecoverTables *rt = w->z.as<RecoverTables>();
        uint64_t *d_up = reinterpret_cast<uint64_t *>(rt + cap);
        const RecoverBlob *d_desc = reinterpret_cast<const RecoverBlob *>(d_up + 2 * cap);
        CqPair *d_pairs = reinterpret_cast<CqPair *>(d_up + (2 + desc_words) * cap);
        size_t dst = 0;
        for (const auto &c : copies) {
            HIPCHK(hipMemcpyAsync(w->blobs.as<uint8_t>() + dst * CELL_BYTES, cells + c.first * CELL_BYTES, c.second * CELL_BYTES, hipMemcpyHostToDevice, st));
            dst += c.second;
        }
        HIPCHK(hipMemcpyAsync(d_up, up.data(), up_bytes, hipMemcpyHostToDevice, st));
        if (any_refused) HIPCHK(hipMemcpyAsync(w->err.p, refused.data(), sizeof(int) * mc, hipMemcpyHostToDevice, st));
        if (P) HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(CqPair) * P, hipMemcpyHostToDevice, st));
        const uint8_t *d_known = device ? cells + koff * CELL_BYTES : w->blobs.as<uint8_t>();
        tm.begin("rc_vanish");
        launch_rc_vanish(cc, d_up, (int)sets.size(), rt, st);
        tm.end();
        tm.begin("rc_interp");
        launch_rc_interp(d_known, d_desc, (int)mc, cc, rt, w->scal_b.as<Fr>(), w->err.as<int>(), st);
        tm.end();
        tm.begin("rc_columns");
        launch_rc_columns(w->scal_b.as<Fr>(), d_desc, (int)mc, cc, rt, proofs_out ? w->y.as<Fr>() : nullptr, cells_out != nullptr, st);
        tm.end();
        if (cells_out && P) {
            tm.begin("rc_cells_at");
            launch_rc_cells_at(w->scal_b.as<Fr>(), d_desc, d_pairs, (int)P, cc, device ? cells_out + (size_t)CELL_BYTES * woff : w->records.as<uint8_t>(), st);
            tm.end();
            if (!device) for (const RaRun &r : runs)
                HIPCHK(hipMemcpyAsync(cells_out + (size_t)CELL_BYTES * (woff + r.slot), w->records.as<uint8_t>() + (size_t)CELL_BYTES * r.pair,
                                      (size_t)CELL_BYTES * r.len, hipMemcpyDeviceToHost, st));
        }
        if (proofs_out && P) {
            tm.begin("cq_quotient");
            launch_cq_quotient(w->y.as<Fr>(), d_pairs, (int)P, w->err.as<int>(), cc, w->scal_a.as<Fr>(), st);
            tm.end();
            if ((crc = msm_to_device(s, w, tm, (int)P, nullptr, w->scal_a.as<Fr>()))) return crc;
            if (!device) HIPCHK(hipMemcpyAsync(w->h_out.p, w->out48.p, 48 * P, hipMemcpyDeviceToHost, st));
            else for (const RaRun &r : runs)
                HIPCHK(hipMemcpyAsync(proofs_out + 48 * (woff + r.slot), w->out48.as<uint8_t>() + 48 * r.pair, 48 * r.len, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipGetLastError());
        if ((crc = launch_set_results(w, mc)) || (crc = launch_set_wait(w, tm))) return crc;
        // a refused blob's proofs are not copied into host outputs
        size_t slot = woff;
        crc = launch_set_read(w, mc, status ? status + c0 : nullptr, 0, [&](size_t i, int &bst) {
            const size_t wc = wcounts[c0 + i];
            if (bst == KZG355_OK && proofs_out && !device && wc) memcpy(proofs_out + 48 * slot, w->h_out.as<uint8_t>() + 48 * first_pair[i], 48 * wc);
            slot += wc;
        });
        if (first == KZG355_OK) first = crc;
        koff += known;
        woff += slots;
        c0 += mc;
    }
    return KZG355_OK;
    };
    if ((rc = run())) return refuse(rc);
    return first;
}

// the sum of m counts, refused when it or its 2048-fold leaves size_t
static bool ra_sum(size_t &total, const size_t *counts, size_t m) {
    total = 0;
    for (size_t i = 0; i < m; i++) {
        if (counts[i] > SIZE_MAX / CELL_BYTES - total) return false;
        total += counts[i];
    }
    return true;
}

static int ra_impl(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *kcounts, const size_t *kidx, const uint8_t *cells,
                   const size_t *wcounts, const size_t *widx, size_t m, const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, m, code); };
    if (!cs || (!cells_out && !proofs_out)) return refuse(KZG355_BADARGS);
    if (m == 0) return KZG355_OK;
    if (!kcounts || !wcounts || !kidx || !cells || m > ((size_t)1 << 32)) return refuse(KZG355_BADARGS);
    if (device && (((uintptr_t)cells_out & 15) || ((uintptr_t)proofs_out & 15) || ((uintptr_t)cells & 15))) return refuse(KZG355_BADARGS);
    size_t known = 0, wanted = 0;
    if (!ra_sum(known, kcounts, m) || !ra_sum(wanted, wcounts, m) || (wanted && !widx)) return refuse(KZG355_BADARGS);
    if (cs->multi && !device) {                                   // ranges of blobs over the replicas: each starts at its own two prefix sums
        std::vector<size_t> kfirst(m + 1, 0), wfirst(m + 1, 0);
        for (size_t i = 0; i < m; i++) { kfirst[i + 1] = kfirst[i] + kcounts[i]; wfirst[i + 1] = wfirst[i] + wcounts[i]; }
        return cc_fan_out(cs, m, status, [&](const kzg355_settings *rep, size_t u0, size_t k) {
            return ra_run(cells_out ? cells_out + (size_t)CELL_BYTES * wfirst[u0] : nullptr, proofs_out ? proofs_out + 48 * wfirst[u0] : nullptr,
                          status ? status + u0 : nullptr, kcounts + u0, kidx + kfirst[u0], cells + (size_t)CELL_BYTES * kfirst[u0], wcounts + u0,
                          widx ? widx + wfirst[u0] : nullptr, k, rep, false);
        });
    }
    return ra_run(cells_out, proofs_out, status, kcounts, kidx, cells, wcounts, widx, m, cs, device);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_recover_cells_and_kzg_proofs_at_many_sets(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *cell_counts,
                                                     const size_t *cell_indices, const uint8_t *cells, const size_t *want_counts,
                                                     const size_t *want_indices, size_t m, const kzg355_settings *s) {
    return ra_impl(cells_out, proofs_out, status, cell_counts, cell_indices, cells, want_counts, want_indices, m, s, false);
}

int kzg355_recover_cells_and_kzg_proofs_at_many_sets_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const size_t *cell_counts,
                                                            const size_t *cell_indices, const uint8_t *d_cells, const size_t *want_counts,
                                                            const size_t *want_indices, size_t m, const kzg355_settings *s) {
    return ra_impl(d_cells_out, d_proofs_out, status, cell_counts, cell_indices, d_cells, want_counts, want_indices, m, s, true);
}

int kzg355_recover_cells_and_kzg_proofs_at(uint8_t *cells_out, uint8_t *proofs_out, const size_t *cell_indices, const uint8_t *cells, size_t n,
                                           const size_t *want_indices, size_t k, const kzg355_settings *s) {
    return ra_impl(cells_out, proofs_out, nullptr, &n, cell_indices, cells, &k, want_indices, 1, s, false);
}

#pragma GCC visibility pop
}  // extern "C"
