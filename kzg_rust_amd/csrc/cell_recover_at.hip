// cell_recover_at.hip -- the C entry points of recover_cells_and_kzg_proofs_at (chosen EIP-7594 cells of recovered blobs and their proofs;
// include/kzg355.h) (host side of libkzg355.so; see engine.h).  recover_cells_and_kzg_proofs pays the whole FK20 chain whatever is wanted of its
// 128 proofs.  Here the erasure decoding of that call (k_cell_recover.hip: k_rc_vanish, k_rc_interp, k_rc_columns) is joined to the per-pair
// chain of compute_cell_kzg_proofs_at (k_cq_quotient on the recovered coefficients, then the fixed-base MSM of the commitment path), and the
// cells asked for are written by k_rc_cells_at (k_cell_recover_at.hip).  One set of launches per chunk of whole blobs; the host checks both
// lists of every blob, lays out the chunk's sets, descriptors and pairs, copies known cells in and cells / proofs out and sets the statuses.
#include "engine.h"

namespace kzg355_impl {

// m > 0 blobs on the device of cs (a replica, for a handle over several devices); the arguments are checked, and both sums of counts fit.
// Blob i is known at kcounts[i] cells (indices kidx[koff_i ..], cells at cells + 2048 koff_i) and asks for wcounts[i] cells, the indices
// widx[woff_i ..]; slot woff_i + j of cells_out / proofs_out receives cell widx[woff_i + j] of its recovered extension and that cell's proof.
// device: cells, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where they are.
// The workspace's buffers by role: blobs = the chunk's known cells (host form); z = the chunk's recover tables, the masks of its sets, the
// descriptors of its blobs and, behind them, its pair list; scal_b = u; y = coefficients; scal_a = MSM scalars; records = the pairs' cells (host
// form); partials, digits, out48 and h_out are the MSM's, as on the commitment path.
static int ra_run(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *kcounts, const size_t *kidx, const uint8_t *cells,
                  const size_t *wcounts, const size_t *widx, size_t m, const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, m, code); };
    std::unique_ptr<WsGuard> g;
    int rc;
    if ((rc = cell_call_begin(cs, m, g, proofs_out ? wide_table_setup : nullptr))) return refuse(rc);
    kzg355_settings *s = g->s; Workspace *w = g->w;
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    CellChunk ch(CC_CHUNK, CQ_CHUNK);
    Timed tm(s, w);
    int first = KZG355_OK;
    size_t koff = 0, woff = 0;                                    // the call's known cells and slots before the chunk
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    for (size_t c0 = 0; c0 < m; c0 += ch.m, woff += ch.slots) {
        // the chunk (cell_plan.h); its tables are laid out for as many sets as it could have blobs
        const size_t cap = m - c0 < CC_CHUNK ? m - c0 : CC_CHUNK;
        RecoverStage rs(cap, cap);
        rs.reset(koff);
        plan_recover_chunk(ch, rs, kcounts + c0, kidx + koff, wcounts + c0, widx ? widx + woff : nullptr, m - c0, device);
        const size_t mc = ch.m, P = ch.pairs.size();
        uint8_t *cells_at = cells_out ? cells_out + (size_t)CELL_BYTES * woff : nullptr, *proofs_at = proofs_out ? proofs_out + 48 * woff : nullptr;
        int crc;
        if ((!device && (crc = w->blobs.ensure((size_t)CELL_BYTES * (rs.staged ? rs.staged : 1)))) ||
            (crc = w->z.ensure(rs.end_off<RecoverTables>() + sizeof(CqPair) * (P ? P : 1))) ||
            (crc = w->scal_b.ensure(sizeof(Fr) * CELLS_PER_EXT_BLOB * CELL_FE * mc)) ||
            (proofs_out && ((crc = w->y.ensure(sizeof(Fr) * N_FE * mc)) || (P && (crc = w->scal_a.ensure(sizeof(Fr) * N_FE * P))) ||
                            (P && !device && (crc = w->h_out.ensure(48 * P))))) ||
            (cells_out && P && !device && (crc = w->records.ensure((size_t)CELL_BYTES * P))))
            return crc;
        if ((crc = launch_set_begin(w, mc))) return crc;
        hipStream_t st = w->stream;
        CqPair *d_pairs = reinterpret_cast<CqPair *>(w->z.as<uint8_t>() + rs.end_off<RecoverTables>());
        const RecoverBlob *d_desc;
        if (P) HIPCHK(hipMemcpyAsync(d_pairs, ch.pairs.data(), sizeof(CqPair) * P, hipMemcpyHostToDevice, st));
        if ((crc = rc_field_stage(w, tm, cc, rs, (int)mc, ch.any_refused ? ch.refused.data() : nullptr, cells, device, proofs_out, cells_out, &d_desc)))
            return crc;
        if (cells_out && P) {
            tm.begin("rc_cells_at");
            launch_rc_cells_at(w->scal_b.as<Fr>(), d_desc, d_pairs, (int)P, cc, device ? cells_at : w->records.as<uint8_t>(), st);
            tm.end();
            if (!device && (crc = cq_cells_to_host(w, ch, cells_at))) return crc;
        }
        if (proofs_out && P && (crc = cq_proofs(s, w, tm, cc, ch, d_pairs, proofs_at, device))) return crc;
        if ((crc = cq_finish(w, tm, ch, wcounts + c0, device ? nullptr : proofs_at, status ? status + c0 : nullptr, first))) return crc;
        koff += rs.known;
    }
    return KZG355_OK;
    };
    if ((rc = run())) return refuse(rc);
    return first;
}

static int ra_impl(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *kcounts, const size_t *kidx, const uint8_t *cells,
                   const size_t *wcounts, const size_t *widx, size_t m, const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, m, code); };
    if (!cs || (!cells_out && !proofs_out)) return refuse(KZG355_BADARGS);
    if (m == 0) return KZG355_OK;
    if (!kcounts || !wcounts || !kidx || !cells || m > ((size_t)1 << 32)) return refuse(KZG355_BADARGS);
    if (device && misaligned(cells_out, proofs_out, cells)) return refuse(KZG355_BADARGS);
    size_t known = 0, wanted = 0;
    if (!sum_counts(known, kcounts, m) || !sum_counts(wanted, wcounts, m) || (wanted && !widx)) return refuse(KZG355_BADARGS);
    if (cs->multi && !device) {                                   // ranges of blobs over the replicas: each starts at its own two prefix sums
        const std::vector<size_t> kfirst = prefix_sums(kcounts, m), wfirst = prefix_sums(wcounts, m);
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
