// cell_recover.hip -- the C entry points of recover_cells_and_kzg_proofs (EIP-7594 cells; include/kzg355.h; host side of libkzg355.so, see
// engine.h).  The host checks the index sets, copies the known cells in and cells / proofs out and sets the statuses.  The erasure decoding runs
// in the kernels of k_cell_recover.hip and leaves, per blob, what the field stage of compute_cells_and_kzg_proofs leaves: the coefficients and
// the 128 cells.  The chunk loop and the proofs are that call's own (cell_compute.hip: cc_run).
#include "engine.h"

namespace kzg355_impl {

static const size_t RC_CELLS_OUT = (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES, RC_PROOFS_OUT = (size_t)48 * CC_FFT;   // bytes of output per blob

// The field stage of a recover chunk as rs laid it out (engine.h).  Also the first half of recover_cells_and_kzg_proofs_at (cell_recover_at.hip).
int rc_field_stage(Workspace *w, Timed &tm, const CellComputeConsts *cc, const RecoverStage &rs, int mc, const int *refused, const uint8_t *cells,
                   bool device, bool want_coef, bool want_cells, const RecoverBlob **d_desc) {
    hipStream_t st = w->stream;
    RecoverTables *rt = w->z.as<RecoverTables>();
    uint64_t *d_up = reinterpret_cast<uint64_t *>(w->z.as<uint8_t>() + rs.masks_off<RecoverTables>());
    *d_desc = reinterpret_cast<const RecoverBlob *>(w->z.as<uint8_t>() + rs.desc_off<RecoverTables>());
    size_t dst = 0;
    for (const auto &c : rs.copies) {
        HIPCHK(hipMemcpyAsync(w->blobs.as<uint8_t>() + dst * CELL_BYTES, cells + c.first * CELL_BYTES, c.second * CELL_BYTES, hipMemcpyHostToDevice, st));
        dst += c.second;
    }
    HIPCHK(hipMemcpyAsync(d_up, rs.up.data(), rs.up_bytes(), hipMemcpyHostToDevice, st));
    if (refused) HIPCHK(hipMemcpyAsync(w->err.p, refused, sizeof(int) * mc, hipMemcpyHostToDevice, st));
    const uint8_t *d_known = device ? cells + rs.base * CELL_BYTES : w->blobs.as<uint8_t>();
    tm.begin("rc_vanish");
    launch_rc_vanish(cc, d_up, (int)rs.sets.size(), rt, st);
    tm.end();
    tm.begin("rc_interp");
    launch_rc_interp(d_known, *d_desc, mc, cc, rt, w->scal_b.as<Fr>(), w->err.as<int>(), st);
    tm.end();
    tm.begin("rc_columns");
    launch_rc_columns(w->scal_b.as<Fr>(), *d_desc, mc, cc, rt, want_coef ? w->y.as<Fr>() : nullptr, want_cells, st);
    tm.end();
    return KZG355_OK;
}

// What every recover call runs, once its arguments are checked (m > 0).  counts null: the shared-set calls, every blob known at the n indices
// idx (a valid list).  Otherwise blob i is known at counts[i] cells and its index list and cells start counts[0] + .. + counts[i-1] entries
// into idx and cells (the sum does not overflow); a blob whose list is refused gets KZG355_BADARGS and the others do not notice.
// Per chunk w->z holds, one after the other: the chunk's tables, the masks of its sets and the descriptors of its blobs (cell_plan.h).
// device: cells, commitments_out, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where
// they are.  commitments_out (or null): 48 bytes per blob, the commitment of the coefficients the decoding keeps (conv[63] of the FK20 chain).
static int rc_run(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *counts, const size_t *idx, size_t n,
                  const uint8_t *cells, size_t m, const kzg355_settings *cs, bool device) {
    uint64_t shared_mask[2] = {0, 0};
    if (!counts) rc_mask(shared_mask, idx, n);
    std::unique_ptr<RecoverStage> rs;                            // made for the call's chunk size
    size_t next = 0;                                             // the call's cells before the chunk about to be staged
    std::vector<int> refused;                                    // the chunk's err words, when the host refuses one of its blobs
    return cc_run(cs, m, commitments_out, cells_out, proofs_out, nullptr, status,
        // the workspace's buffers by role: blobs = known cells, z = tables, masks and descriptors, scal_b = u (cell interpolants, then P_r(a_k))
        [&](Workspace *w, size_t CH) {
            rs.reset(new RecoverStage(CH, counts ? CH : 1));
            int rc;
            if ((!device && (rc = w->blobs.ensure((size_t)CELL_BYTES * (counts ? (size_t)CELLS_PER_EXT_BLOB : n) * CH))) ||
                (rc = w->z.ensure(rs->end_off<RecoverTables>())))
                return rc;
            return w->scal_b.ensure(sizeof(Fr) * CELLS_PER_EXT_BLOB * CELL_FE * CH);
        },
        [&](Workspace *w, Timed &tm, size_t c0, int mc, uint8_t *d_cells, bool want_coef) -> int {
            const CellComputeConsts *cc = cs->cc_consts.as<CellComputeConsts>();
            bool any_refused = false;
            refused.assign(mc, 0);
            rs->reset(next);
            for (int b = 0; b < mc; b++) {
                const size_t cnt = counts ? counts[c0 + b] : n;
                uint64_t mask[2] = {shared_mask[0], shared_mask[1]};
                const bool good = !counts || rc_mask(mask, idx + next, cnt);
                if (!good) refused[b] = ERR_NONCANONICAL_FR;     // any err word is this blob's KZG355_BADARGS (status_from_err)
                any_refused |= !good;
                rs->add(good, mask, cnt, device);
                next += cnt;
            }
            const RecoverBlob *d_desc;
            int rc;
            if ((rc = rc_field_stage(w, tm, cc, *rs, mc, any_refused ? refused.data() : nullptr, cells, device, want_coef, cells_out, &d_desc))) return rc;
            if (cells_out) {
                tm.begin("rc_cells");
                launch_rc_cells(w->scal_b.as<Fr>(), d_desc, mc, cc, d_cells, w->stream);
                tm.end();
            }
            return KZG355_OK;
        }, device);
}

// m blobs of n cells each, the cells of a blob at the n strictly ascending indices idx (one set for all blobs; always host memory)
static int rc_shared(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *idx, const uint8_t *cells, size_t n,
                     size_t m, const kzg355_settings *cs, bool device = false) {
    auto refuse = [&](int code) { return refuse_call(status, m, code); };
    if (!cs || (!commitments_out && !cells_out && !proofs_out)) return refuse(KZG355_BADARGS);
    uint64_t mask[2];
    if (!idx || !rc_mask(mask, idx, n)) return refuse(KZG355_BADARGS);
    if (m == 0) return KZG355_OK;
    if (!cells) return refuse(KZG355_BADARGS);
    if (device && misaligned(commitments_out, cells_out, proofs_out, cells)) return refuse(KZG355_BADARGS);
    if (cs->multi && !device)                                     // ranges of blobs over the replicas (cc_fan_out)
        return cc_fan_out(cs, m, status, [&](const kzg355_settings *rep, size_t u0, size_t k) {
            return rc_run(commitments_out ? commitments_out + 48 * u0 : nullptr, cells_out ? cells_out + RC_CELLS_OUT * u0 : nullptr,
                          proofs_out ? proofs_out + RC_PROOFS_OUT * u0 : nullptr, status ? status + u0 : nullptr, nullptr, idx, n,
                          cells + (size_t)CELL_BYTES * n * u0, k, rep, false);
        });
    return rc_run(commitments_out, cells_out, proofs_out, status, nullptr, idx, n, cells, m, cs, device);
}

// m blobs, blob i known at counts[i] cells: its index list and its cells follow those of blob i - 1 in idx and cells
static int rc_sets(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *counts, const size_t *idx,
                   const uint8_t *cells, size_t m, const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, m, code); };
    if (!cs || (!commitments_out && !cells_out && !proofs_out)) return refuse(KZG355_BADARGS);
    if (m == 0) return KZG355_OK;
    if (!counts || !idx || !cells || m > ((size_t)1 << 32)) return refuse(KZG355_BADARGS);
    if (device && misaligned(commitments_out, cells_out, proofs_out, cells)) return refuse(KZG355_BADARGS);
    size_t total;
    if (!sum_counts(total, counts, m)) return refuse(KZG355_BADARGS);
    if (cs->multi && !device) {                                   // ranges of blobs over the replicas: a range's indices and cells start at the sum of the counts before it
        const std::vector<size_t> first = prefix_sums(counts, m);
        return cc_fan_out(cs, m, status, [&](const kzg355_settings *rep, size_t u0, size_t k) {
            return rc_run(commitments_out ? commitments_out + 48 * u0 : nullptr, cells_out ? cells_out + RC_CELLS_OUT * u0 : nullptr,
                          proofs_out ? proofs_out + RC_PROOFS_OUT * u0 : nullptr, status ? status + u0 : nullptr, counts + u0, idx + first[u0], 0,
                          cells + (size_t)CELL_BYTES * first[u0], k, rep, false);
        });
    }
    return rc_run(commitments_out, cells_out, proofs_out, status, counts, idx, 0, cells, m, cs, device);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_recover_cells_and_kzg_proofs_many(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *cell_indices, const uint8_t *cells,
                                             size_t n, size_t m, const kzg355_settings *s) {
    return rc_shared(nullptr, cells_out, proofs_out, status, cell_indices, cells, n, m, s);
}

int kzg355_recover_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const size_t *cell_indices,
                                                    const uint8_t *d_cells, size_t n, size_t m, const kzg355_settings *s) {
    return rc_shared(nullptr, d_cells_out, d_proofs_out, status, cell_indices, d_cells, n, m, s, true);
}

int kzg355_recover_cells_and_kzg_proofs(uint8_t *cells_out, uint8_t *proofs_out, const size_t *cell_indices, const uint8_t *cells, size_t n,
                                        const kzg355_settings *s) {
    return rc_shared(nullptr, cells_out, proofs_out, nullptr, cell_indices, cells, n, 1, s);
}

int kzg355_recover_cells_and_kzg_proofs_many_sets(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *cell_counts,
                                                  const size_t *cell_indices, const uint8_t *cells, size_t m, const kzg355_settings *s) {
    return rc_sets(nullptr, cells_out, proofs_out, status, cell_counts, cell_indices, cells, m, s, false);
}

int kzg355_recover_cells_and_kzg_proofs_many_sets_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const size_t *cell_counts,
                                                         const size_t *cell_indices, const uint8_t *d_cells, size_t m, const kzg355_settings *s) {
    return rc_sets(nullptr, d_cells_out, d_proofs_out, status, cell_counts, cell_indices, d_cells, m, s, true);
}

int kzg355_recover_commitments_cells_and_kzg_proofs_many(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, int *status,
                                                         const size_t *cell_indices, const uint8_t *cells, size_t n, size_t m, const kzg355_settings *s) {
    return rc_shared(commitments_out, cells_out, proofs_out, status, cell_indices, cells, n, m, s);
}

int kzg355_recover_commitments_cells_and_kzg_proofs_many_device(uint8_t *d_commitments_out, uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status,
                                                                const size_t *cell_indices, const uint8_t *d_cells, size_t n, size_t m,
                                                                const kzg355_settings *s) {
    return rc_shared(d_commitments_out, d_cells_out, d_proofs_out, status, cell_indices, d_cells, n, m, s, true);
}

int kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, int *status,
                                                              const size_t *cell_counts, const size_t *cell_indices, const uint8_t *cells, size_t m,
                                                              const kzg355_settings *s) {
    return rc_sets(commitments_out, cells_out, proofs_out, status, cell_counts, cell_indices, cells, m, s, false);
}

int kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(uint8_t *d_commitments_out, uint8_t *d_cells_out, uint8_t *d_proofs_out,
                                                                     int *status, const size_t *cell_counts, const size_t *cell_indices,
                                                                     const uint8_t *d_cells, size_t m, const kzg355_settings *s) {
    return rc_sets(d_commitments_out, d_cells_out, d_proofs_out, status, cell_counts, cell_indices, d_cells, m, s, true);
}

#pragma GCC visibility pop
}  // extern "C"
