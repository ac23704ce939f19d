// cell_recover.hip -- the C entry points of recover_cells_and_kzg_proofs (EIP-7594 cells; include/kzg355.h; host side of libkzg355.so, see
// engine.h).  The host checks the index set, copies the known cells in and cells / proofs out and sets the statuses.  The erasure decoding runs
// in the kernels of k_cell_recover.hip and leaves, per blob, what the field stage of compute_cells_and_kzg_proofs leaves: the coefficients and
// the 128 cells.  The chunk loop and the proofs are that call's own (cell_compute.hip: cc_run).
#include "engine.h"

namespace kzg355_impl {

// cells: m blobs of n cells each, the cells of a blob at the n strictly ascending indices idx (one set for all blobs; always host memory).
// device: cells, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where they are
static int rc_impl(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *idx, const uint8_t *cells, size_t n, size_t m,
                   const kzg355_settings *cs, bool device = false) {
    auto refuse = [&](int code) { return cc_refuse(status, m, code); };
    if (!cs || (!cells_out && !proofs_out)) return refuse(KZG355_BADARGS);
    if (n < (size_t)CELLS_PER_EXT_BLOB / 2 || n > (size_t)CELLS_PER_EXT_BLOB || !idx) return refuse(KZG355_BADARGS);
    int pos[CELLS_PER_EXT_BLOB];
    for (int k = 0; k < CELLS_PER_EXT_BLOB; k++) pos[k] = -1;
    for (size_t i = 0; i < n; i++) {
        if (idx[i] >= (size_t)CELLS_PER_EXT_BLOB || (i && idx[i] <= idx[i - 1])) return refuse(KZG355_BADARGS);
        pos[idx[i]] = (int)i;
    }
    if (m == 0) return KZG355_OK;
    if (!cells) return refuse(KZG355_BADARGS);
    if (device && (((uintptr_t)cells_out & 15) || ((uintptr_t)proofs_out & 15) || ((uintptr_t)cells & 15))) return refuse(KZG355_BADARGS);
    const size_t in_bytes = (size_t)CELL_BYTES * n;               // per blob
    return cc_run(cs, m, cells_out, proofs_out, nullptr, status,
        // the workspace's buffers by role: blobs = known cells, z = the call's tables, scal_b = u (cell interpolants, then P_r(a_k))
        [&](Workspace *w, size_t CH) {
            int rc;
            if ((!device && (rc = w->blobs.ensure(in_bytes * CH))) || (rc = w->z.ensure(sizeof(RecoverTables)))) return rc;
            return w->scal_b.ensure(sizeof(Fr) * CELLS_PER_EXT_BLOB * CELL_FE * CH);
        },
        [&](Workspace *w, Timed &tm, size_t c0, int mc, uint8_t *d_cells) -> int {
            const CellComputeConsts *cc = cs->cc_consts.as<CellComputeConsts>();
            RecoverTables *rt = w->z.as<RecoverTables>();
            hipStream_t st = w->stream;
            const uint8_t *d_known = device ? cells + in_bytes * c0 : w->blobs.as<uint8_t>();
            if (!device) HIPCHK(hipMemcpyAsync(w->blobs.p, cells + in_bytes * c0, in_bytes * mc, hipMemcpyHostToDevice, st));
            if (c0 == 0) {
                HIPCHK(hipMemcpyAsync(rt->pos, pos, sizeof(pos), hipMemcpyHostToDevice, st));
                tm.begin("rc_vanish");
                launch_rc_vanish(cc, rt, st);
                tm.end();
            }
            tm.begin("rc_interp");
            launch_rc_interp(d_known, (int)n, mc, cc, rt, w->scal_b.as<Fr>(), w->err.as<int>(), st);
            tm.end();
            tm.begin("rc_columns");
            launch_rc_columns(w->scal_b.as<Fr>(), mc, cc, rt, proofs_out ? w->y.as<Fr>() : nullptr, cells_out != nullptr, st);
            tm.end();
            if (cells_out) {
                tm.begin("rc_cells");
                launch_rc_cells(w->scal_b.as<Fr>(), mc, cc, d_cells, st);
                tm.end();
            }
            return KZG355_OK;
        }, device);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_recover_cells_and_kzg_proofs_many(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *cell_indices, const uint8_t *cells,
                                             size_t n, size_t m, const kzg355_settings *s) {
    return rc_impl(cells_out, proofs_out, status, cell_indices, cells, n, m, s);
}

int kzg355_recover_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const size_t *cell_indices,
                                                    const uint8_t *d_cells, size_t n, size_t m, const kzg355_settings *s) {
    return rc_impl(d_cells_out, d_proofs_out, status, cell_indices, d_cells, n, m, s, true);
}

int kzg355_recover_cells_and_kzg_proofs(uint8_t *cells_out, uint8_t *proofs_out, const size_t *cell_indices, const uint8_t *cells, size_t n,
                                        const kzg355_settings *s) {
    return rc_impl(cells_out, proofs_out, nullptr, cell_indices, cells, n, 1, s);
}

#pragma GCC visibility pop
}  // extern "C"
