// cell_recover.hip -- the C entry points of recover_cells_and_kzg_proofs (EIP-7594 cells; include/kzg355.h; host side of libkzg355.so, see
// engine.h).  The host checks the index set, copies the known cells in and cells / proofs out and sets the statuses.  The erasure decoding runs
// in the kernels of k_cell_recover.hip and leaves, per blob, what the field stage of compute_cells_and_kzg_proofs leaves: the coefficients and
// the 128 cells.  The proofs come from that call's own chain (cell_compute.hip: cc_proof_chain).
#include "engine.h"

namespace kzg355_impl {

// cells: m blobs of n cells each, the cells of a blob at the n strictly ascending indices idx (one set for all blobs)
static int rc_impl(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *idx, const uint8_t *cells, size_t n, size_t m,
                   const kzg355_settings *cs) {
    auto refuse = [&](int code) { if (status) for (size_t i = 0; i < m; i++) status[i] = code; return code; };
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
    if (m > ((size_t)1 << 32)) return refuse(KZG355_BADARGS);
    if (is_small(cs)) return refuse(KZG355_BADARGS);             // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    if ((rc = ensure_cc_consts(s, w))) return refuse(rc);
    if (proofs_out && (rc = ensure_cc_proof_setup(s, w))) return refuse(rc);
    const size_t CH = m < CC_CHUNK ? m : CC_CHUNK;
    const size_t in_bytes = (size_t)CELL_BYTES * n;               // per blob
    // the workspace's buffers by role: blobs = known cells, z = the call's tables, scal_b = u (cell interpolants, then P_r(a_k)); then cc_chain_buffers'
    if ((rc = w->blobs.ensure(in_bytes * CH)) || (rc = w->z.ensure(sizeof(RecoverTables))) ||
        (rc = w->scal_b.ensure(sizeof(Fr) * CELLS_PER_EXT_BLOB * CELL_FE * CH)) || (rc = cc_chain_buffers(w, CH, cells_out, proofs_out, false)))
        return refuse(rc);
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    RecoverTables *rt = w->z.as<RecoverTables>();
    hipStream_t st = w->stream;
    Timed tm(s, w);
    int first = KZG355_OK;
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    for (size_t c0 = 0; c0 < m; c0 += CH) {
        const int mc = (int)(m - c0 < CH ? m - c0 : CH);
        w->in_flight = true;
        HIPCHK(hipMemsetAsync(w->err.p, 0, sizeof(int) * mc, st));
        HIPCHK(hipMemcpyAsync(w->blobs.p, cells + in_bytes * c0, in_bytes * mc, hipMemcpyHostToDevice, st));
        if (c0 == 0) {
            HIPCHK(hipMemcpyAsync(rt->pos, pos, sizeof(pos), hipMemcpyHostToDevice, st));
            tm.begin("rc_vanish");
            launch_rc_vanish(cc, rt, st);
            tm.end();
        }
        tm.begin("rc_interp");
        launch_rc_interp(w->blobs.as<uint8_t>(), (int)n, mc, cc, rt, w->scal_b.as<Fr>(), w->err.as<int>(), st);
        tm.end();
        tm.begin("rc_columns");
        launch_rc_columns(w->scal_b.as<Fr>(), mc, cc, rt, proofs_out ? w->y.as<Fr>() : nullptr, cells_out != nullptr, st);
        tm.end();
        if (cells_out) {
            tm.begin("rc_cells");
            launch_rc_cells(w->scal_b.as<Fr>(), mc, cc, w->q.as<uint8_t>(), st);
            tm.end();
        }
        if (proofs_out) cc_proof_chain(s, w, tm, mc, false);
        int crc;
        if ((crc = cc_collect_chunk(w, tm, cells_out, proofs_out, nullptr, status, c0, mc, first))) return crc;
    }
    return KZG355_OK;
    };
    if ((rc = run())) return refuse(rc);
    return first;
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_recover_cells_and_kzg_proofs_many(uint8_t *cells_out, uint8_t *proofs_out, int *status, const size_t *cell_indices, const uint8_t *cells,
                                             size_t n, size_t m, const kzg355_settings *s) {
    return rc_impl(cells_out, proofs_out, status, cell_indices, cells, n, m, s);
}

int kzg355_recover_cells_and_kzg_proofs(uint8_t *cells_out, uint8_t *proofs_out, const size_t *cell_indices, const uint8_t *cells, size_t n,
                                        const kzg355_settings *s) {
    return rc_impl(cells_out, proofs_out, nullptr, cell_indices, cells, n, 1, s);
}

#pragma GCC visibility pop
}  // extern "C"
