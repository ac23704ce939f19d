// cell_compute.hip -- the C entry points of compute_cells_and_kzg_proofs (EIP-7594 cells; include/kzg355.h) and the per-handle setup they need
// (host side of libkzg355.so; see engine.h).  The host copies blobs in and cells / proofs out and sets the statuses; every field and group
// operation runs in the kernels of k_cell_compute.hip, one set of launches per chunk of blobs.  The chunk loop (cc_run) also serves
// recover_cells_and_kzg_proofs (cell_recover.hip), and the builder of the monomial points the setup of verify_cell_kzg_proof_batch (cells.hip).
#include "engine.h"

namespace kzg355_impl {

// Constants of the field stage (w4096 powers, twiddle splits): the first compute call of a handle.  Under cc_mu.
int ensure_cc_consts(kzg355_settings *s, Workspace *w) {
    std::lock_guard<std::mutex> lk(s->cc_mu);
    if (s->cc_consts_ready) return KZG355_OK;
    int rc;
    if ((rc = s->cc_consts.ensure(sizeof(CellComputeConsts)))) return rc;
    launch_cc_consts(s->t.roots, s->cc_consts.as<CellComputeConsts>(), w->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(w->stream));
    s->cc_consts_ready = true;
    return KZG355_OK;
}

// The monomial points [tau^t]_1 = sum_i w_i^t [L_i(tau)]_1, t < count (a multiple of 64), for the setups of the cell paths: the commitments of the
// "blobs" (w_i^t)_i through the 8-bit fixed-base MSM of the commitment path, 64 at a time, compressed into d_mono48 and decoded into d_mono.  The
// scratch is this function's own and is released on every path; the caller holds its setup mutex and owns the two buffers.
int build_monomial_points(kzg355_settings *s, Workspace *w, int count, uint8_t *d_mono48, G1Affine *d_mono) {
    DevBuf scal, digits, partials, err;
    auto done = [&](int rc) { for (DevBuf *b : {&scal, &digits, &partials, &err}) b->release(); return rc; };
    int rc;
    if ((rc = scal.ensure(sizeof(Fr) * CELL_FE * N_FE)) || (rc = digits.ensure((size_t)CELL_FE * MSM_WINDOWS * N_FE)) ||
        (rc = partials.ensure(sizeof(G1Jac) * CELL_FE * MSM_WINDOWS)) || (rc = err.ensure(sizeof(int))))
        return done(rc);
    hipStream_t st = w->stream;
    auto hip_fail = [&]() { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return done(KZG355_DEVICE_ERROR); };
    if (hipMemsetAsync(err.p, 0, sizeof(int), st) != hipSuccess) return hip_fail();
    for (int t0 = 0; t0 < count; t0 += CELL_FE) launch_monomial_chunk(s->t, t0, scal.as<Fr>(), digits.as<uint8_t>(), partials.as<G1Jac>(), d_mono48, st);
    launch_monomial_decode(d_mono48, count, d_mono, err.as<int>(), st);
    int herr = 0;
    uint8_t first[48];
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(first, d_mono48, 48, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return hip_fail();
    // [tau^0]_1 = sum_i [L_i(tau)]_1 = G1: the derived points start at the generator whatever the ceremony
    if (herr || memcmp(first, G1_GEN, 48) != 0) return done(KZG355_INTERNAL);
    return done(KZG355_OK);
}

// The proof setup, on the first call that wants proofs (after ensure_cc_consts): the 4096 monomial points, X_r = NTT128(x_r) and their comb table.
// Under cc_mu.  A failure releases what was being filled; every failure but NO_MEMORY is remembered (engine.h, at cc_mu).
static int ensure_cc_proof_setup(kzg355_settings *s, Workspace *w) {
    std::lock_guard<std::mutex> lk(s->cc_mu);
    if (s->cc_proof_ready) return s->cc_proof_rc;
    DevBuf X;
    auto done = [&](int rc) {
        X.release();
        if (rc != KZG355_OK) for (DevBuf *b : {&s->cc_mono48, &s->cc_mono, &s->cc_table}) b->release();
        if (rc == KZG355_NO_MEMORY) return rc;                     // not remembered: a later call may find the memory
        s->cc_proof_ready = true;
        s->cc_proof_rc = rc;
        return rc;
    };
    int rc;
    if ((rc = s->cc_mono48.ensure(48 * (size_t)N_FE)) || (rc = s->cc_mono.ensure(sizeof(G1Affine) * N_FE)) ||
        (rc = s->cc_table.ensure(sizeof(G1Affine) * CC_TABLE_ENTRIES)) || (rc = X.ensure(sizeof(G1Jac) * CC_POINTS)) ||
        (rc = build_monomial_points(s, w, N_FE, s->cc_mono48.as<uint8_t>(), s->cc_mono.as<G1Affine>())))
        return done(rc);
    launch_cc_setup_points(s->cc_mono.as<G1Affine>(), s->cc_consts.as<CellComputeConsts>(), X.as<G1Jac>(), s->cc_table.as<G1Affine>(), w->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) {
        (void)hipStreamSynchronize(w->stream); (void)hipGetLastError();
        return done(KZG355_DEVICE_ERROR);
    }
    return done(KZG355_OK);
}

// The device chain behind the field stage.  compute_cells_and_kzg_proofs and recover_cells_and_kzg_proofs (cell_recover.hip) differ in their field
// stage only, and both leave the same two things on the device: coefficients in w->y and cells in w->q.  The workspace's buffers by role:
// y = coefficients, scal_a = column scalars, partials = Z, q = cells, out48 = proofs, small = H, commitments = commitments.
// want_chain: proofs, H or commitments are wanted.  out48 only when proofs (or H, which leaves them there) stay in the workspace (ws_proofs),
// commitments only when they go to the host (ws_commit).  With dev_out the cells, proofs and commitments go straight into the caller's device
// buffers and q is not needed.
static int cc_chain_buffers(Workspace *w, size_t CH, bool want_cells, bool want_chain, bool want_h, bool dev_out, bool ws_proofs, bool ws_commit) {
    int rc;
    if ((rc = w->err.ensure(sizeof(int) * CH)) || (rc = w->h_err.ensure(sizeof(int) * CH)) ||
        (want_cells && !dev_out && (rc = w->q.ensure((size_t)CELLS_PER_EXT_BLOB * CELL_BYTES * CH))) ||
        (want_chain && ((rc = w->y.ensure(sizeof(Fr) * N_FE * CH)) || (rc = w->scal_a.ensure(sizeof(uint32_t) * 8 * CC_FFT * CELL_FE * CH)) ||
                        (rc = w->partials.ensure(sizeof(G1Jac) * CC_FFT * CH)) || (ws_proofs && (rc = w->out48.ensure((size_t)48 * CC_FFT * CH))) ||
                        (ws_commit && (rc = w->commitments.ensure((size_t)48 * CH))))) ||
        (want_h && (rc = w->small.ensure((size_t)48 * CELL_FE * CH))))
        return rc;
    return KZG355_OK;
}
// coefficients of m blobs in w->y -> proofs in d_proofs (w->out48, or the caller's device buffer at the chunk's offset; null: none wanted; and H
// in w->small) and commitments in d_commit (w->commitments or the caller's device buffer; null: none wanted), queued on w->stream
static void cc_proof_chain(kzg355_settings *s, Workspace *w, Timed &tm, int m, bool want_h, uint8_t *d_proofs, uint8_t *d_commit) {
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    hipStream_t st = w->stream;
    tm.begin("cc_columns");
    launch_cc_columns(w->y.as<Fr>(), m, cc, w->scal_a.as<uint32_t>(), st);
    tm.end();
    tm.begin("cc_msm");
    launch_cc_msm(w->scal_a.as<uint32_t>(), m, s->cc_table.as<G1Affine>(), w->partials.as<G1Jac>(), st);
    tm.end();
    tm.begin("cc_proofs");
    launch_cc_proofs(w->partials.as<G1Jac>(), m, cc, d_proofs, want_h ? w->small.as<uint8_t>() : nullptr, d_commit, st);
    tm.end();
}
// the results of a chunk of m blobs (blob c0 onwards) back to the host (dev_out: they are in the caller's device buffers already), the wait, and
// the per-blob statuses
static int cc_collect_chunk(Workspace *w, Timed &tm, uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, uint8_t *h_dbg, int *status,
                            size_t c0, int m, int &first, bool dev_out) {
    const size_t cell_bytes = (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES;
    hipStream_t st = w->stream;
    HIPCHK(hipGetLastError());
    int rc;
    if ((rc = launch_set_results(w, m))) return rc;
    if (commitments_out && !dev_out) HIPCHK(hipMemcpyAsync(commitments_out + 48 * c0, w->commitments.p, (size_t)48 * m, hipMemcpyDeviceToHost, st));
    if (cells_out && !dev_out) HIPCHK(hipMemcpyAsync(cells_out + cell_bytes * c0, w->q.p, cell_bytes * m, hipMemcpyDeviceToHost, st));
    if (proofs_out && !dev_out) HIPCHK(hipMemcpyAsync(proofs_out + (size_t)48 * CC_FFT * c0, w->out48.p, (size_t)48 * CC_FFT * m, hipMemcpyDeviceToHost, st));
    if (h_dbg) HIPCHK(hipMemcpyAsync(h_dbg + (size_t)48 * CELL_FE * c0, w->small.p, (size_t)48 * CELL_FE * m, hipMemcpyDeviceToHost, st));
    if ((rc = launch_set_wait(w, tm))) return rc;
    rc = launch_set_read(w, m, status ? status + c0 : nullptr);
    if (first == KZG355_OK) first = rc;
    return KZG355_OK;
}

int cell_call_begin(const kzg355_settings *cs, size_t units, std::unique_ptr<WsGuard> &g, int (*second_setup)(kzg355_settings *, Workspace *)) {
    if (units > ((size_t)1 << 32) || is_small(cs)) return KZG355_BADARGS;     // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    g.reset(new WsGuard(cs));
    if (!g->w) return KZG355_NO_DEVICE;
    int rc;
    if ((rc = ensure_cc_consts(g->s, g->w)) || (second_setup && (rc = second_setup(g->s, g->w)))) return rc;
    g->s->n_cell_sets.fetch_add(1);
    return KZG355_OK;
}

// What the two calls share once the caller has checked its own arguments (`units` > 0 blobs, some output wanted): the remaining refusals, the
// setups, and the chunk loop.  `reserve` sizes the caller's own workspace buffers for CH blobs; `stage` copies the input of blobs c0 .. c0 + m - 1
// in (or reads it where it is, for device-resident input) and queues the kernels that leave their coefficients in w->y (want_chain: proofs, H
// or commitments are wanted) and their cells in the d_cells it is handed (when cells are; null otherwise).
// commitments_out / cells_out / proofs_out: host memory, or with dev_out device memory on the handle's device, 16-byte aligned (the kernels then
// write there at the chunk's offset: no copy); h_dbg: host memory (any of the four may be null, not all); status (or null): per blob, host.
int cc_run(const kzg355_settings *cs, size_t units, uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, uint8_t *h_dbg, int *status,
           const std::function<int(Workspace *, size_t)> &reserve,
           const std::function<int(Workspace *, Timed &, size_t, int, uint8_t *, bool)> &stage, bool dev_out) {
    auto refuse = [&](int code) { return refuse_call(status, units, code); };
    const bool want_chain = proofs_out || h_dbg || commitments_out;
    const bool dev_proofs = dev_out && proofs_out, ws_proofs = (proofs_out || h_dbg) && !dev_proofs;
    std::unique_ptr<WsGuard> g;
    int rc;
    if ((rc = cell_call_begin(cs, units, g, want_chain ? ensure_cc_proof_setup : nullptr))) return refuse(rc);
    kzg355_settings *s = g->s; Workspace *w = g->w;
    const size_t CH = units < CC_CHUNK ? units : CC_CHUNK;
    if ((rc = reserve(w, CH)) || (rc = cc_chain_buffers(w, CH, cells_out, want_chain, h_dbg, dev_out, ws_proofs, commitments_out && !dev_out)))
        return refuse(rc);
    const size_t cell_bytes = (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES;
    Timed tm(s, w);
    int first = KZG355_OK;
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    for (size_t c0 = 0; c0 < units; c0 += CH) {
        const int m = (int)(units - c0 < CH ? units - c0 : CH);
        int crc;
        if ((crc = launch_set_begin(w, m))) return crc;           // (cc_chain_buffers has sized the words for CH)
        uint8_t *d_cells = !cells_out ? nullptr : dev_out ? cells_out + cell_bytes * c0 : w->q.as<uint8_t>();
        uint8_t *d_proofs = dev_proofs ? proofs_out + (size_t)48 * CC_FFT * c0 : ws_proofs ? w->out48.as<uint8_t>() : nullptr;
        uint8_t *d_commit = !commitments_out ? nullptr : dev_out ? commitments_out + 48 * c0 : w->commitments.as<uint8_t>();
        if ((crc = stage(w, tm, c0, m, d_cells, want_chain))) return crc;
        if (want_chain) cc_proof_chain(s, w, tm, m, h_dbg, d_proofs, d_commit);
        if ((crc = cc_collect_chunk(w, tm, commitments_out, cells_out, proofs_out, h_dbg, status, c0, m, first, dev_out))) return crc;
    }
    return KZG355_OK;
    };
    if ((rc = run())) return refuse(rc);
    return first;
}

// The host-buffer compute and recover calls on a handle over several devices (multi_device.hip): what cc_run would refuse for every range alike
// is refused here, once; then contiguous ranges of the blobs go to as many replicas as there are blobs, fn(replica, first blob, count) on the
// replica's own host thread (cc_run takes its workspace and scopes its device there).  A blob is never cut.
int cc_fan_out(const kzg355_settings *cs, size_t units, int *status, const std::function<int(const kzg355_settings *, size_t, size_t)> &fn) {
    if (units > ((size_t)1 << 32) || is_small(cs)) return refuse_call(status, units, KZG355_BADARGS);
    const size_t D = cs->multi->rep.size();
    return fan_out(cs, units < D ? units : D, units, fn);
}

// n blobs on the device of cs (a replica, for a handle over several devices); the arguments are checked
static int cc_single(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, uint8_t *h_dbg, int *status, const uint8_t *blobs, size_t n,
                     const kzg355_settings *cs, bool device) {
    return cc_run(cs, n, commitments_out, cells_out, proofs_out, h_dbg, status,
        [&](Workspace *w, size_t CH) { return device ? KZG355_OK : w->blobs.ensure((size_t)BLOB_BYTES * CH); },
        [&](Workspace *w, Timed &tm, size_t c0, int m, uint8_t *d_cells, bool want_coef) -> int {
            const uint8_t *d_blobs = device ? blobs + (size_t)BLOB_BYTES * c0 : w->blobs.as<uint8_t>();
            if (!device) HIPCHK(hipMemcpyAsync(w->blobs.p, blobs + (size_t)BLOB_BYTES * c0, (size_t)BLOB_BYTES * m, hipMemcpyHostToDevice, w->stream));
            tm.begin("cc_field");
            launch_cc_field(d_blobs, m, cs->cc_consts.as<CellComputeConsts>(), want_coef ? w->y.as<Fr>() : nullptr, d_cells, w->err.as<int>(),
                            w->stream);
            tm.end();
            return KZG355_OK;
        }, device);
}

// device: blobs, commitments_out, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where
// they are -- on the first device of a handle over several, where they live
static int cc_impl(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, uint8_t *h_dbg, int *status, const uint8_t *blobs, size_t n,
                   const kzg355_settings *cs, bool device = false) {
    if (!cs || (!commitments_out && !cells_out && !proofs_out && !h_dbg)) return refuse_call(status, n, KZG355_BADARGS);
    if (n == 0) return KZG355_OK;
    if (!blobs) return refuse_call(status, n, KZG355_BADARGS);
    if (device && misaligned(commitments_out, cells_out, proofs_out, blobs)) return refuse_call(status, n, KZG355_BADARGS);
    if (cs->multi && !device)
        return cc_fan_out(cs, n, status, [&](const kzg355_settings *rep, size_t u0, size_t k) {
            return cc_single(commitments_out ? commitments_out + 48 * u0 : nullptr,
                             cells_out ? cells_out + (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES * u0 : nullptr,
                             proofs_out ? proofs_out + (size_t)48 * CC_FFT * u0 : nullptr, h_dbg ? h_dbg + (size_t)48 * CELL_FE * u0 : nullptr,
                             status ? status + u0 : nullptr, blobs + (size_t)BLOB_BYTES * u0, k, rep, false);
        });
    return cc_single(commitments_out, cells_out, proofs_out, h_dbg, status, blobs, n, cs, device);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_compute_cells_and_kzg_proofs_many(uint8_t *cells_out, uint8_t *proofs_out, int *status, const uint8_t *blobs, size_t n,
                                             const kzg355_settings *s) {
    return cc_impl(nullptr, cells_out, proofs_out, nullptr, status, blobs, n, s);
}

int kzg355_compute_commitments_cells_and_kzg_proofs_many(uint8_t *commitments_out, uint8_t *cells_out, uint8_t *proofs_out, int *status,
                                                         const uint8_t *blobs, size_t n, const kzg355_settings *s) {
    return cc_impl(commitments_out, cells_out, proofs_out, nullptr, status, blobs, n, s);
}

int kzg355_compute_commitments_cells_and_kzg_proofs_many_device(uint8_t *d_commitments_out, uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status,
                                                                const uint8_t *d_blobs, size_t n, const kzg355_settings *s) {
    return cc_impl(d_commitments_out, d_cells_out, d_proofs_out, nullptr, status, d_blobs, n, s, true);
}

int kzg355_compute_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const uint8_t *d_blobs, size_t n,
                                                    const kzg355_settings *s) {
    return cc_impl(nullptr, d_cells_out, d_proofs_out, nullptr, status, d_blobs, n, s, true);
}

int kzg355_compute_cells_and_kzg_proofs(uint8_t *cells_out, uint8_t *proofs_out, const uint8_t *blob, const kzg355_settings *s) {
    return cc_impl(nullptr, cells_out, proofs_out, nullptr, nullptr, blob, 1, s);
}

int kzg355_debug_cell_compute_h(uint8_t *out, int *status, const uint8_t *blobs, size_t n, const kzg355_settings *s) {
    if (!out) return KZG355_BADARGS;
    return cc_impl(nullptr, nullptr, nullptr, out, status, blobs, n, s);
}

int kzg355_debug_cell_setup_monomial_all(uint8_t *out, const kzg355_settings *cs) {
    if (!cs || !out) return KZG355_BADARGS;
    if (is_small(cs)) return KZG355_BADARGS;
    WsGuard g(cs);
    if (!g.w) return KZG355_NO_DEVICE;
    int rc;
    if ((rc = ensure_cc_consts(g.s, g.w)) || (rc = ensure_cc_proof_setup(g.s, g.w))) return rc;
    HIPCHK(hipMemcpy(out, g.s->cc_mono48.p, 48 * (size_t)N_FE, hipMemcpyDeviceToHost));
    return KZG355_OK;
}

#pragma GCC visibility pop
}  // extern "C"
