// cell_proofs_at.hip -- the C entry points of compute_cell_kzg_proofs_at (chosen EIP-7594 cells of blobs and their proofs; include/kzg355.h)
// (host side of libkzg355.so; see engine.h).  compute_cells_and_kzg_proofs pays the whole FK20 chain whatever is wanted of its 128 proofs; here
// every (blob, cell) pair is computed on its own: the field stage of that call (k_cc_field: canonical check, coefficients, cells), the pair's
// quotient in evaluation form (k_cell_quotient.hip), and the fixed-base MSM of the commitment path over it (msm_ops.hip).  One set of launches
// per chunk of whole blobs; the host builds the chunk's pair list, copies blobs in and cells / proofs out and sets the statuses.
#include "engine.h"

namespace kzg355_impl {

// coefficients of the chunk's blobs in w->y -> the proofs of its pairs (engine.h)
int cq_proofs(kzg355_settings *s, Workspace *w, Timed &tm, const CellComputeConsts *cc, const CellChunk &ch, const CqPair *d_pairs, uint8_t *proofs_out,
              bool device) {
    const size_t P = ch.pairs.size();
    hipStream_t st = w->stream;
    tm.begin("cq_quotient");
    launch_cq_quotient(w->y.as<Fr>(), d_pairs, (int)P, w->err.as<int>(), cc, w->scal_a.as<Fr>(), st);
    tm.end();
    int rc;
    if ((rc = msm_to_device(s, w, tm, (int)P, nullptr, w->scal_a.as<Fr>()))) return rc;
    if (!device) HIPCHK(hipMemcpyAsync(w->h_out.p, w->out48.p, 48 * P, hipMemcpyDeviceToHost, st));
    else for (const PlanRun &r : ch.runs)
        HIPCHK(hipMemcpyAsync(proofs_out + 48 * r.slot, w->out48.as<uint8_t>() + 48 * r.pair, 48 * r.len, hipMemcpyDeviceToDevice, st));
    return KZG355_OK;
}

int cq_cells_to_host(Workspace *w, const CellChunk &ch, uint8_t *cells_out) {
    for (const PlanRun &r : ch.runs)
        HIPCHK(hipMemcpyAsync(cells_out + (size_t)CELL_BYTES * r.slot, w->records.as<uint8_t>() + (size_t)CELL_BYTES * r.pair, (size_t)CELL_BYTES * r.len,
                              hipMemcpyDeviceToHost, w->stream));
    return KZG355_OK;
}

int cq_finish(Workspace *w, Timed &tm, const CellChunk &ch, const size_t *counts, uint8_t *host_proofs_out, int *status, int &first) {
    HIPCHK(hipGetLastError());
    int rc;
    if ((rc = launch_set_results(w, ch.m)) || (rc = launch_set_wait(w, tm))) return rc;
    // a refused blob's proofs are not copied into host outputs
    size_t slot = 0;
    rc = launch_set_read(w, ch.m, status, 0, [&](size_t i, int &bst) {
        if (bst == KZG355_OK && host_proofs_out && counts[i])
            memcpy(host_proofs_out + 48 * slot, w->h_out.as<uint8_t>() + 48 * ch.first_pair[i], 48 * counts[i]);
        slot += counts[i];
    });
    if (first == KZG355_OK) first = rc;
    return KZG355_OK;
}

// n > 0 blobs on the device of cs (a replica, for a handle over several devices); the arguments are checked, and the sum of the counts fits.
// Blob i asks for counts[i] cells, the indices idx[off_i ..]; slot off_i + j of cells_out / proofs_out receives cell idx[off_i + j] and its proof.
// device: blobs, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where they are.
// The workspace's buffers by role: blobs = the chunk's blobs (host form), y = coefficients, q = the chunk's 128 cells per blob, z = pair list,
// scal_a = MSM scalars, records = gathered cells (host form); partials, digits, out48 and h_out are the MSM's, as on the commitment path.
static int cq_run(uint8_t *cells_out, uint8_t *proofs_out, int *status, const uint8_t *blobs, size_t n, const size_t *counts, const size_t *idx,
                  const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, n, code); };
    std::unique_ptr<WsGuard> g;
    int rc;
    if ((rc = cell_call_begin(cs, n, g, proofs_out ? wide_table_setup : nullptr))) return refuse(rc);
    kzg355_settings *s = g->s; Workspace *w = g->w;
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    const size_t cell_bytes = (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES;
    CellChunk ch(CC_CHUNK, CQ_CHUNK);
    Timed tm(s, w);
    int first = KZG355_OK;
    size_t off = 0;                                               // the call's slots before the chunk
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    for (size_t c0 = 0; c0 < n; c0 += ch.m, off += ch.slots) {
        plan_compute_chunk(ch, counts + c0, idx ? idx + off : nullptr, n - c0, device);
        const size_t m = ch.m, P = ch.pairs.size();
        uint8_t *cells_at = cells_out ? cells_out + (size_t)CELL_BYTES * off : nullptr, *proofs_at = proofs_out ? proofs_out + 48 * off : nullptr;
        int crc;
        if ((!device && (crc = w->blobs.ensure((size_t)BLOB_BYTES * m))) || (crc = w->z.ensure(sizeof(CqPair) * P)) ||
            (proofs_out && ((crc = w->y.ensure(sizeof(Fr) * N_FE * m)) || (crc = w->scal_a.ensure(sizeof(Fr) * N_FE * P)) ||
                            (!device && (crc = w->h_out.ensure(48 * P))))) ||
            (cells_out && ((crc = w->q.ensure(cell_bytes * m)) || (!device && (crc = w->records.ensure((size_t)CELL_BYTES * P))))))
            return crc;
        if ((crc = launch_set_begin(w, m))) return crc;
        hipStream_t st = w->stream;
        const uint8_t *d_blobs = device ? blobs + (size_t)BLOB_BYTES * c0 : w->blobs.as<uint8_t>();
        if (!device) HIPCHK(hipMemcpyAsync(w->blobs.p, blobs + (size_t)BLOB_BYTES * c0, (size_t)BLOB_BYTES * m, hipMemcpyHostToDevice, st));
        if (ch.any_refused) HIPCHK(hipMemcpyAsync(w->err.p, ch.refused.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
        if (P) HIPCHK(hipMemcpyAsync(w->z.p, ch.pairs.data(), sizeof(CqPair) * P, hipMemcpyHostToDevice, st));
        tm.begin("cc_field");
        launch_cc_field(d_blobs, (int)m, cc, proofs_out ? w->y.as<Fr>() : nullptr, cells_out ? w->q.as<uint8_t>() : nullptr, w->err.as<int>(), st);
        tm.end();
        if (proofs_out && P && (crc = cq_proofs(s, w, tm, cc, ch, w->z.as<CqPair>(), proofs_at, device))) return crc;
        if (cells_out && P) {
            tm.begin("cq_gather");
            launch_cq_gather(w->q.as<uint8_t>(), w->z.as<CqPair>(), (int)P, device ? cells_at : w->records.as<uint8_t>(), st);
            tm.end();
            if (!device && (crc = cq_cells_to_host(w, ch, cells_at))) return crc;
        }
        if ((crc = cq_finish(w, tm, ch, counts + c0, device ? nullptr : proofs_at, status ? status + c0 : nullptr, first))) return crc;
    }
    return KZG355_OK;
    };
    if ((rc = run())) return refuse(rc);
    return first;
}

static int cq_impl(uint8_t *cells_out, uint8_t *proofs_out, int *status, const uint8_t *blobs, size_t n, const size_t *counts, const size_t *idx,
                   const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, n, code); };
    if (!cs || (!cells_out && !proofs_out)) return refuse(KZG355_BADARGS);
    if (n == 0) return KZG355_OK;
    if (!blobs || !counts || n > ((size_t)1 << 32)) return refuse(KZG355_BADARGS);
    if (device && misaligned(cells_out, proofs_out, blobs)) return refuse(KZG355_BADARGS);
    size_t total;
    if (!sum_counts(total, counts, n) || (total && !idx)) return refuse(KZG355_BADARGS);
    if (cs->multi && !device) {                                   // ranges of blobs over the replicas: a range's indices and slots start at the sum before it
        const std::vector<size_t> first = prefix_sums(counts, n);
        return cc_fan_out(cs, n, status, [&](const kzg355_settings *rep, size_t u0, size_t k) {
            return cq_run(cells_out ? cells_out + (size_t)CELL_BYTES * first[u0] : nullptr, proofs_out ? proofs_out + 48 * first[u0] : nullptr,
                          status ? status + u0 : nullptr, blobs + (size_t)BLOB_BYTES * u0, k, counts + u0, idx ? idx + first[u0] : nullptr, rep, false);
        });
    }
    return cq_run(cells_out, proofs_out, status, blobs, n, counts, idx, cs, device);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_compute_cell_kzg_proofs_at_many(uint8_t *cells_out, uint8_t *proofs_out, int *status, const uint8_t *blobs, size_t n,
                                           const size_t *cell_counts, const size_t *cell_indices, const kzg355_settings *s) {
    return cq_impl(cells_out, proofs_out, status, blobs, n, cell_counts, cell_indices, s, false);
}

int kzg355_compute_cell_kzg_proofs_at_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, int *status, const uint8_t *d_blobs, size_t n,
                                                  const size_t *cell_counts, const size_t *cell_indices, const kzg355_settings *s) {
    return cq_impl(d_cells_out, d_proofs_out, status, d_blobs, n, cell_counts, cell_indices, s, true);
}

int kzg355_compute_cell_kzg_proofs_at(uint8_t *cells_out, uint8_t *proofs_out, const uint8_t *blob, const size_t *cell_indices, size_t k,
                                      const kzg355_settings *s) {
    return cq_impl(cells_out, proofs_out, nullptr, blob, 1, &k, cell_indices, s, false);
}

#pragma GCC visibility pop
}  // extern "C"
