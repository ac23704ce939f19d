// cell_proofs_at.hip -- the C entry points of compute_cell_kzg_proofs_at (chosen EIP-7594 cells of blobs and their proofs; include/kzg355.h)
// (host side of libkzg355.so; see engine.h).  compute_cells_and_kzg_proofs pays the whole FK20 chain whatever is wanted of its 128 proofs; here
// every (blob, cell) pair is computed on its own: the field stage of that call (k_cc_field: canonical check, coefficients, cells), the pair's
// quotient in evaluation form (k_cell_quotient.hip), and the fixed-base MSM of the commitment path over it (msm_ops.hip).  One set of launches
// per chunk of whole blobs; the host builds the chunk's pair list, copies blobs in and cells / proofs out and sets the statuses.
#include "engine.h"

namespace kzg355_impl {

// a chunk's output runs: `len` pairs from the chunk's pair `pair` on land in the call's slots `slot` onwards (a blob the host refused fills no
// pair and may still take slots, so that the pairs of a chunk are not always one run)
struct CqRun { size_t pair, slot, len; };

// n > 0 blobs on the device of cs (a replica, for a handle over several devices); the arguments are checked, and the sum of the counts fits.
// Blob i asks for counts[i] cells, the indices idx[off_i ..]; slot off_i + j of cells_out / proofs_out receives cell idx[off_i + j] and its proof.
// device: blobs, cells_out and proofs_out are device memory on the handle's device (16-byte aligned), read and written where they are.
// The workspace's buffers by role: blobs = the chunk's blobs (host form), y = coefficients, q = the chunk's 128 cells per blob, z = pair list,
// scal_a = MSM scalars, records = gathered cells (host form); partials, digits, out48 and h_out are the MSM's, as on the commitment path.
static int cq_run(uint8_t *cells_out, uint8_t *proofs_out, int *status, const uint8_t *blobs, size_t n, const size_t *counts, const size_t *idx,
                  const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, n, code); };
    if (n > ((size_t)1 << 32) || is_small(cs)) return refuse(KZG355_BADARGS);    // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    if ((rc = ensure_cc_consts(s, w))) return refuse(rc);
    if (proofs_out && (rc = ensure_wide_table(s))) return refuse(rc);             // the first call that wants proofs builds the table, as a commitment does
    s->n_cell_sets.fetch_add(1);
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    const size_t cell_bytes = (size_t)CELLS_PER_EXT_BLOB * CELL_BYTES;
    std::vector<CqPair> pairs;
    std::vector<CqRun> runs;
    std::vector<int> refused;                                     // the chunk's err words, when the host refuses one of its blobs
    std::vector<size_t> first_pair;                               // of each blob of the chunk (refused: none)
    Timed tm(s, w);
    int first = KZG355_OK;
    size_t off = 0;                                               // the call's slots before the chunk
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    for (size_t c0 = 0; c0 < n;) {
        // the chunk: whole blobs while their pairs fit CQ_CHUNK (a blob has at most 128) and there are at most CC_CHUNK of them
        pairs.clear(); runs.clear(); refused.clear(); first_pair.clear();
        bool any_refused = false;
        size_t m = 0, slots = 0;
        for (; c0 + m < n && m < CC_CHUNK; m++) {
            const size_t cnt = counts[c0 + m], *ix = cnt ? idx + off + slots : nullptr;
            bool good = cnt <= (size_t)CELLS_PER_EXT_BLOB;
            for (size_t j = 0; good && j < cnt; j++) good = ix[j] < (size_t)CELLS_PER_EXT_BLOB;
            if (good && pairs.size() + cnt > CQ_CHUNK) break;
            first_pair.push_back(pairs.size());
            refused.push_back(good ? 0 : ERR_NONCANONICAL_FR);   // any err word is this blob's KZG355_BADARGS (status_from_err)
            any_refused |= !good;
            if (good && cnt) {
                if (runs.empty() || runs.back().slot + runs.back().len != slots) runs.push_back(CqRun{pairs.size(), slots, 0});
                runs.back().len += cnt;
                // (the host form gathers pair after pair and copies run by run; the device form gathers into the caller's slots)
                for (size_t j = 0; j < cnt; j++) pairs.push_back(CqPair{(uint32_t)m, (uint32_t)ix[j], device ? slots + j : (uint64_t)pairs.size()});
            }
            slots += cnt;
        }
        const size_t P = pairs.size();
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
        if (any_refused) HIPCHK(hipMemcpyAsync(w->err.p, refused.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
        if (P) HIPCHK(hipMemcpyAsync(w->z.p, pairs.data(), sizeof(CqPair) * P, hipMemcpyHostToDevice, st));
        tm.begin("cc_field");
        launch_cc_field(d_blobs, (int)m, cc, proofs_out ? w->y.as<Fr>() : nullptr, cells_out ? w->q.as<uint8_t>() : nullptr, w->err.as<int>(), st);
        tm.end();
        if (proofs_out && P) {
            tm.begin("cq_quotient");
            launch_cq_quotient(w->y.as<Fr>(), w->z.as<CqPair>(), (int)P, w->err.as<int>(), cc, w->scal_a.as<Fr>(), st);
            tm.end();
            if ((crc = msm_to_device(s, w, tm, (int)P, nullptr, w->scal_a.as<Fr>()))) return crc;
            if (!device) HIPCHK(hipMemcpyAsync(w->h_out.p, w->out48.p, 48 * P, hipMemcpyDeviceToHost, st));
            else for (const CqRun &r : runs)
                HIPCHK(hipMemcpyAsync(proofs_out + 48 * (off + r.slot), w->out48.as<uint8_t>() + 48 * r.pair, 48 * r.len, hipMemcpyDeviceToDevice, st));
        }
        if (cells_out && P) {
            tm.begin("cq_gather");
            launch_cq_gather(w->q.as<uint8_t>(), w->z.as<CqPair>(), (int)P, device ? cells_out + (size_t)CELL_BYTES * off : w->records.as<uint8_t>(), st);
            tm.end();
            if (!device) for (const CqRun &r : runs)
                HIPCHK(hipMemcpyAsync(cells_out + (size_t)CELL_BYTES * (off + r.slot), w->records.as<uint8_t>() + (size_t)CELL_BYTES * r.pair,
                                      (size_t)CELL_BYTES * r.len, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipGetLastError());
        if ((crc = launch_set_results(w, m)) || (crc = launch_set_wait(w, tm))) return crc;
        // a refused blob's proofs are not copied into host outputs
        size_t slot = off;
        crc = launch_set_read(w, m, status ? status + c0 : nullptr, 0, [&](size_t i, int &bst) {
            const size_t cnt = counts[c0 + i];
            if (bst == KZG355_OK && proofs_out && !device && cnt) memcpy(proofs_out + 48 * slot, w->h_out.as<uint8_t>() + 48 * first_pair[i], 48 * cnt);
            slot += cnt;
        });
        if (first == KZG355_OK) first = crc;
        off += slots;
        c0 += m;
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
    if (device && (((uintptr_t)cells_out & 15) || ((uintptr_t)proofs_out & 15) || ((uintptr_t)blobs & 15))) return refuse(KZG355_BADARGS);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (counts[i] > SIZE_MAX / CELL_BYTES - total) return refuse(KZG355_BADARGS);    // the sum, in bytes of cells, stays a size_t
        total += counts[i];
    }
    if (total && !idx) return refuse(KZG355_BADARGS);
    if (cs->multi && !device) {                                   // ranges of blobs over the replicas: a range's indices and slots start at the sum before it
        std::vector<size_t> first(n + 1, 0);
        for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + counts[i];
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
