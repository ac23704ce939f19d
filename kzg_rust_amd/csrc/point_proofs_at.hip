// point_proofs_at.hip -- the C entry points of compute_kzg_proofs_at (openings of blobs at chosen points: proofs and y = p(z); include/kzg355.h)
// (host side of libkzg355.so; see engine.h).  compute_kzg_proof_many takes one blob per opening; here a blob is read once per chunk and every
// (blob, point) pair is computed on its own: the field stage of the cell calls (k_cc_field: canonical check, coefficients), the pair's y and
// quotient in evaluation form (k_point_quotient.hip), and the fixed-base MSM of the commitment path over it (msm_ops.hip).  One set of launches
// per chunk (point_plan.h: pieces of blobs, a blob may be cut at the border); the host checks the points while it plans, copies blobs and
// points in and proofs / ys out and sets the statuses.
#include "engine.h"

namespace kzg355_impl {

// n > 0 blobs on the device of cs (a replica, for a handle over several devices); the arguments are checked, and the sum of the counts fits.
// Blob i is opened at counts[i] points, zs[32 off_i ..]; slot off_i + j of proofs_out / ys_out receives the proof and y of the j-th of them.
// device: blobs, proofs_out and ys_out are device memory on the handle's device (16-byte aligned), read and written where they are.
// The workspace's buffers by role: blobs = the chunk's blobs (host form), y = coefficients, z = pair list, proofs = the pairs' points as bytes,
// zpow = the same in Montgomery form (ok: the conversion's error words, never set -- the plan took canonical points only), scal_a = MSM scalars,
// records / h_records = the pairs' ys (host form); partials, digits, out48 and h_out are the MSM's, as on the commitment path.
static int pq_run(uint8_t *proofs_out, uint8_t *ys_out, int *status, const uint8_t *blobs, size_t n, const size_t *counts, const uint8_t *zs,
                  const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, n, code); };
    std::unique_ptr<WsGuard> g;
    int rc;
    if ((rc = cell_call_begin(cs, n, g, proofs_out ? wide_table_setup : nullptr))) return refuse(rc);
    kzg355_settings *s = g->s; Workspace *w = g->w;
    const CellComputeConsts *cc = s->cc_consts.as<CellComputeConsts>();
    PointPlan plan(CC_CHUNK, CQ_CHUNK, counts, zs, n);
    PointChunk ch;
    Timed tm(s, w);
    int first = KZG355_OK, cut = KZG355_OK;                         // cut: the status so far of the blob the last chunk ended inside
    auto run = [&]() -> int {                                     // (HIPCHK returns from here: a failed chunk refuses the whole call)
    while (plan.next(ch, device)) {
        const size_t m = ch.m(), P = ch.pairs.size(), c0 = ch.pieces[0].blob;
        int crc;
        if ((!device && (crc = w->blobs.ensure((size_t)BLOB_BYTES * m))) || (crc = w->y.ensure(sizeof(Fr) * N_FE * m)) ||
            (crc = w->z.ensure(sizeof(PqPair) * P)) || (crc = w->proofs.ensure(32 * P)) || (crc = w->zpow.ensure(sizeof(Fr) * P)) ||
            (crc = w->ok.ensure(sizeof(int) * P)) ||
            (proofs_out && ((crc = w->scal_a.ensure(sizeof(Fr) * N_FE * P)) || (!device && (crc = w->h_out.ensure(48 * P))))) ||
            (ys_out && !device && ((crc = w->records.ensure(32 * P)) || (crc = w->h_records.ensure(32 * P)))))
            return crc;
        if ((crc = launch_set_begin(w, m))) return crc;
        hipStream_t st = w->stream;
        const uint8_t *d_blobs = device ? blobs + (size_t)BLOB_BYTES * c0 : w->blobs.as<uint8_t>();
        if (!device) HIPCHK(hipMemcpyAsync(w->blobs.p, blobs + (size_t)BLOB_BYTES * c0, (size_t)BLOB_BYTES * m, hipMemcpyHostToDevice, st));
        if (ch.any_refused) HIPCHK(hipMemcpyAsync(w->err.p, ch.refused.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
        if (P) {
            HIPCHK(hipMemcpyAsync(w->z.p, ch.pairs.data(), sizeof(PqPair) * P, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(w->proofs.p, ch.zs.data(), 32 * P, hipMemcpyHostToDevice, st));
            launch_fr_from_bytes(w->proofs.as<uint8_t>(), (int)P, w->zpow.as<Fr>(), w->ok.as<int>(), st);
        }
        tm.begin("cc_field");
        launch_cc_field(d_blobs, (int)m, cc, w->y.as<Fr>(), nullptr, w->err.as<int>(), st);
        tm.end();
        if (P) {
            uint8_t *d_ys = !ys_out ? nullptr : device ? ys_out : w->records.as<uint8_t>();
            Fr *d_scal = proofs_out ? w->scal_a.as<Fr>() : nullptr;
            tm.begin("pq_quotient");
            launch_pq_quotient(w->y.as<Fr>(), w->z.as<PqPair>(), w->zpow.as<Fr>(), (int)P, w->err.as<int>(), cc, d_scal, d_ys, st);
            tm.end();
            if (ys_out && !device) HIPCHK(hipMemcpyAsync(w->h_records.p, w->records.p, 32 * P, hipMemcpyDeviceToHost, st));
            if (proofs_out) {
                if ((crc = msm_to_device(s, w, tm, (int)P, nullptr, d_scal))) return crc;
                if (!device) HIPCHK(hipMemcpyAsync(w->h_out.p, w->out48.p, 48 * P, hipMemcpyDeviceToHost, st));
                else for (const PointRun &r : ch.runs)
                    HIPCHK(hipMemcpyAsync(proofs_out + 48 * r.slot, w->out48.as<uint8_t>() + 48 * r.pair, 48 * r.len, hipMemcpyDeviceToDevice, st));
            }
        }
        HIPCHK(hipGetLastError());
        if ((crc = launch_set_results(w, m)) || (crc = launch_set_wait(w, tm))) return crc;
        // a cut blob's status is the first non-OK of its pieces; a refused blob's results are not copied into host outputs
        crc = launch_set_read(w, m, status ? status + c0 : nullptr, 0, [&](size_t i, int &bst) {
            const PointPiece &pc = ch.pieces[i];
            if (pc.skip && cut != KZG355_OK) bst = cut;
            if (i + 1 == m) cut = bst;
            if (bst != KZG355_OK || device || !pc.len) return;
            if (proofs_out) memcpy(proofs_out + 48 * pc.slot, w->h_out.as<uint8_t>() + 48 * pc.first_pair, 48 * pc.len);
            if (ys_out) memcpy(ys_out + 32 * pc.slot, w->h_records.as<uint8_t>() + 32 * pc.first_pair, 32 * pc.len);
        });
        if (first == KZG355_OK) first = crc;
    }
    return KZG355_OK;
    };
    if ((rc = run())) return refuse(rc);
    return first;
}

static int pq_impl(uint8_t *proofs_out, uint8_t *ys_out, int *status, const uint8_t *blobs, size_t n, const size_t *counts, const uint8_t *zs,
                   const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, n, code); };
    if (!cs || (!proofs_out && !ys_out)) return refuse(KZG355_BADARGS);
    if (n == 0) return KZG355_OK;
    if (!blobs || !counts || n > ((size_t)1 << 32)) return refuse(KZG355_BADARGS);
    if (device && misaligned(proofs_out, ys_out, blobs)) return refuse(KZG355_BADARGS);
    size_t total;
    if (!sum_point_counts(total, counts, n) || (total && !zs)) return refuse(KZG355_BADARGS);
    if (cs->multi && !device) {                                   // ranges of blobs over the replicas: a range's points and slots start at the sum before it
        const std::vector<size_t> first = prefix_sums(counts, n);
        return cc_fan_out(cs, n, status, [&](const kzg355_settings *rep, size_t u0, size_t k) {
            return pq_run(proofs_out ? proofs_out + 48 * first[u0] : nullptr, ys_out ? ys_out + 32 * first[u0] : nullptr, status ? status + u0 : nullptr,
                          blobs + (size_t)BLOB_BYTES * u0, k, counts + u0, zs ? zs + 32 * first[u0] : nullptr, rep, false);
        });
    }
    return pq_run(proofs_out, ys_out, status, blobs, n, counts, zs, cs, device);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_compute_kzg_proofs_at_many(uint8_t *proofs_out, uint8_t *ys_out, int *status, const uint8_t *blobs, size_t n, const size_t *point_counts,
                                      const uint8_t *zs, const kzg355_settings *s) {
    return pq_impl(proofs_out, ys_out, status, blobs, n, point_counts, zs, s, false);
}

int kzg355_compute_kzg_proofs_at_many_device(uint8_t *d_proofs_out, uint8_t *d_ys_out, int *status, const uint8_t *d_blobs, size_t n,
                                             const size_t *point_counts, const uint8_t *zs, const kzg355_settings *s) {
    return pq_impl(d_proofs_out, d_ys_out, status, d_blobs, n, point_counts, zs, s, true);
}

int kzg355_compute_kzg_proofs_at(uint8_t *proofs_out, uint8_t *ys_out, const uint8_t *blob, const uint8_t *zs, size_t k, const kzg355_settings *s) {
    return pq_impl(proofs_out, ys_out, nullptr, blob, 1, &k, zs, s, false);
}

#pragma GCC visibility pop
}  // extern "C"
