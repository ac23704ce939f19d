// blob_cells.hip -- the C entry points of verify_blob_cell_proofs_batch (include/kzg355.h): blobs against their EIP-7594 cell proofs, the Fulu
// counterpart of verify_blob_kzg_proof_batch (host side of libkzg355.so; see engine.h).  The answer is, by definition, that of
// verify_cell_kzg_proof_batch on all 128 cells of every blob of a group, the cells computed from the blobs; here the blobs go to the device once,
// k_cc_field (k_cell_compute.hip) leaves their coefficients and their cells there, and the chain of cells.hip checks them where they are, its
// interpolation taken from the coefficients (k_blob_cells.hip).  The host deduplicates the n commitments of a group and, for calls of few groups,
// hashes the transcripts (the extension halves of the cells come back for that) while the point kernels run.
// The `_sets` entry points take groups of different blob counts: the same launch set on the ragged entries of the kernels (blob_set with boff).
#include "engine.h"

namespace kzg355_impl {

static const size_t BLOB_CELLS_MAX_BLOBS = CELL_MAX_CELLS / CELLS_PER_EXT_BLOB;      // blobs per group, and per launch set
static const size_t HALF_BYTES = (size_t)BLOB_BYTES;                                 // cells 0..63 of a blob, and cells 64..127

// the transcript digest of one group of n blobs: u unique commitments uc, blob b carrying commitment pos[b], its cells 0..63 at lo(b) and
// 64..127 at hi(b) (HALF_BYTES each), its 128 proofs following those of blob b - 1
template <class Lo, class Hi>
static void blob_transcript(const kzg355_settings *s, const uint8_t *uc, int u, const int *pos, size_t n, Lo lo, Hi hi, const uint8_t *proofs, uint8_t *dig) {
    const size_t npg = (size_t)CELLS_PER_EXT_BLOB * n, len = 16 + 32 + 48 * (size_t)u + npg * (16 + CELL_BYTES + 48);
    std::vector<uint8_t> msg(len);
    uint8_t *p = msg.data();
    memcpy(p, CELL_DOMAIN, 16); p += 16;
    put_u64be(p, N_FE); put_u64be(p + 8, CELL_FE); put_u64be(p + 16, (uint64_t)u); put_u64be(p + 24, npg); p += 32;
    memcpy(p, uc, 48 * (size_t)u); p += 48 * (size_t)u;
    for (size_t b = 0; b < n; b++) {
        const uint8_t *half[2] = {lo(b), hi(b)};
        for (size_t k = 0; k < (size_t)CELLS_PER_EXT_BLOB; k++) {
            put_u64be(p, (uint64_t)pos[b]); put_u64be(p + 8, k); p += 16;
            memcpy(p, half[k / CELL_FE] + (size_t)CELL_BYTES * (k % CELL_FE), CELL_BYTES); p += CELL_BYTES;
            memcpy(p, proofs + 48 * (CELLS_PER_EXT_BLOB * b + k), 48); p += 48;
        }
    }
    kzg_host::sha256(dig, msg.data(), len, s->sha_impl);
}

// One launch set: `groups` whole groups of n blobs (128 n groups <= CELL_MAX_CELLS cells) on the workspace's device.  boff (groups + 1 entries,
// strictly increasing; n is then unused): the groups have their own blob counts, group g being blobs [boff[g], boff[g + 1]) of the three arrays,
// and the `_sets` entries of the kernels run on the offsets 128 boff[g] (cell_chain, sets_N).  device: the three arrays are device memory
// there.  form: 1 the interpolation from the coefficients, 2 k_cell_columns over the computed cells.  The workspace's buffers by role, beyond
// those of cell_reserve (blobs = the computed cells): qprep = the blobs, zpow = their coefficients, shifts = W, small = the unique commitments
// as deduplicated, scal_c = commitment positions | unique counts | per-blob error words, scal_b = the index array of the device hash.
static int blob_set(kzg355_settings *s, Workspace *w, bool *ok, int *status, uint8_t *dbg, const uint8_t *blobs, const uint8_t *commitments,
                    const uint8_t *proofs, size_t n, size_t groups, bool device, int form, int prep_form, const size_t *boff = nullptr) {
    s->n_cell_sets.fetch_add(1);
    auto blob0 = [&](size_t g) { return boff ? boff[g] : n * g; };                 // the blobs before group g, and its own
    auto blobs_of = [&](size_t g) { return boff ? boff[g + 1] - boff[g] : n; };
    size_t n_max = boff ? 0 : n;                                                   // the largest group
    if (boff) for (size_t g = 0; g < groups; g++) n_max = std::max(n_max, blobs_of(g));
    const size_t npg = (size_t)CELLS_PER_EXT_BLOB * n, nb = blob0(groups), N = (size_t)CELLS_PER_EXT_BLOB * nb;
    const int G = (int)groups, S = G * (form == 1 ? CELL_FE : CELLS_PER_EXT_BLOB);
    const size_t meta_ints = (size_t)4 * S + (G + 1) + 3 * N + (boff ? (G + 1) + N : 0);
    // Groups of different sizes: the rule sees the launch set's LARGEST group and its number of groups.  It was measured on uniform shapes
    // only (cells.hip); where it puts the crossover of a ragged launch set has NOT been measured.
    const bool host_hash = cell_device_call_prepares_on_host(s, (size_t)CELLS_PER_EXT_BLOB * n_max, groups, prep_form);
    hipStream_t st = w->stream;
    int rc;
    if ((rc = boff ? cell_reserve_sized(w, true, N, (size_t)cell_terms_sets((int)N, G), groups, S, meta_ints)
                   : cell_reserve(w, true, (int)npg, groups, S, meta_ints)) ||
        (!device && (rc = w->qprep.ensure(HALF_BYTES * nb))) ||
        (form == 1 && ((rc = w->zpow.ensure(sizeof(Fr) * N_FE * nb)) || (rc = w->shifts.ensure(sizeof(Fr) * CELL_FE * groups)))) ||
        (rc = w->small.ensure(48 * nb)) || (rc = w->scal_c.ensure(sizeof(int) * (2 * nb + groups))) ||
        (!host_hash && (rc = w->scal_b.ensure(sizeof(size_t) * N))))
        return rc;
    // pinned staging: the commitments of a device call, then what the host hashes -- of a host call the extension halves of the cells, of a
    // device call its proofs and all the cells
    const size_t stage_c = device ? (48 * nb + 15) & ~(size_t)15 : 0, stage_p = device && host_hash ? 48 * N : 0;
    const size_t stage_cells = !host_hash ? 0 : device ? 2 * HALF_BYTES * nb : HALF_BYTES * nb;
    if (stage_c + stage_p + stage_cells && (rc = w->h_stage.ensure(stage_c + stage_p + stage_cells))) return rc;
    uint8_t *h_c = w->h_stage.as<uint8_t>(), *h_p = h_c + stage_c, *h_cells = h_p + stage_p;
    Fp *f12 = nullptr;
    if (w->pair_f.ensure(pairing_f12_bytes(G)) == KZG355_OK) f12 = w->pair_f.as<Fp>();
    if ((rc = launch_set_begin(w, groups, true))) return rc;       // (cell_reserve has sized the words)
    Timed tm(s, w);

    // ---- the commitments: deduplicated per group, always here (48 bytes per blob)
    if (device) {
        HIPCHK(hipMemcpyAsync(h_c, commitments, 48 * nb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    const uint8_t *hc = device ? h_c : commitments;
    std::vector<uint8_t> h_uc(48 * nb);
    std::vector<int> h_meta(2 * nb + groups, 0);                  // positions | unique counts | error words (zero)
    std::vector<uint8_t> h_dig(host_hash ? 32 * groups : 0);
    for (size_t g = 0; g < groups; g++)
        h_meta[nb + g] = cell_dedup(hc + 48 * blob0(g), blobs_of(g), h_uc.data() + 48 * blob0(g), h_meta.data() + blob0(g));
    int *d_pos = w->scal_c.as<int>(), *d_ucount = d_pos + nb, *d_blob_err = d_ucount + groups;
    HIPCHK(hipMemcpyAsync(w->small.p, h_uc.data(), 48 * nb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_pos, h_meta.data(), sizeof(int) * h_meta.size(), hipMemcpyHostToDevice, st));

    // ---- the blobs: 128 KiB each up, coefficients and cells by k_cc_field
    const uint8_t *d_blobs = device ? blobs : w->qprep.as<uint8_t>(), *d_proofs = device ? proofs : w->proofs.as<uint8_t>();
    uint8_t *d_cells = w->blobs.as<uint8_t>();
    if (!device) {
        HIPCHK(hipMemcpyAsync(w->qprep.p, blobs, HALF_BYTES * nb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(w->proofs.p, proofs, 48 * N, hipMemcpyHostToDevice, st));
    }
    tm.begin("cc_field");
    launch_cc_field(d_blobs, (int)nb, s->cc_consts.as<CellComputeConsts>(), form == 1 ? w->zpow.as<Fr>() : nullptr, d_cells, d_blob_err, st);
    tm.end();
    int *m = w->q.as<int>() + 4 * (size_t)S;                      // gseg | cell index | commitment position | perm
    int *d_goff = m + (G + 1) + 3 * N, *d_cgrp = d_goff + (G + 1);   // (boff only) the cells before each group, the group of every cell
    if (boff) {
        std::vector<int> h_geo((G + 1) + N);
        for (size_t g = 0; g <= groups; g++) h_geo[g] = (int)((size_t)CELLS_PER_EXT_BLOB * boff[g]);
        for (size_t g = 0; g < groups; g++) std::fill(h_geo.begin() + (G + 1) + h_geo[g], h_geo.begin() + (G + 1) + h_geo[g + 1], (int)g);
        HIPCHK(hipMemcpyAsync(d_goff, h_geo.data(), sizeof(int) * h_geo.size(), hipMemcpyHostToDevice, st));     // (pageable: staged before it returns)
    }
    tm.begin("cell_prep");
    if (boff)
        launch_blob_cell_meta_sets(d_pos, d_ucount, w->small.as<uint8_t>(), d_blob_err, d_goff, d_cgrp, (int)N, G, form == 2, w->q.as<int4>(), m, m + (G + 1),
                                   m + (G + 1) + N, m + (G + 1) + 2 * N, host_hash ? nullptr : w->scal_b.as<size_t>(), w->commitments.as<uint8_t>(),
                                   w->err.as<int>(), st);
    else
        launch_blob_cell_meta(d_pos, d_ucount, w->small.as<uint8_t>(), d_blob_err, (int)n, G, form == 2, w->q.as<int4>(), m, m + (G + 1), m + (G + 1) + N,
                              m + (G + 1) + 2 * N, host_hash ? nullptr : w->scal_b.as<size_t>(), w->commitments.as<uint8_t>(), w->err.as<int>(), st);
    tm.end();

    // ---- the transcript digests: on the host beside the point kernels, or on the device
    if (host_hash) {
        if (device) {
            HIPCHK(hipMemcpyAsync(h_p, proofs, 48 * N, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_cells, d_cells, 2 * HALF_BYTES * nb, hipMemcpyDeviceToHost, st));
        } else {
            HIPCHK(hipMemcpy2DAsync(h_cells, HALF_BYTES, d_cells + HALF_BYTES, 2 * HALF_BYTES, HALF_BYTES, nb, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipEventRecord(w->ev_stage, st));
    }
    if (boff) cell_chain_points_sets(w, tm, d_proofs, S, N, G);
    else cell_chain_points(w, tm, d_proofs, (int)npg, G);
    if (host_hash) {
        HIPCHK(hipEventSynchronize(w->ev_stage));
        const uint8_t *hp = device ? h_p : proofs;
        const auto t0 = std::chrono::steady_clock::now();
        auto one = [&](size_t g) {
            const size_t b0 = blob0(g);
            auto lo = [&](size_t b) { return device ? h_cells + 2 * HALF_BYTES * (b0 + b) : blobs + HALF_BYTES * (b0 + b); };
            auto hi = [&](size_t b) { return device ? h_cells + 2 * HALF_BYTES * (b0 + b) + HALF_BYTES : h_cells + HALF_BYTES * (b0 + b); };
            blob_transcript(s, h_uc.data() + 48 * b0, h_meta[nb + g], h_meta.data() + b0, blobs_of(g), lo, hi, hp + 48 * CELLS_PER_EXT_BLOB * b0,
                            h_dig.data() + 32 * g);
        };
        if (s->host_pool && groups > 1) s->host_pool->parallel_for(groups, one);
        else for (size_t g = 0; g < groups; g++) one(g);
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (s->timing) { std::lock_guard<std::mutex> lk(s->mu); auto &k = s->last_ms["cell_host"]; k.last = host_ms; k.total += host_ms; k.count++; }
        HIPCHK(hipMemcpyAsync(w->digests.p, h_dig.data(), 32 * groups, hipMemcpyHostToDevice, st));
    } else {
        tm.begin("cell_rhash");
        if (boff)
            launch_cell_rhash_sets(w->commitments.as<uint8_t>(), w->scal_b.as<size_t>(), d_cells, d_proofs, m + (G + 1) + N, d_ucount, d_goff, G,
                                   G >= s->rhash_lanes_from, w->digests.as<uint8_t>(), st);
        else
            launch_cell_rhash(w->commitments.as<uint8_t>(), w->scal_b.as<size_t>(), d_cells, d_proofs, m + (G + 1) + N, d_ucount, (int)npg, G,
                              G >= s->rhash_lanes_from, w->digests.as<uint8_t>(), st);
        tm.end();
    }

    // ---- the chain of verify_cell_kzg_proof_batch from the scalars on
    uint8_t *d_dbg = dbg ? w->out48.as<uint8_t>() + 32 * groups : nullptr;
    const BlobInterp bi{w->zpow.as<Fr>(), (int)n, w->shifts.as<Fr>()};
    cell_chain(s, w, tm, d_cells, d_proofs, S, (int)npg, G, 0, true, d_dbg, true, form == 1 ? &bi : nullptr, boff ? N : 0);
    tm.begin("cell_pairing");
    launch_pairing(w->pair_pts.as<PairPt>(), s->cell_t, G, w->ok.as<int>(), st, s->pairing_two_wave_upto, f12, s->pairing_hard12_from, s->miller_segments);
    tm.end();
    HIPCHK(hipGetLastError());
    if ((rc = launch_set_results(w, groups, true))) return rc;
    if (dbg) HIPCHK(hipMemcpyAsync(w->h_out.p, d_dbg, (size_t)CELL_DEBUG_BYTES * groups, hipMemcpyDeviceToHost, st));
    if ((rc = launch_set_wait(w, tm))) return rc;
    if (dbg) memcpy(dbg, w->h_out.p, (size_t)CELL_DEBUG_BYTES * groups);
    return launch_set_read(w, groups, status, 0, [&](size_t i, int &stt) { ok[i] = stt == KZG355_OK && w->h_ok.as<int>()[i] != 0; });
}

// Which interpolation interp_form 0 takes.  The coefficient route reads every blob coefficient once and needs no inverse DFT; the column route
// runs 128 DFTs of size 64 per group over the cell bytes.  MEASURED ("verify blobs against cell proofs", the cell_interp family, ms,
// coefficients / columns): 64 x 1 blobs 0.13 / 0.41, 64 x 6: 0.15 / 0.46, 1 x 128: 0.24 / 0.34 -- but 1 x 1: 0.12 / 0.10 and 1 x 6: 0.13 / 0.11,
// where either route is a few waves and the coefficient route's third dependent launch is what shows.  So a launch set of at most
// BLOB_COLUMNS_UPTO_BLOBS blobs takes the columns; the crossover lies between 6 and 64 blobs and has not been located more closely.
static const size_t BLOB_COLUMNS_UPTO_BLOBS = 6;
static int blob_interp_form(int interp_form, size_t blobs) { return interp_form ? interp_form : blobs <= BLOB_COLUMNS_UPTO_BLOBS ? 2 : 1; }

// `groups` whole groups on the device of cs (a replica, for a handle over several devices), in launch sets of whole groups; the arguments are checked
static int blob_single(bool *ok, int *status, uint8_t *dbg, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs, size_t n, size_t groups,
                       const kzg355_settings *cs, bool device, int interp_form, int prep_form) {
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    // the constants of the extension and the setup of the check: neither is the proof setup of compute_cells_and_kzg_proofs
    if ((rc = ensure_cc_consts(s, w)) || (rc = ensure_cell_setup(s, w))) return refuse(rc);
    const size_t per = BLOB_CELLS_MAX_BLOBS / n, npg = (size_t)CELLS_PER_EXT_BLOB * n;
    int first = KZG355_OK;
    for (size_t g0 = 0; g0 < groups; g0 += per) {
        const size_t cnt = groups - g0 < per ? groups - g0 : per, b0 = g0 * n;
        rc = blob_set(s, w, ok + g0, status ? status + g0 : nullptr, dbg ? dbg + (size_t)CELL_DEBUG_BYTES * g0 : nullptr, blobs + HALF_BYTES * b0,
                      commitments + 48 * b0, proofs + 48 * npg * g0, n, cnt, device, blob_interp_form(interp_form, n * cnt), prep_form);
        if (call_failed(rc)) return refuse(rc);
        if (first == KZG355_OK) first = rc;
    }
    return first;
}

// What is decided once for the whole call, whatever runs it afterwards
static int blob_impl(bool *ok, int *status, uint8_t *dbg, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs, size_t n, size_t groups,
                     const kzg355_settings *cs, bool device = false, int interp_form = 0, int prep_form = 0) {
    if (!ok) return refuse_call(status, groups, KZG355_BADARGS);
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    if (!cs) return refuse(KZG355_BADARGS);
    if (groups == 0) return KZG355_OK;
    if (interp_form < 0 || interp_form > 2 || prep_form < 0 || prep_form > 2) return refuse(KZG355_BADARGS);
    if (n == 0) {                                                 // verify_cell_kzg_proof_batch of no cells: true
        for (size_t i = 0; i < groups; i++) { ok[i] = true; if (status) status[i] = KZG355_OK; }
        if (dbg) memset(dbg, 0, (size_t)CELL_DEBUG_BYTES * groups);
        return KZG355_OK;
    }
    if (!blobs || !commitments || !proofs) return refuse(KZG355_BADARGS);
    if (device && (((uintptr_t)blobs & 15) || ((uintptr_t)commitments & 15) || ((uintptr_t)proofs & 15))) return refuse(KZG355_BADARGS);
    if (n > BLOB_CELLS_MAX_BLOBS || out_of_range(n, groups, MAX_BLOBS)) return refuse(KZG355_BADARGS);
    if (is_small(cs)) return refuse(KZG355_BADARGS);             // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    // device-resident arrays live on the handle's first device and stay there; host arrays: contiguous ranges of groups, as many replicas as groups
    if (cs->multi && !device) {
        const size_t D = cs->multi->rep.size();
        return fan_out(cs, groups < D ? groups : D, groups, [&](const kzg355_settings *rep, size_t g0, size_t cnt) -> int {
            const size_t b0 = g0 * n;
            return blob_single(ok + g0, status ? status + g0 : nullptr, dbg ? dbg + (size_t)CELL_DEBUG_BYTES * g0 : nullptr, blobs + HALF_BYTES * b0,
                               commitments + 48 * b0, proofs + 48 * CELLS_PER_EXT_BLOB * b0, n, cnt, rep, false, interp_form, 0);
        });
    }
    return blob_single(ok, status, dbg, blobs, commitments, proofs, n, groups, cs, device, interp_form, prep_form);
}

// ---- groups of different blob counts (the `_sets` entry points) --------------------------------------------------------------------------------
// `groups` non-empty whole groups on the device of cs, group g being blobs [boff[g], boff[g + 1]) of the three arrays (boff strictly increasing,
// boff[0] = 0, no group above BLOB_CELLS_MAX_BLOBS): launch sets of whole groups, taken in order while the set's blobs stay within
// BLOB_CELLS_MAX_BLOBS.  interp_form 0 is decided per launch set from its own blob total (blob_interp_form).
static int blob_sets_single(bool *ok, int *status, uint8_t *dbg, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs, const size_t *boff,
                            size_t groups, const kzg355_settings *cs, bool device, int interp_form, int prep_form) {
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    if ((rc = ensure_cc_consts(s, w)) || (rc = ensure_cell_setup(s, w))) return refuse(rc);
    int first = KZG355_OK;
    std::vector<size_t> sub;
    for (size_t g0 = 0; g0 < groups;) {
        size_t g1 = g0 + 1;                                       // (one group always fits)
        while (g1 < groups && boff[g1 + 1] - boff[g0] <= BLOB_CELLS_MAX_BLOBS) g1++;
        const size_t cnt = g1 - g0, b0 = boff[g0];
        sub.resize(cnt + 1);
        for (size_t i = 0; i <= cnt; i++) sub[i] = boff[g0 + i] - b0;
        rc = blob_set(s, w, ok + g0, status ? status + g0 : nullptr, dbg ? dbg + (size_t)CELL_DEBUG_BYTES * g0 : nullptr, blobs + HALF_BYTES * b0,
                      commitments + 48 * b0, proofs + 48 * CELLS_PER_EXT_BLOB * b0, 0, cnt, device, blob_interp_form(interp_form, sub[cnt]), prep_form,
                      sub.data());
        if (call_failed(rc)) return refuse(rc);
        if (first == KZG355_OK) first = rc;
        g0 = g1;
    }
    return first;
}

// What is decided once for the whole call: everything that refuses it, from the counts alone, before an array is read or a device touched (the
// order of cell_sets_impl, cells.hip).  An empty group is true / OK on the spot and takes no part in a launch set: the rest are numbered anew, so
// that the offsets the kernels see are strictly increasing, and their results go back to their places.  The arrays need no packing for that.
static const size_t BLOB_SETS_MAX_GROUPS = (size_t)1 << 24;
static int blob_sets_impl(bool *ok, int *status, uint8_t *dbg, const size_t *counts, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs,
                          size_t groups, const kzg355_settings *cs, bool device = false, int interp_form = 0, int prep_form = 0) {
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    if (!cs || !ok || (groups > 0 && !counts)) return refuse(KZG355_BADARGS);
    if (groups == 0) return KZG355_OK;
    if (groups > BLOB_SETS_MAX_GROUPS) return refuse(KZG355_BADARGS);
    if (interp_form < 0 || interp_form > 2 || prep_form < 0 || prep_form > 2) return refuse(KZG355_BADARGS);
    size_t total = 0, live = 0;
    for (size_t g = 0; g < groups; g++) {
        // a group is one launch set at most; the sum is not limited, but it and its bytes (131072 per blob) must fit size_t
        if (counts[g] > BLOB_CELLS_MAX_BLOBS || counts[g] > SIZE_MAX / HALF_BYTES - total) return refuse(KZG355_BADARGS);
        total += counts[g];
        live += counts[g] != 0;
    }
    if (total > 0 && (!blobs || !commitments || !proofs)) return refuse(KZG355_BADARGS);
    if (device && total > 0 && (((uintptr_t)blobs & 15) || ((uintptr_t)commitments & 15) || ((uintptr_t)proofs & 15))) return refuse(KZG355_BADARGS);
    if (is_small(cs)) return refuse(KZG355_BADARGS);             // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    // the non-empty groups: where each came from, and the blobs before each
    std::vector<size_t> from(live), boff(live + 1, 0);
    for (size_t g = 0, l = 0; g < groups; g++) {
        if (counts[g] == 0) {                                     // verify_cell_kzg_proof_batch of no cells: true
            ok[g] = true;
            if (status) status[g] = KZG355_OK;
            if (dbg) memset(dbg + (size_t)CELL_DEBUG_BYTES * g, 0, CELL_DEBUG_BYTES);
            continue;
        }
        from[l] = g;
        boff[l + 1] = boff[l] + counts[g];
        l++;
    }
    if (live == 0) return KZG355_OK;
    // results in the order of the non-empty groups (std::vector<bool> has no bool array to hand out)
    std::unique_ptr<bool[]> l_ok(new bool[live]());
    std::vector<int> l_st(live, KZG355_OK);
    std::vector<uint8_t> l_dbg(dbg ? (size_t)CELL_DEBUG_BYTES * live : 0);
    auto run = [&](const kzg355_settings *on, size_t l0, size_t k, bool dev, int pf) -> int {
        // groups l0 .. l0 + k - 1: their arrays start at blob boff[l0], their offsets count from there
        const size_t b0 = boff[l0];
        std::vector<size_t> sub(k + 1);
        for (size_t i = 0; i <= k; i++) sub[i] = boff[l0 + i] - b0;
        const int rc = blob_sets_single(l_ok.get() + l0, l_st.data() + l0, dbg ? l_dbg.data() + (size_t)CELL_DEBUG_BYTES * l0 : nullptr,
                                        blobs + HALF_BYTES * b0, commitments + 48 * b0, proofs + 48 * CELLS_PER_EXT_BLOB * b0, sub.data(), k, on, dev,
                                        interp_form, pf);
        return call_failed(rc) ? refuse_call(l_st.data() + l0, k, rc, l_ok.get() + l0) : rc;      // (a failure of the range is every group's of the range)
    };
    // Device-resident arrays live on the handle's first device and stay there.  Host arrays on a handle over several devices: contiguous ranges
    // of the non-empty groups, equal in GROUPS, each range's arrays starting at its own sum of counts.  A group is never cut; the ranges can be
    // uneven in blobs (balancing them by blobs is not done, and nothing here was measured on several cards).
    int rc;
    if (cs->multi && !device) {
        const size_t D = cs->multi->rep.size();
        rc = fan_out(cs, live < D ? live : D, live, [&](const kzg355_settings *rep, size_t l0, size_t k) -> int { return run(rep, l0, k, false, 0); });
    } else {
        rc = run(cs, 0, live, device, prep_form);
    }
    int first = KZG355_OK;
    for (size_t l = 0; l < live; l++) {
        const size_t g = from[l];
        ok[g] = l_ok[l];
        if (status) status[g] = l_st[l];
        if (dbg) memcpy(dbg + (size_t)CELL_DEBUG_BYTES * g, l_dbg.data() + (size_t)CELL_DEBUG_BYTES * l, CELL_DEBUG_BYTES);
        if (l_st[l] != KZG355_OK && first == KZG355_OK) first = l_st[l];
    }
    return call_failed(rc) ? rc : first;
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_verify_blob_cell_proofs_batch_many(bool *ok, int *status, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *cell_proofs,
                                              size_t n_per_group, size_t groups, const kzg355_settings *s) {
    return blob_impl(ok, status, nullptr, blobs, commitments, cell_proofs, n_per_group, groups, s);
}

int kzg355_verify_blob_cell_proofs_batch(bool *ok, const uint8_t *blobs, size_t n_blobs, const uint8_t *commitments, size_t n_commitments,
                                         const uint8_t *cell_proofs, size_t n_cell_proofs, const kzg355_settings *s) {
    if (!s || !ok) return KZG355_BADARGS;
    if (n_commitments != n_blobs || n_blobs > BLOB_CELLS_MAX_BLOBS || n_cell_proofs != (size_t)CELLS_PER_EXT_BLOB * n_blobs) return KZG355_BADARGS;
    bool r = false; int st = KZG355_OK;
    const int rc = blob_impl(&r, &st, nullptr, blobs, commitments, cell_proofs, n_blobs, 1, s);
    if (rc == KZG355_OK) *ok = r;
    return rc;
}

int kzg355_verify_blob_cell_proofs_batch_many_device(bool *ok, int *status, const uint8_t *d_blobs, const uint8_t *d_commitments, const uint8_t *d_cell_proofs,
                                                     size_t n_per_group, size_t groups, const kzg355_settings *s) {
    return blob_impl(ok, status, nullptr, d_blobs, d_commitments, d_cell_proofs, n_per_group, groups, s, true);
}

int kzg355_debug_blob_cell_batch_intermediates(uint8_t *out, bool *ok, int *status, const uint8_t *blobs, const uint8_t *commitments,
                                               const uint8_t *cell_proofs, size_t n_per_group, size_t groups, int interp_form, const kzg355_settings *s) {
    if (!out) return refuse_call(status, groups, KZG355_BADARGS, ok);
    return blob_impl(ok, status, out, blobs, commitments, cell_proofs, n_per_group, groups, s, false, interp_form, 0);
}

int kzg355_debug_blob_cell_batch_intermediates_device(uint8_t *out, bool *ok, int *status, const uint8_t *d_blobs, const uint8_t *d_commitments,
                                                      const uint8_t *d_cell_proofs, size_t n_per_group, size_t groups, int interp_form, int prep_form,
                                                      const kzg355_settings *s) {
    if (!out) return refuse_call(status, groups, KZG355_BADARGS, ok);
    return blob_impl(ok, status, out, d_blobs, d_commitments, d_cell_proofs, n_per_group, groups, s, true, interp_form, prep_form);
}

int kzg355_verify_blob_cell_proofs_batch_many_sets(bool *ok, int *status, const size_t *blob_counts, const uint8_t *blobs, const uint8_t *commitments,
                                                   const uint8_t *cell_proofs, size_t groups, const kzg355_settings *s) {
    return blob_sets_impl(ok, status, nullptr, blob_counts, blobs, commitments, cell_proofs, groups, s);
}

int kzg355_verify_blob_cell_proofs_batch_many_sets_device(bool *ok, int *status, const size_t *blob_counts, const uint8_t *d_blobs,
                                                          const uint8_t *d_commitments, const uint8_t *d_cell_proofs, size_t groups,
                                                          const kzg355_settings *s) {
    return blob_sets_impl(ok, status, nullptr, blob_counts, d_blobs, d_commitments, d_cell_proofs, groups, s, true);
}

int kzg355_debug_blob_cell_batch_intermediates_sets(uint8_t *out, bool *ok, int *status, const size_t *blob_counts, const uint8_t *blobs,
                                                    const uint8_t *commitments, const uint8_t *cell_proofs, size_t groups, int interp_form,
                                                    const kzg355_settings *s) {
    if (!out) return refuse_call(status, groups, KZG355_BADARGS, ok);
    return blob_sets_impl(ok, status, out, blob_counts, blobs, commitments, cell_proofs, groups, s, false, interp_form, 0);
}

int kzg355_debug_blob_cell_batch_intermediates_sets_device(uint8_t *out, bool *ok, int *status, const size_t *blob_counts, const uint8_t *d_blobs,
                                                           const uint8_t *d_commitments, const uint8_t *d_cell_proofs, size_t groups, int interp_form,
                                                           int prep_form, const kzg355_settings *s) {
    if (!out) return refuse_call(status, groups, KZG355_BADARGS, ok);
    return blob_sets_impl(ok, status, out, blob_counts, d_blobs, d_commitments, d_cell_proofs, groups, s, true, interp_form, prep_form);
}

#pragma GCC visibility pop
}  // extern "C"
