// cells.hip -- the C entry points of verify_cell_kzg_proof_batch (EIP-7594 cells; include/kzg355.h) and the per-handle setup they need (host side
// of libkzg355.so; see engine.h).  The host deduplicates the commitments, sorts every group's cells by column and hashes its transcript (one group
// per host-pool task); the kernels of k_cells.hip and the shared point / pairing kernels do the rest in one set of launches for all groups.
#include "engine.h"

#include <string_view>
#include <unordered_map>

namespace kzg355_impl {

// The first cell call of a handle: constants, the 64 monomial points [tau^t]_1 (build_monomial_points, cell_compute.hip) and the line table of
// [tau^64]_2.  Under cell_mu.  A failure releases what was being filled and is not remembered: the next call tries again (engine.h, at cell_mu).
int ensure_cell_setup(kzg355_settings *s, Workspace *w) {
    std::lock_guard<std::mutex> lk(s->cell_mu);
    if (s->cell_ready) return KZG355_OK;
    DevBuf err, g2b;
    auto done = [&](int rc) {
        for (DevBuf *b : {&err, &g2b}) b->release();
        if (rc != KZG355_OK)
            for (DevBuf *b : {&s->cell_consts, &s->cell_mono, &s->cell_mono48, &s->cell_lines, &s->cell_lines_w, &s->cell_lines_inf}) b->release();
        s->cell_ready = rc == KZG355_OK;
        return rc;
    };
    int rc;
    if ((rc = s->cell_consts.ensure(sizeof(CellConsts))) || (rc = s->cell_mono.ensure(sizeof(G1Affine) * CELL_FE)) ||
        (rc = s->cell_mono48.ensure(48 * CELL_FE)) || (rc = s->cell_lines.ensure(sizeof(LineCoeff) * 3 * N_LINES)) ||
        (rc = s->cell_lines_w.ensure(sizeof(LineW) * 3 * N_LINES)) || (rc = s->cell_lines_inf.ensure(sizeof(int) * 3)) ||
        (rc = err.ensure(sizeof(int))) || (rc = g2b.ensure(96)) ||
        (rc = build_monomial_points(s, w, CELL_FE, s->cell_mono48.as<uint8_t>(), s->cell_mono.as<G1Affine>())))
        return done(rc);
    hipStream_t st = w->stream;
    auto hip_fail = [&]() { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return done(KZG355_DEVICE_ERROR); };
    // slots 0 and 1 as the blob path has them (slot 0: G2 generator), slot 2 rebuilt from g2[64]
    if (hipMemcpyAsync(s->cell_lines.p, s->t.lines, sizeof(LineCoeff) * 3 * N_LINES, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s->cell_lines_inf.p, s->t.lines_inf, sizeof(int) * 3, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(g2b.p, s->g2_tau64, 96, hipMemcpyHostToDevice, st) != hipSuccess || hipMemsetAsync(err.p, 0, sizeof(int), st) != hipSuccess)
        return hip_fail();
    DeviceTables ct = s->t;
    ct.lines = s->cell_lines.as<LineCoeff>();
    ct.lines_w = s->cell_lines_w.as<LineW>();
    ct.lines_inf = s->cell_lines_inf.as<int>();
    launch_cell_setup(g2b.as<uint8_t>(), s->cell_consts.as<CellConsts>(), ct.lines, ct.lines_inf, err.as<int>(), st);
    launch_lines_to_w(ct, st);
    int herr = 0;
    if (hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
        hipGetLastError() != hipSuccess)
        return hip_fail();
    if (herr) return done(KZG355_INTERNAL);                        // (load validated g2[64]: its bytes decode)
    s->cell_t = ct;
    return done(KZG355_OK);
}

// What the host prepares per group: the unique commitments (padded to n with the encoding of infinity, weight 0), each cell's position in
// that list, the cells sorted by column (perm, global cell numbers) with one segment per column present, and the transcript digest.
struct CellHostGroup { int n_segs = 0; bool bad_index = false; };
struct CellHostPrep {
    std::vector<uint8_t> uc, dig;            // 48 N, 32 groups
    std::vector<int> meta;                   // segments (int4, first: 16-byte aligned) | gseg[G + 1] | cell index | commitment position | perm
    std::vector<CellHostGroup> hg;
    int S = 0;                               // segments of all groups
};
// The preparation has two pieces.  One hashes: a group's transcript over all its cells, with the commitments deduplicated over the whole group.
// The other deduplicates and column-sorts a RANGE of a group's cells, which is all the kernels need of it.  A whole group is the range of all
// its cells and shares one dedup between the two; a group cut over several devices (cell_multi_sharded) is hashed once and its blocks are
// ranges of their own.
// the unique commitments among `count` in order of first appearance into uc (48 per slot, padded to `count` slots with the encoding of infinity),
// every entry's slot into cidx; returns how many there are
int cell_dedup(const uint8_t *commitments, size_t count, uint8_t *uc, int *cidx) {
    std::unordered_map<std::string_view, int> seen;
    seen.reserve(count * 2);
    int u = 0;
    for (size_t k = 0; k < count; k++) {
        const std::string_view key(reinterpret_cast<const char *>(commitments + 48 * k), 48);
        auto it = seen.find(key);
        int pos;
        if (it == seen.end()) {
            pos = u++;
            memcpy(uc + 48 * pos, key.data(), 48);
            seen.emplace(key, pos);                             // (the key views caller memory, which outlives the map)
        } else {
            pos = it->second;
        }
        cidx[k] = pos;
    }
    for (size_t i = u; i < count; i++) { memset(uc + 48 * i, 0, 48); uc[48 * i] = 0xc0; }      // infinity, weight 0
    return u;
}
// the transcript digest of one group of npg cells whose u unique commitments are uc, entry k carrying commitment cidx[k]
static void cell_transcript(const kzg355_settings *s, const uint8_t *uc, int u, const int *cidx, const size_t *cell_indices, const uint8_t *cells,
                            const uint8_t *proofs, size_t npg, uint8_t *dig) {
    const size_t len = 16 + 32 + 48 * (size_t)u + npg * (16 + CELL_BYTES + 48);
    std::vector<uint8_t> msg(len);
    uint8_t *p = msg.data();
    memcpy(p, CELL_DOMAIN, 16); p += 16;
    put_u64be(p, N_FE); put_u64be(p + 8, CELL_FE); put_u64be(p + 16, (uint64_t)u); put_u64be(p + 24, npg); p += 32;
    memcpy(p, uc, 48 * (size_t)u); p += 48 * (size_t)u;
    for (size_t k = 0; k < npg; k++) {
        put_u64be(p, (uint64_t)cidx[k]); put_u64be(p + 8, cell_indices[k]); p += 16;
        memcpy(p, cells + (size_t)CELL_BYTES * k, CELL_BYTES); p += CELL_BYTES;
        memcpy(p, proofs + 48 * k, 48); p += 48;
    }
    kzg_host::sha256(dig, msg.data(), len, s->sha_impl);
}
// the digests alone, of `groups` whole groups of npg cells (32 bytes each into dig); one group per host-pool task
static void cell_host_digests(kzg355_settings *s, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                              size_t npg, size_t groups, uint8_t *dig) {
    auto one = [&](size_t gi) {
        const size_t base = gi * npg;
        std::vector<uint8_t> uc(48 * npg);
        std::vector<int> cidx(npg);
        const int u = cell_dedup(commitments + 48 * base, npg, uc.data(), cidx.data());
        cell_transcript(s, uc.data(), u, cidx.data(), cell_indices + base, cells + (size_t)CELL_BYTES * base, proofs + 48 * base, npg, dig + 32 * gi);
    };
    if (s->host_pool && groups > 1) s->host_pool->parallel_for(groups, one);
    else for (size_t gi = 0; gi < groups; gi++) one(gi);
}
// The four arrays in host memory (the caller's, or a device-resident call's copied back) -> hp; one group per host-pool task.  A launch set
// takes cells [off, off + cnt) of every group of npg, numbered gi * cnt + k on the device.  The whole group (off 0, cnt npg) is hashed here from
// the same dedup; a block of it leaves hp.dig alone (the group's digest covers all its cells: cell_host_digests).
// goff (groups + 1 entries, strictly increasing; npg, off and cnt are then unused): groups of different sizes, each whole -- group gi is entries
// [goff[gi], goff[gi + 1]) of the caller's arrays and the same cell numbers on the device -- and the meta buffer ends with what the `_sets`
// kernels find a group by: goff as ints, then the group of every cell.
static void cell_host_prep(kzg355_settings *s, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs, size_t npg,
                           size_t groups, CellHostPrep &hp, size_t off, size_t cnt_all, const size_t *goff = nullptr) {
    const bool whole = goff || (off == 0 && cnt_all == npg);
    const int G = (int)groups;
    const size_t N = goff ? goff[groups] : cnt_all * groups;
    // a group has at most min(its cells, 128) segments; until they are packed, group gi's start at seg_at(gi)
    const size_t seg_cap = cnt_all < (size_t)CELLS_PER_EXT_BLOB ? cnt_all : (size_t)CELLS_PER_EXT_BLOB;
    auto seg_at = [&](size_t gi) { return goff ? goff[gi] : gi * seg_cap; };
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> &h_uc = hp.uc, &h_dig = hp.dig;
    h_uc.resize(48 * N);
    if (whole) h_dig.resize(32 * groups);
    std::vector<int> h_cell(N), h_cidx(N), h_perm(N);
    std::vector<int4> h_seg_local(goff ? N : groups * seg_cap);
    std::vector<CellHostGroup> &hg = hp.hg;
    hg.assign(groups, CellHostGroup());
    auto prep = [&](size_t gi) {
        // the range on the device and in the caller's arrays, and its length
        const size_t base = goff ? goff[gi] : gi * cnt_all, src = goff ? goff[gi] : gi * npg + off, cnt = goff ? goff[gi + 1] - goff[gi] : cnt_all;
        CellHostGroup &gr = hg[gi];
        for (size_t k = 0; k < cnt; k++) {
            const size_t c = cell_indices[src + k];
            if (c >= (size_t)CELLS_PER_EXT_BLOB) gr.bad_index = true;
            h_cell[base + k] = c < (size_t)CELLS_PER_EXT_BLOB ? (int)c : 0;
        }
        uint8_t *uc = h_uc.data() + 48 * base;
        const int u = cell_dedup(commitments + 48 * src, cnt, uc, h_cidx.data() + base);
        // counting sort by column
        int ccnt[CELLS_PER_EXT_BLOB] = {0}, at[CELLS_PER_EXT_BLOB];
        for (size_t k = 0; k < cnt; k++) ccnt[h_cell[base + k]]++;
        int acc = 0;
        for (int c = 0; c < CELLS_PER_EXT_BLOB; c++) {
            at[c] = acc;
            if (ccnt[c]) h_seg_local[seg_at(gi) + gr.n_segs++] = make_int4((int)gi, c, (int)base + acc, ccnt[c]);
            acc += ccnt[c];
        }
        for (size_t k = 0; k < cnt; k++) h_perm[base + at[h_cell[base + k]]++] = (int)(base + k);
        if (whole)
            cell_transcript(s, uc, u, h_cidx.data() + base, cell_indices + src, cells + (size_t)CELL_BYTES * src, proofs + 48 * src, cnt, h_dig.data() + 32 * gi);
    };
    if (s->host_pool && groups > 1) s->host_pool->parallel_for(groups, prep);
    else for (size_t gi = 0; gi < groups; gi++) prep(gi);
    std::vector<int> h_gseg(groups + 1, 0);
    for (int gi = 0; gi < G; gi++) h_gseg[gi + 1] = h_gseg[gi] + hg[gi].n_segs;
    const int S = hp.S = h_gseg[G];
    std::vector<int> &meta = hp.meta;
    meta.resize((size_t)4 * S + (G + 1) + 3 * N + (goff ? (G + 1) + N : 0));
    {
        int4 *sg = reinterpret_cast<int4 *>(meta.data());
        for (int gi = 0; gi < G; gi++) memcpy(sg + h_gseg[gi], h_seg_local.data() + seg_at(gi), sizeof(int4) * hg[gi].n_segs);
        int *q = meta.data() + 4 * (size_t)S;
        memcpy(q, h_gseg.data(), sizeof(int) * (G + 1)); q += G + 1;
        memcpy(q, h_cell.data(), sizeof(int) * N); q += N;
        memcpy(q, h_cidx.data(), sizeof(int) * N); q += N;
        memcpy(q, h_perm.data(), sizeof(int) * N); q += N;
        if (goff) {
            for (int gi = 0; gi <= G; gi++) q[gi] = (int)goff[gi];
            q += G + 1;
            for (int gi = 0; gi < G; gi++) std::fill(q + goff[gi], q + goff[gi + 1], gi);
        }
    }
    const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (s->timing) { std::lock_guard<std::mutex> lk(s->mu); auto &k = s->last_ms["cell_host"]; k.last = host_ms; k.total += host_ms; k.count++; }
}

// How a device-resident call (the *_device entry points) is prepared: on the device (k_cell_prep.hip), or -- the four arrays copied back into
// pinned memory -- by the host preparation above.  A transcript is one serial SHA-256 chain per group, and the card runs a chain at 1.7-1.9 us
// per 64-byte block alone and 6.9 us with 128 groups at once, against a host pool that hashes 128 groups of 135 KB in 0.6 ms; so the host
// prepares when a group's transcript exceeds CELL_PREP_HOST_FROM_BYTES and the groups per compute unit stay below
// CELL_PREP_HOST_UPTO_GROUPS_PER_CU.
// The bytes are MEASURED ("device-resident cell calls"): of the six shapes of the cell-verify table the device preparation ties
// at one cell per group (2.2 KB) and loses from six cells (12.9 KB: 1.4 ms of hashing against 0.1 ms) upwards, the loss growing with the bytes;
// 4 KiB lies between the two.  The groups per compute unit are still DERIVED, not measured (the table has no shape above 128 groups): the blob
// path's device chain of 131 KB loses to its host route up to about 1500 blobs = 6 per compute unit
// (profiles/r05/device_host_hash_crossover.txt), where the one-lane-per-message form has taken over.
static const size_t CELL_PREP_HOST_FROM_BYTES = (size_t)4 << 10;
static const int CELL_PREP_HOST_UPTO_GROUPS_PER_CU = 6;
bool cell_device_call_prepares_on_host(const kzg355_settings *s, size_t npg, size_t groups, int prep_form) {
    if (npg > (size_t)CELL_PREP_MAX_CELLS) return true;           // above the device preparation's cap every form takes the host's
    if (prep_form) return prep_form == 2;
    const size_t bytes = 16 + 32 + 48 + npg * (16 + CELL_BYTES + 48);          // (48 more per further unique commitment)
    return bytes > CELL_PREP_HOST_FROM_BYTES && groups < (size_t)CELL_PREP_HOST_UPTO_GROUPS_PER_CU * (size_t)s->cu_count;
}

// What cell_single and a stage-1 block of cell_multi_sharded share: the buffers of a launch set, the upload of a host-prepared one and the chain.
// The workspace's buffers by role: blobs = cells, commitments = unique commitments, q = meta, z = r powers, y = column coefficients, scal_a =
// lincomb scalars, partials = lincomb terms, lc_partials = the three sums per group, out48 = r | debug output.  N = n * groups cells, S segments;
// host_input: cells and proofs are uploaded (else read where the caller has them).
// N cells and `terms` lincomb terms in all groups together
int cell_reserve_sized(Workspace *w, bool host_input, size_t N, size_t terms, size_t groups, int S, size_t meta_ints) {
    int rc;
    if ((host_input && ((rc = w->blobs.ensure((size_t)CELL_BYTES * N)) || (rc = w->proofs.ensure(48 * N)))) || (rc = w->commitments.ensure(48 * N)) ||
        (rc = w->pts.ensure(sizeof(G1Affine) * 2 * N)) || (rc = w->digests.ensure(32 * groups)) || (rc = w->q.ensure(sizeof(int) * meta_ints)) ||
        (rc = w->z.ensure(sizeof(Fr) * N)) || (rc = w->y.ensure(sizeof(Fr) * CELL_FE * (size_t)(S > 0 ? S : 1))) ||
        (rc = w->scal_a.ensure(sizeof(uint32_t) * 8 * terms)) || (rc = w->partials.ensure(sizeof(G1Jac) * terms)) ||
        (rc = w->lc_partials.ensure(sizeof(G1Jac) * 3 * groups)) || (rc = w->pair_pts.ensure(sizeof(PairPt) * 2 * groups)) ||
        (rc = w->ok.ensure(sizeof(int) * groups)) || (rc = w->err.ensure(sizeof(int) * groups)) || (rc = w->h_ok.ensure(sizeof(int) * groups)) ||
        (rc = w->h_err.ensure(sizeof(int) * groups)) || (rc = w->out48.ensure((size_t)(32 + CELL_DEBUG_BYTES) * groups)) ||
        (rc = w->h_out.ensure((size_t)CELL_DEBUG_BYTES * groups)))
        return rc;
    return KZG355_OK;
}
int cell_reserve(Workspace *w, bool host_input, int n, size_t groups, int S, size_t meta_ints) {
    return cell_reserve_sized(w, host_input, (size_t)n * groups, (size_t)cell_terms(n) * groups, groups, S, meta_ints);
}
// hp and the digests up; with host arrays (cells, proofs not null) also cells [off, off + cnt) of every group of npg and their proofs, group after group.
// sets_N: the launch set is sets_N cells in whole groups of different sizes (npg, off and cnt are unused)
static int cell_upload(Workspace *w, const CellHostPrep &hp, const uint8_t *dig, const uint8_t *cells, const uint8_t *proofs, size_t npg, size_t off,
                       size_t cnt, size_t groups, size_t sets_N = 0) {
    hipStream_t st = w->stream;
    const bool back_to_back = sets_N || cnt == npg;               // whole groups lie back to back
    const size_t N = sets_N ? sets_N : cnt * groups;
    HIPCHK(hipMemcpyAsync(w->commitments.p, hp.uc.data(), 48 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->q.p, hp.meta.data(), sizeof(int) * hp.meta.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->digests.p, dig, 32 * groups, hipMemcpyHostToDevice, st));
    if (!cells) return KZG355_OK;
    const size_t runs = back_to_back ? 1 : groups, len = back_to_back ? N : cnt;
    for (size_t g = 0; g < runs; g++) {
        const size_t src = g * npg + off, dst = g * cnt;
        HIPCHK(hipMemcpyAsync(w->proofs.as<uint8_t>() + 48 * dst, proofs + 48 * src, 48 * len, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(w->blobs.as<uint8_t>() + (size_t)CELL_BYTES * dst, cells + (size_t)CELL_BYTES * src, (size_t)CELL_BYTES * len, hipMemcpyHostToDevice,
                              st));
    }
    return KZG355_OK;
}
// The chain on prepared buffers: points, scalars with weights r^(k0 + k), interpolation, then the three sums per group in lc_partials -- and, with
// finish, the pairing arguments (d_dbg or null: the debug bytes).  A block of a cut group stops at the sums (k_cell_merge ends it elsewhere).
// The points need no digest: a caller that hashes on the host while they run (blob_cells.hip) queues cell_chain_points itself and says so
// (points_queued).  bi: the groups are whole blobs and the interpolation starts from their coefficients (k_blob_cells.hip), not from the cells.
void cell_chain_points(Workspace *w, Timed &tm, const uint8_t *d_proofs, int n, int G) {
    const size_t N = (size_t)n * G;
    hipStream_t st = w->stream;
    tm.begin("cell_points");
    launch_decompress_points(w->commitments.as<uint8_t>(), d_proofs, (int)N, n, w->pts.as<G1Affine>(), w->err.as<int>(), st);
    launch_subgroup_points(w->pts.as<G1Affine>(), (int)N, n, w->err.as<int>(), st);
    tm.end();
}
void cell_chain_points_sets(Workspace *w, Timed &tm, const uint8_t *d_proofs, int S, size_t N, int G) {
    const int *d_goff = w->q.as<int>() + 4 * (size_t)S + (G + 1) + 3 * N, *d_cgrp = d_goff + G + 1;
    tm.begin("cell_points");
    launch_cell_points_sets(w->commitments.as<uint8_t>(), d_proofs, d_goff, d_cgrp, (int)N, w->pts.as<G1Affine>(), w->err.as<int>(), w->stream);
    tm.end();
}
// sets_N (not with k0): the launch set is sets_N cells in G whole groups of different sizes, n is unused, and the meta buffer ends with the group
// offsets and the group of every cell (cell_host_prep with goff; blob_cells.hip writes the same): the `_sets` entries of the same kernel bodies
// run, then k_cell_finish and the pairing as for any launch set.  points_queued: the caller has queued cell_chain_points_sets; bi: the groups are
// whole blobs of different counts, bi->f their coefficients blob after blob (bi->n_blobs is unused: the offsets give every group's count).
void cell_chain(kzg355_settings *s, Workspace *w, Timed &tm, const uint8_t *d_cells, const uint8_t *d_proofs, int S, int n, int G, int k0, bool finish,
                uint8_t *d_dbg, bool points_queued, const BlobInterp *bi, size_t sets_N) {
    const size_t N = sets_N ? sets_N : (size_t)n * G;
    hipStream_t st = w->stream;
    const int4 *d_segs = w->q.as<int4>();
    const int *d_gseg = w->q.as<int>() + 4 * (size_t)S, *d_cell = d_gseg + G + 1, *d_cidx = d_cell + N, *d_perm = d_cidx + N;
    uint8_t *d_r = w->out48.as<uint8_t>();
    if (sets_N) {
        const int *d_goff = d_perm + N, *d_cgrp = d_goff + G + 1;
        if (!points_queued) cell_chain_points_sets(w, tm, d_proofs, S, N, G);
        tm.begin("cell_scalars");
        launch_cell_scalars_sets(w->digests.as<uint8_t>(), d_cell, d_cidx, d_goff, d_cgrp, (int)N, s->cell_consts.as<CellConsts>(), w->z.as<Fr>(),
                                 w->scal_a.as<uint32_t>(), d_r, st);
        tm.end();
        tm.begin("cell_interp");
        if (bi) launch_blob_cell_coefs_sets(bi->f, w->z.as<Fr>(), s->cc_consts.as<CellComputeConsts>(), d_goff, G, bi->W, w->y.as<Fr>(), st);
        launch_cell_interp_sets(d_cells, d_perm, d_segs, bi ? 0 : S, d_gseg, w->z.as<Fr>(), s->cell_consts.as<CellConsts>(), d_goff, G, w->y.as<Fr>(),
                                w->scal_a.as<uint32_t>(), w->err.as<int>(), st);
        tm.end();
        tm.begin("cell_lincomb");
        launch_cell_lincomb_sets(w->pts.as<G1Affine>(), s->cell_mono.as<G1Affine>(), w->scal_a.as<uint32_t>(), d_goff, (int)N, G, w->partials.as<G1Jac>(),
                                 w->lc_partials.as<G1Jac>(), d_r, w->pair_pts.as<PairPt>(), d_dbg, st);
        tm.end();
        return;
    }
    if (!points_queued) cell_chain_points(w, tm, d_proofs, n, G);
    tm.begin("cell_scalars");
    launch_cell_scalars(w->digests.as<uint8_t>(), d_cell, d_cidx, n, G, k0, s->cell_consts.as<CellConsts>(), w->z.as<Fr>(), w->scal_a.as<uint32_t>(), d_r, st);
    tm.end();
    tm.begin("cell_interp");
    if (bi) launch_blob_cell_coefs(bi->f, w->z.as<Fr>(), s->cc_consts.as<CellComputeConsts>(), bi->n_blobs, G, bi->W, w->y.as<Fr>(), st);
    launch_cell_interp(d_cells, d_perm, d_segs, bi ? 0 : S, d_gseg, w->z.as<Fr>(), s->cell_consts.as<CellConsts>(), n, G, w->y.as<Fr>(),
                       w->scal_a.as<uint32_t>(), w->err.as<int>(), st);
    tm.end();
    tm.begin("cell_lincomb");
    if (finish)
        launch_cell_lincomb(w->pts.as<G1Affine>(), s->cell_mono.as<G1Affine>(), w->scal_a.as<uint32_t>(), n, G, w->partials.as<G1Jac>(),
                            w->lc_partials.as<G1Jac>(), d_r, w->pair_pts.as<PairPt>(), d_dbg, st);
    else
        launch_cell_sums(w->pts.as<G1Affine>(), s->cell_mono.as<G1Affine>(), w->scal_a.as<uint32_t>(), n, G, w->partials.as<G1Jac>(), w->lc_partials.as<G1Jac>(), st);
    tm.end();
}

// One set of launches for `groups` whole groups on the device of cs (a replica, for a handle over several devices); the arguments are checked.
// device = false: the four arrays are host memory (the launch sequence of the host-buffer calls).  device = true: they are device memory on the
// handle's device; prep_form 0 by size, 1 device preparation, 2 copy back and prepare on the host.
// goff (groups + 1 entries, strictly increasing; npg is unused): the groups have their own sizes, group i being entries [goff[i], goff[i + 1])
// of the four arrays, host or device.  With device arrays the route is chosen from the largest group and the number of groups (the rule of
// blob_cells.hip's launch sets; measured on uniform shapes only), and one group above CELL_PREP_MAX_CELLS sends the whole call to the host
// preparation.  The device preparation gets goff and gseg from here (2 (groups + 1) ints); no per-cell array crosses PCIe.
static int cell_single(bool *ok, int *status, uint8_t *dbg, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                       size_t npg, size_t groups, const kzg355_settings *cs, bool device, int prep_form, const size_t *goff = nullptr) {
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    if ((rc = ensure_cell_setup(s, w))) return refuse(rc);
    s->n_cell_sets.fetch_add(1);
    const int n = (int)npg, G = (int)groups;
    const size_t N = goff ? goff[groups] : npg * groups;
    const int seg_cap = n < CELLS_PER_EXT_BLOB ? n : CELLS_PER_EXT_BLOB;
    hipStream_t st = w->stream;
    size_t n_max = goff ? 0 : npg;                                // the largest group
    if (goff) for (size_t i = 0; i < groups; i++) n_max = std::max(n_max, goff[i + 1] - goff[i]);

    // ---- prepare: dedup, column sort, transcripts -- by the host from the caller's arrays, by the host from a copy of them, or on the device
    const bool dev_prep = device && !cell_device_call_prepares_on_host(s, n_max, groups, prep_form);
    CellHostPrep hp;
    if (!device) {
        cell_host_prep(s, commitments, cell_indices, cells, proofs, npg, groups, hp, 0, npg, goff);
    } else if (!dev_prep) {
        // into the workspace's pinned staging buffer (kept from call to call): indices | commitments | proofs | cells
        if ((rc = w->h_stage.ensure((sizeof(size_t) + 48 + 48 + (size_t)CELL_BYTES) * N))) return refuse(rc);
        size_t *b_idx = w->h_stage.as<size_t>();
        uint8_t *b_c = reinterpret_cast<uint8_t *>(b_idx + N), *b_p = b_c + 48 * N, *b_cells = b_p + 48 * N;
        HIPCHK(hipMemcpyAsync(b_idx, cell_indices, sizeof(size_t) * N, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b_c, commitments, 48 * N, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b_p, proofs, 48 * N, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b_cells, cells, (size_t)CELL_BYTES * N, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        cell_host_prep(s, b_c, b_idx, b_cells, b_p, npg, groups, hp, 0, npg, goff);
    }
    // meta buffer of the device preparation: the host's layout with min(count, 128) segments per group (groups of different sizes: then the
    // offsets and the group of every cell, as cell_chain reads them), then the unique-commitment counts and (tables too large for LDS) the
    // dedup tables -- tab_size slots per group, or with goff 4 per cell (k_cell_prep_sets)
    const int tab_size = dev_prep ? cell_prep_table_slots((int)n_max) : 0;
    const size_t gtab_ints = tab_size > CELL_PREP_LDS_SLOTS ? (goff ? 4 * N : (size_t)tab_size * groups) : 0;
    std::vector<int> h_geo;                                       // (device preparation with goff) gseg | goff
    if (dev_prep && goff) {
        h_geo.assign(2 * (groups + 1), 0);
        for (size_t i = 0; i < groups; i++) {
            h_geo[i + 1] = h_geo[i] + (int)std::min(goff[i + 1] - goff[i], (size_t)CELLS_PER_EXT_BLOB);
            h_geo[groups + 1 + i + 1] = (int)goff[i + 1];
        }
    }
    const int S = !dev_prep ? hp.S : goff ? h_geo[groups] : G * seg_cap;
    const size_t sets_ints = goff ? (G + 1) + N : 0;
    const size_t meta_ints = dev_prep ? (size_t)4 * S + (G + 1) + 3 * N + sets_ints + groups + gtab_ints : hp.meta.size();

    // ---- device
    if ((rc = goff ? cell_reserve_sized(w, !device, N, (size_t)cell_terms_sets((int)N, G), groups, S, meta_ints)
                   : cell_reserve(w, !device, n, groups, S, meta_ints)))
        return refuse(rc);
    Fp *f12 = nullptr;
    if (w->pair_f.ensure(pairing_f12_bytes(G)) == KZG355_OK) f12 = w->pair_f.as<Fp>();
    if ((rc = launch_set_begin(w, groups, true))) return rc;       // (cell_reserve has sized the words)
    Timed tm(s, w);
    const uint8_t *d_cells = device ? cells : w->blobs.as<uint8_t>(), *d_proofs = device ? proofs : w->proofs.as<uint8_t>();
    uint8_t *d_dbg = dbg ? w->out48.as<uint8_t>() + 32 * groups : nullptr;
    if (dev_prep) {
        int *m = w->q.as<int>() + 4 * (size_t)S;
        int *d_cidx = m + (G + 1) + N, *d_goff = m + (G + 1) + 3 * N, *d_ucount = d_goff + sets_ints, *d_gtab = gtab_ints ? d_ucount + groups : nullptr;
        if (goff) {                                               // (pageable: staged before the copies return)
            HIPCHK(hipMemcpyAsync(m, h_geo.data(), sizeof(int) * (G + 1), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_goff, h_geo.data() + (G + 1), sizeof(int) * (G + 1), hipMemcpyHostToDevice, st));
        }
        tm.begin("cell_prep");
        if (goff)
            launch_cell_prep_sets(commitments, cell_indices, d_goff, m, G, d_gtab, w->commitments.as<uint8_t>(), w->q.as<int4>(), m + (G + 1), d_cidx,
                                  m + (G + 1) + 2 * N, d_goff + (G + 1), d_ucount, w->err.as<int>(), st);
        else
            launch_cell_prep(commitments, cell_indices, n, G, tab_size, d_gtab, w->commitments.as<uint8_t>(), w->q.as<int4>(), m, m + (G + 1), d_cidx,
                             m + (G + 1) + 2 * N, d_ucount, w->err.as<int>(), st);
        tm.end();
        tm.begin("cell_rhash");
        if (goff)
            launch_cell_rhash_sets(w->commitments.as<uint8_t>(), cell_indices, cells, proofs, d_cidx, d_ucount, d_goff, G, G >= s->rhash_lanes_from,
                                   w->digests.as<uint8_t>(), st);
        else
            launch_cell_rhash(w->commitments.as<uint8_t>(), cell_indices, cells, proofs, d_cidx, d_ucount, n, G, G >= s->rhash_lanes_from,
                              w->digests.as<uint8_t>(), st);
        tm.end();
        s->n_cell_device_prep.fetch_add(1);
    } else if ((rc = cell_upload(w, hp, hp.dig.data(), device ? nullptr : cells, proofs, npg, 0, npg, groups, goff ? N : 0))) {
        return rc;
    }
    cell_chain(s, w, tm, d_cells, d_proofs, S, n, G, 0, true, d_dbg, false, nullptr, goff ? N : 0);
    tm.begin("cell_pairing");
    launch_pairing(w->pair_pts.as<PairPt>(), s->cell_t, G, w->ok.as<int>(), st, s->pairing_two_wave_upto, f12, s->pairing_hard12_from, s->miller_segments);
    tm.end();
    HIPCHK(hipGetLastError());
    if ((rc = launch_set_results(w, groups, true))) return rc;
    if (dbg) HIPCHK(hipMemcpyAsync(w->h_out.p, d_dbg, (size_t)CELL_DEBUG_BYTES * groups, hipMemcpyDeviceToHost, st));
    if ((rc = launch_set_wait(w, tm))) return rc;
    if (dbg) memcpy(dbg, w->h_out.p, (size_t)CELL_DEBUG_BYTES * groups);
    return launch_set_read(w, groups, status, 0, [&](size_t i, int &stt) {
        if (!dev_prep && hp.hg[i].bad_index) stt = KZG355_BADARGS;            // the host's own finding (the device preparation sets the error word)
        ok[i] = stt == KZG355_OK && w->h_ok.as<int>()[i] != 0;
    });
}

// ---- a handle over several devices (multi_device.hip) ------------------------------------------------------------------------------------------
// A group cut over the devices.  The check is linear in the cells once r is known: LL = sum r^k pi_k, RL = sum w_i C_i - [I(tau)]_1 +
// sum r^k h_k^64 pi_k, and I is a sum over the cells of r^k times a linear map of the cell.  So device d takes cells [off_d, off_d + cnt_d) of every
// group (off_d = n d / D, ragged allowed, cnt_d >= 1 by the rule of cell_multi), deduplicates and column-sorts its block on its own -- a
// commitment in two blocks is weighted in both, a column in two blocks is a segment in each -- and runs the chain of cell_single with weights
// r^(off_d + k) up to the three sums per group.  r comes from the group's transcript over ALL its cells, hashed once on the host.  The exchange is
// those three points per (block, group), copied to the group's stage-2 device g mod D, where k_cell_merge adds them and the pairing runs.
static int cell_multi_sharded(bool *ok, int *status, uint8_t *dbg, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells,
                              const uint8_t *proofs, size_t npg, size_t groups, const kzg355_settings *cs) {
    MultiDev *m = cs->multi;
    const size_t D = m->rep.size();
    const int G = (int)groups;
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    DeviceScope keep; keep.hold();               // this thread visits every replica's device below
    std::vector<size_t> cnt(D), off(D);
    for (size_t d = 0; d < D; d++) { off[d] = npg * d / D; cnt[d] = npg * (d + 1) / D - off[d]; }
    GuardList gs;                                                 // (whatever device the last guard leaves current, `keep` puts the caller's back)
    for (size_t d = 0; d < D; d++) if (!gs.add(m->rep[d])) return refuse(KZG355_NO_DEVICE);
    std::vector<uint8_t> h_dig(32 * groups);
    cell_host_digests(gs[0]->s, commitments, cell_indices, cells, proofs, npg, groups, h_dig.data());
    // stage 1: the block's three sums per group in lc_partials, r of every group in out48, its status per group in st1
    std::vector<std::vector<int>> st1(D, std::vector<int>(groups, KZG355_OK));
    {
        const int rc1 = fan_out_guards(gs, D, [&](size_t d) -> int {
            kzg355_settings *s = gs[d]->s; Workspace *w = gs[d]->w;
            int rc;
            if ((rc = ensure_cell_setup(s, w))) return rc;
            s->n_cell_sets.fetch_add(1);
            CellHostPrep hp;
            cell_host_prep(s, commitments, cell_indices, cells, proofs, npg, groups, hp, off[d], cnt[d]);
            if ((rc = cell_reserve(w, true, (int)cnt[d], groups, hp.S, hp.meta.size()))) return rc;
            if ((rc = launch_set_begin(w, groups))) return rc;
            Timed tm(s, w);
            if ((rc = cell_upload(w, hp, h_dig.data(), cells, proofs, npg, off[d], cnt[d], groups))) return rc;
            cell_chain(s, w, tm, w->blobs.as<uint8_t>(), w->proofs.as<uint8_t>(), hp.S, (int)cnt[d], G, (int)off[d], false, nullptr);
            HIPCHK(hipGetLastError());
            if ((rc = launch_set_results(w, groups)) || (rc = launch_set_wait(w, tm))) return rc;
            launch_set_read(w, groups, st1[d].data(), 0, [&](size_t g, int &stt) { if (hp.hg[g].bad_index) stt = KZG355_BADARGS; });
            return KZG355_OK;
        });
        if (rc1 != KZG355_OK) return refuse(rc1);
    }
    m->n_peer_exchanges++;
    // stage 2: group g on device g mod D, over the sums of all blocks
    {
        const int rc2 = fan_out_guards(gs, D < groups ? D : groups, [&](size_t t) -> int {
            kzg355_settings *s = gs[t]->s; Workspace *w = gs[t]->w;
            const size_t Gt = (groups - t + D - 1) / D;              // groups t, t + D, ...
            int rc;
            DevBuf &gath = w->records;                                 // [group of this device][block][3 sums]
            if ((rc = gath.ensure(sizeof(G1Jac) * 3 * D * Gt))) return rc;       // (pair_pts, ok, out48 ...: cell_reserve sized them for all groups)
            Fp *f12 = nullptr;
            if (w->pair_f.ensure(pairing_f12_bytes((int)Gt)) == KZG355_OK) f12 = w->pair_f.as<Fp>();
            hipStream_t st = w->stream;
            w->in_flight = true;                                  // (no error words in this stage -- the blocks' are in st1 -- so of the frame only the wait)
            Timed tm(s, w);
            for (size_t k = 0; k < Gt; k++)
                for (size_t d = 0; d < D; d++) {
                    G1Jac *dst = gath.as<G1Jac>() + 3 * (k * D + d);
                    const G1Jac *src = gs[d]->w->lc_partials.as<G1Jac>() + 3 * (t + k * D);
                    if (gs[d]->s->device == s->device) HIPCHK(hipMemcpyAsync(dst, src, sizeof(G1Jac) * 3, hipMemcpyDeviceToDevice, st));
                    else HIPCHK(hipMemcpyPeerAsync(dst, s->device, src, gs[d]->s->device, sizeof(G1Jac) * 3, st));
                }
            uint8_t *d_r = w->out48.as<uint8_t>(), *d_dbg = dbg ? d_r + 32 * groups : nullptr;
            tm.begin("cell_merge");
            if (!launch_cell_merge(gath.as<G1Jac>(), (int)D, (int)Gt, d_r, (int)t, (int)D, w->pair_pts.as<PairPt>(), d_dbg, st)) return KZG355_INTERNAL;
            tm.end();
            tm.begin("cell_pairing");
            launch_pairing(w->pair_pts.as<PairPt>(), s->cell_t, (int)Gt, w->ok.as<int>(), st, s->pairing_two_wave_upto, f12, s->pairing_hard12_from,
                           s->miller_segments);
            tm.end();
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(w->h_ok.p, w->ok.p, sizeof(int) * Gt, hipMemcpyDeviceToHost, st));
            if (dbg) HIPCHK(hipMemcpyAsync(w->h_out.p, d_dbg, (size_t)CELL_DEBUG_BYTES * Gt, hipMemcpyDeviceToHost, st));
            if ((rc = launch_set_wait(w, tm))) return rc;
            for (size_t k = 0; k < Gt; k++) {
                const size_t g = t + k * D;
                if (dbg) memcpy(dbg + (size_t)CELL_DEBUG_BYTES * g, w->h_out.as<uint8_t>() + (size_t)CELL_DEBUG_BYTES * k, CELL_DEBUG_BYTES);
                ok[g] = w->h_ok.as<int>()[k] != 0;
            }
            return KZG355_OK;
        });
        if (rc2 != KZG355_OK) return refuse(rc2);
    }
    // an Err in any block is the group's Err: the first one in block order
    int first = KZG355_OK;
    for (size_t g = 0; g < groups; g++) {
        int stt = KZG355_OK;
        for (size_t d = 0; d < D && stt == KZG355_OK; d++) stt = st1[d][g];
        if (status) status[g] = stt;
        if (stt != KZG355_OK) ok[g] = false;
        if (stt != KZG355_OK && first == KZG355_OK) first = stt;
    }
    return first;
}

// Cells per device from which a call with fewer groups than devices cuts its groups over the devices: the blob path's rule (multi_verify_many),
// so that one rule describes the handle.  No measurement on several cards stands behind the figure.
static const size_t CELL_SHARD_MIN_CELLS_PER_DEVICE = 2;
static_assert(MAX_HANDLE_DEVICES <= (size_t)CELL_MERGE_MAX_BLOCKS, "k_cell_merge adds one block per lane of one wave");

// The host-buffer calls on a handle over several devices: enough independent groups (or groups too small to cut) go to the replicas in
// contiguous ranges, each on its replica's own host thread and workspace, with no exchange; fewer groups than devices are cut into blocks.
static int cell_multi(bool *ok, int *status, uint8_t *dbg, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                      size_t npg, size_t groups, const kzg355_settings *cs) {
    MultiDev *m = cs->multi;
    const size_t D = m->rep.size();
    const bool force_sharded = cs->force_sharded && npg >= D;         // (test hook: kzg355_options.force_sharded)
    if (!force_sharded && (groups >= D || npg < CELL_SHARD_MIN_CELLS_PER_DEVICE * D)) {
        // as many replicas as there are groups; each range's WsGuard scopes its device on the range's own thread
        return fan_out(cs, groups < D ? groups : D, groups, [&](const kzg355_settings *rep, size_t g0, size_t n) -> int {
            const size_t c0 = g0 * npg;
            return cell_single(ok + g0, status ? status + g0 : nullptr, dbg ? dbg + (size_t)CELL_DEBUG_BYTES * g0 : nullptr, commitments + 48 * c0,
                               cell_indices + c0, cells + (size_t)CELL_BYTES * c0, proofs + 48 * c0, npg, n, rep, false, 0);
        });
    }
    return cell_multi_sharded(ok, status, dbg, commitments, cell_indices, cells, proofs, npg, groups, cs);
}

// What is decided once for the whole call, whatever runs it afterwards
static int cell_impl(bool *ok, int *status, uint8_t *dbg, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                     size_t npg, size_t groups, const kzg355_settings *cs, bool device = false, int prep_form = 0) {
    if (!cs || !ok) return KZG355_BADARGS;
    if (groups == 0) return KZG355_OK;
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    if (device && (prep_form < 0 || prep_form > 2)) return refuse(KZG355_BADARGS);
    if (npg == 0) {                                               // verify_cell_kzg_proof_batch of no cells: true
        for (size_t i = 0; i < groups; i++) { ok[i] = true; if (status) status[i] = KZG355_OK; }
        if (dbg) memset(dbg, 0, (size_t)CELL_DEBUG_BYTES * groups);
        return KZG355_OK;
    }
    if (!commitments || !cell_indices || !cells || !proofs) return refuse(KZG355_BADARGS);
    if (device && (((uintptr_t)commitments & 15) || ((uintptr_t)cells & 15) || ((uintptr_t)proofs & 15) || ((uintptr_t)cell_indices & 7)))
        return refuse(KZG355_BADARGS);
    if (out_of_range(npg, groups, CELL_MAX_CELLS)) return refuse(KZG355_BADARGS);
    if (is_small(cs)) return refuse(KZG355_BADARGS);             // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    // device-resident arrays live on the handle's first device and stay there
    if (cs->multi && !device) return cell_multi(ok, status, dbg, commitments, cell_indices, cells, proofs, npg, groups, cs);
    return cell_single(ok, status, dbg, commitments, cell_indices, cells, proofs, npg, groups, cs, device, prep_form);
}

// Groups of different sizes (the `_sets` entry points): group g is entries [off_g, off_g + counts[g]) of the four host arrays, off_g the sum of the
// counts before it.  Everything that refuses the whole call is decided from the counts alone, before an array is read or a device touched.  An
// empty group is true / OK on the spot and takes no part in the launch set: the rest are numbered anew, so that the offsets the kernels search
// are strictly increasing, and their results go back to their places.  The arrays need no packing for that -- an empty group has no entries.
// device: the four arrays are device memory on the handle's first device (16- / 8-byte aligned, or the call is refused) and the counts stay host
// memory: one launch set there for all non-empty groups, prep_form as cell_single takes it.
static const size_t CELL_SETS_MAX_GROUPS = (size_t)1 << 24;
static int cell_sets_impl(bool *ok, int *status, uint8_t *dbg, const size_t *counts, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells,
                          const uint8_t *proofs, size_t groups, const kzg355_settings *cs, bool device = false, int prep_form = 0) {
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    if (!cs || !ok || (groups > 0 && !counts)) return refuse(KZG355_BADARGS);
    if (groups == 0) return KZG355_OK;
    if (groups > CELL_SETS_MAX_GROUPS) return refuse(KZG355_BADARGS);
    if (prep_form < 0 || prep_form > 2) return refuse(KZG355_BADARGS);
    size_t total = 0, live = 0;
    for (size_t g = 0; g < groups; g++) {
        if (counts[g] > CELL_MAX_CELLS - total) return refuse(KZG355_BADARGS);       // (so the sum cannot overflow either)
        total += counts[g];
        live += counts[g] != 0;
    }
    if (total > 0 && (!commitments || !cell_indices || !cells || !proofs)) return refuse(KZG355_BADARGS);
    if (device && total > 0 && (((uintptr_t)commitments & 15) || ((uintptr_t)cells & 15) || ((uintptr_t)proofs & 15) || ((uintptr_t)cell_indices & 7)))
        return refuse(KZG355_BADARGS);
    if (is_small(cs)) return refuse(KZG355_BADARGS);             // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    // the non-empty groups: where each came from, and the cells before each
    std::vector<size_t> from(live), goff(live + 1, 0);
    for (size_t g = 0, l = 0; g < groups; g++) {
        if (counts[g] == 0) {                                     // verify_cell_kzg_proof_batch of no cells: true
            ok[g] = true;
            if (status) status[g] = KZG355_OK;
            if (dbg) memset(dbg + (size_t)CELL_DEBUG_BYTES * g, 0, CELL_DEBUG_BYTES);
            continue;
        }
        from[l] = g;
        goff[l + 1] = goff[l] + counts[g];
        l++;
    }
    if (live == 0) return KZG355_OK;
    // results of the launch set(s) in the order of the non-empty groups (std::vector<bool> has no bool array to hand out)
    std::unique_ptr<bool[]> l_ok(new bool[live]());
    std::vector<int> l_st(live, KZG355_OK);
    std::vector<uint8_t> l_dbg(dbg ? (size_t)CELL_DEBUG_BYTES * live : 0);
    auto run = [&](const kzg355_settings *on, size_t l0, size_t k) -> int {
        // groups l0 .. l0 + k - 1: their arrays start at goff[l0], their offsets count from there
        const size_t c0 = goff[l0];
        std::vector<size_t> sub(k + 1);
        for (size_t i = 0; i <= k; i++) sub[i] = goff[l0 + i] - c0;
        const int rc = cell_single(l_ok.get() + l0, l_st.data() + l0, dbg ? l_dbg.data() + (size_t)CELL_DEBUG_BYTES * l0 : nullptr, commitments + 48 * c0,
                                   cell_indices + c0, cells + (size_t)CELL_BYTES * c0, proofs + 48 * c0, 0, k, on, device, prep_form, sub.data());
        return call_failed(rc) ? refuse_call(l_st.data() + l0, k, rc, l_ok.get() + l0) : rc;      // (a failure of the range is every group's of the range)
    };
    // A handle over several devices: contiguous ranges of the non-empty groups, one launch set per replica that gets any.  A group is never cut
    // (and force_sharded does not apply); ranges equal in groups can be uneven in cells.  Device-resident arrays live on the handle's first
    // device and stay there.
    int rc;
    if (cs->multi && !device) {
        const size_t D = cs->multi->rep.size();
        rc = fan_out(cs, live < D ? live : D, live, run);
    } else {
        rc = run(cs, 0, live);
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

int kzg355_verify_cell_kzg_proof_batch_many(bool *ok, int *status, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells,
                                            const uint8_t *proofs, size_t n_per_group, size_t groups, const kzg355_settings *s) {
    return cell_impl(ok, status, nullptr, commitments, cell_indices, cells, proofs, n_per_group, groups, s);
}

int kzg355_verify_cell_kzg_proof_batch(bool *ok, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                                       size_t n, const kzg355_settings *s) {
    if (!s || !ok) return KZG355_BADARGS;
    bool r = false; int st = KZG355_OK;
    const int rc = cell_impl(&r, &st, nullptr, commitments, cell_indices, cells, proofs, n, 1, s);
    if (rc == KZG355_OK) *ok = r;
    return rc;
}

int kzg355_debug_cell_batch_intermediates(uint8_t *out, bool *ok, int *status, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells,
                                          const uint8_t *proofs, size_t n_per_group, size_t groups, const kzg355_settings *s) {
    if (!out) return KZG355_BADARGS;
    return cell_impl(ok, status, out, commitments, cell_indices, cells, proofs, n_per_group, groups, s);
}

int kzg355_verify_cell_kzg_proof_batch_many_sets(bool *ok, int *status, const size_t *cell_counts, const uint8_t *commitments, const size_t *cell_indices,
                                                 const uint8_t *cells, const uint8_t *proofs, size_t groups, const kzg355_settings *s) {
    return cell_sets_impl(ok, status, nullptr, cell_counts, commitments, cell_indices, cells, proofs, groups, s);
}

int kzg355_debug_cell_batch_intermediates_sets(uint8_t *out, bool *ok, int *status, const size_t *cell_counts, const uint8_t *commitments,
                                               const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs, size_t groups,
                                               const kzg355_settings *s) {
    if (!out) return refuse_call(status, groups, KZG355_BADARGS, ok);
    return cell_sets_impl(ok, status, out, cell_counts, commitments, cell_indices, cells, proofs, groups, s);
}

int kzg355_verify_cell_kzg_proof_batch_many_sets_device(bool *ok, int *status, const size_t *cell_counts, const uint8_t *d_commitments,
                                                        const size_t *d_cell_indices, const uint8_t *d_cells, const uint8_t *d_proofs, size_t groups,
                                                        const kzg355_settings *s) {
    return cell_sets_impl(ok, status, nullptr, cell_counts, d_commitments, d_cell_indices, d_cells, d_proofs, groups, s, true, 0);
}

int kzg355_debug_cell_batch_intermediates_sets_device(uint8_t *out, bool *ok, int *status, const size_t *cell_counts, const uint8_t *d_commitments,
                                                      const size_t *d_cell_indices, const uint8_t *d_cells, const uint8_t *d_proofs, size_t groups,
                                                      int prep_form, const kzg355_settings *s) {
    if (!out) return refuse_call(status, groups, KZG355_BADARGS, ok);
    return cell_sets_impl(ok, status, out, cell_counts, d_commitments, d_cell_indices, d_cells, d_proofs, groups, s, true, prep_form);
}

int kzg355_verify_cell_kzg_proof_batch_many_device(bool *ok, int *status, const uint8_t *d_commitments, const size_t *d_cell_indices, const uint8_t *d_cells,
                                                   const uint8_t *d_proofs, size_t n_per_group, size_t groups, const kzg355_settings *s) {
    return cell_impl(ok, status, nullptr, d_commitments, d_cell_indices, d_cells, d_proofs, n_per_group, groups, s, true, 0);
}

int kzg355_debug_cell_batch_intermediates_device(uint8_t *out, bool *ok, int *status, const uint8_t *d_commitments, const size_t *d_cell_indices,
                                                 const uint8_t *d_cells, const uint8_t *d_proofs, size_t n_per_group, size_t groups, int prep_form,
                                                 const kzg355_settings *s) {
    if (!out) return KZG355_BADARGS;
    return cell_impl(ok, status, out, d_commitments, d_cell_indices, d_cells, d_proofs, n_per_group, groups, s, true, prep_form);
}

long kzg355_settings_cell_device_prep_calls(const kzg355_settings *s) { return s ? s->n_cell_device_prep.load() : 0L; }

int kzg355_settings_cell_calls_per_device(const kzg355_settings *s, long *out, size_t cap) {
    if (!s || (!out && cap > 0)) return KZG355_BADARGS;
    const std::vector<kzg355_settings *> rep = replicas_of(const_cast<kzg355_settings *>(s));
    for (size_t d = 0; d < rep.size() && d < cap; d++) out[d] = rep[d]->n_cell_sets.load();
    return (int)rep.size();
}

int kzg355_debug_cell_setup_monomial(uint8_t *out, const kzg355_settings *cs) {
    if (!cs || !out) return KZG355_BADARGS;
    if (is_small(cs)) return KZG355_BADARGS;
    WsGuard g(cs);
    if (!g.w) return KZG355_NO_DEVICE;
    int rc = ensure_cell_setup(g.s, g.w);
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, g.s->cell_mono48.p, 48 * CELL_FE, hipMemcpyDeviceToHost));
    return KZG355_OK;
}

#pragma GCC visibility pop
}  // extern "C"
