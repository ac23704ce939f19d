// cells.hip -- the C entry points of verify_cell_kzg_proof_batch (EIP-7594 cells; include/kzg355.h) and the per-handle setup they need (host side
// of libkzg355.so; see engine.h).  The host deduplicates the commitments, sorts every group's cells by column and hashes its transcript (one group
// per host-pool task); the kernels of k_cells.hip and the shared point / pairing kernels do the rest in one set of launches for all groups.
#include "engine.h"

#include <string_view>
#include <unordered_map>

namespace kzg355_impl {

static const char *const CELL_DOMAIN = "RCKZGCBATCH__V1_";
static const size_t CELL_MAX_CELLS = (size_t)1 << 18;   // cells per call (512 MiB of cells)

static void put_u64be(uint8_t *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (56 - 8 * i)); }

// The first cell call of a handle: constants, the 64 monomial points [tau^t]_1 (build_monomial_points, cell_compute.hip) and the line table of
// [tau^64]_2.  Under cell_mu.  A failure releases what was being filled and is not remembered: the next call tries again (engine.h, at cell_mu).
static int ensure_cell_setup(kzg355_settings *s, Workspace *w) {
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
// the four arrays in host memory (the caller's, or a device-resident call's copied back) -> hp; one group per host-pool task
static void cell_host_prep(kzg355_settings *s, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs, size_t npg,
                           size_t groups, CellHostPrep &hp) {
    const int n = (int)npg, G = (int)groups;
    const size_t N = npg * groups;
    const int seg_cap = n < CELLS_PER_EXT_BLOB ? n : CELLS_PER_EXT_BLOB;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> &h_uc = hp.uc, &h_dig = hp.dig;
    h_uc.resize(48 * N); h_dig.resize(32 * groups);
    std::vector<int> h_cell(N), h_cidx(N), h_perm(N);
    std::vector<int4> h_seg_local((size_t)G * seg_cap);
    std::vector<CellHostGroup> &hg = hp.hg;
    hg.assign(groups, CellHostGroup());
    auto prep = [&](size_t gi) {
        const size_t base = gi * npg;
        CellHostGroup &gr = hg[gi];
        for (size_t k = 0; k < npg; k++) {
            const size_t c = cell_indices[base + k];
            if (c >= (size_t)CELLS_PER_EXT_BLOB) gr.bad_index = true;
            h_cell[base + k] = c < (size_t)CELLS_PER_EXT_BLOB ? (int)c : 0;
        }
        std::unordered_map<std::string_view, int> seen;
        seen.reserve(npg * 2);
        int u = 0;
        uint8_t *uc = h_uc.data() + 48 * base;
        for (size_t k = 0; k < npg; k++) {
            const std::string_view key(reinterpret_cast<const char *>(commitments + 48 * (base + k)), 48);
            auto it = seen.find(key);
            int pos;
            if (it == seen.end()) {
                pos = u++;
                memcpy(uc + 48 * pos, key.data(), 48);
                seen.emplace(key, pos);                             // (the key views caller memory, which outlives the map)
            } else {
                pos = it->second;
            }
            h_cidx[base + k] = pos;
        }
        for (int i = u; i < n; i++) { memset(uc + 48 * i, 0, 48); uc[48 * i] = 0xc0; }      // infinity, weight 0
        // counting sort by column
        int cnt[CELLS_PER_EXT_BLOB] = {0}, at[CELLS_PER_EXT_BLOB];
        for (size_t k = 0; k < npg; k++) cnt[h_cell[base + k]]++;
        int acc = 0;
        for (int c = 0; c < CELLS_PER_EXT_BLOB; c++) {
            at[c] = acc;
            if (cnt[c]) h_seg_local[gi * seg_cap + gr.n_segs++] = make_int4((int)gi, c, (int)base + acc, cnt[c]);
            acc += cnt[c];
        }
        for (size_t k = 0; k < npg; k++) h_perm[base + at[h_cell[base + k]]++] = (int)(base + k);
        // transcript
        const size_t len = 16 + 32 + 48 * (size_t)u + npg * (16 + CELL_BYTES + 48);
        std::vector<uint8_t> msg(len);
        uint8_t *p = msg.data();
        memcpy(p, CELL_DOMAIN, 16); p += 16;
        put_u64be(p, N_FE); put_u64be(p + 8, CELL_FE); put_u64be(p + 16, (uint64_t)u); put_u64be(p + 24, npg); p += 32;
        memcpy(p, uc, 48 * (size_t)u); p += 48 * (size_t)u;
        for (size_t k = 0; k < npg; k++) {
            put_u64be(p, (uint64_t)h_cidx[base + k]); put_u64be(p + 8, cell_indices[base + k]); p += 16;
            memcpy(p, cells + (size_t)CELL_BYTES * (base + k), CELL_BYTES); p += CELL_BYTES;
            memcpy(p, proofs + 48 * (base + k), 48); p += 48;
        }
        kzg_host::sha256(h_dig.data() + 32 * gi, msg.data(), len, s->sha_impl);
    };
    if (s->host_pool && groups > 1) s->host_pool->parallel_for(groups, prep);
    else for (size_t gi = 0; gi < groups; gi++) prep(gi);
    std::vector<int> h_gseg(groups + 1, 0);
    for (int gi = 0; gi < G; gi++) h_gseg[gi + 1] = h_gseg[gi] + hg[gi].n_segs;
    const int S = hp.S = h_gseg[G];
    std::vector<int> &meta = hp.meta;
    meta.resize((size_t)4 * S + (G + 1) + 3 * N);
    {
        int4 *sg = reinterpret_cast<int4 *>(meta.data());
        for (int gi = 0; gi < G; gi++) memcpy(sg + h_gseg[gi], h_seg_local.data() + (size_t)gi * seg_cap, sizeof(int4) * hg[gi].n_segs);
        int *q = meta.data() + 4 * (size_t)S;
        memcpy(q, h_gseg.data(), sizeof(int) * (G + 1)); q += G + 1;
        memcpy(q, h_cell.data(), sizeof(int) * N); q += N;
        memcpy(q, h_cidx.data(), sizeof(int) * N); q += N;
        memcpy(q, h_perm.data(), sizeof(int) * N);
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
static bool cell_device_call_prepares_on_host(const kzg355_settings *s, size_t npg, size_t groups, int prep_form) {
    if (npg > (size_t)CELL_PREP_MAX_CELLS) return true;           // above the device preparation's cap every form takes the host's
    if (prep_form) return prep_form == 2;
    const size_t bytes = 16 + 32 + 48 + npg * (16 + CELL_BYTES + 48);          // (48 more per further unique commitment)
    return bytes > CELL_PREP_HOST_FROM_BYTES && groups < (size_t)CELL_PREP_HOST_UPTO_GROUPS_PER_CU * (size_t)s->cu_count;
}

// device = false: the four arrays are host memory (the launch sequence of the host-buffer calls).  device = true: they are device memory on the
// handle's device; prep_form 0 by size, 1 device preparation, 2 copy back and prepare on the host.
static int cell_impl(bool *ok, int *status, uint8_t *dbg, const uint8_t *commitments, const size_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                     size_t npg, size_t groups, const kzg355_settings *cs, bool device = false, int prep_form = 0) {
    if (!cs || !ok) return KZG355_BADARGS;
    if (groups == 0) return KZG355_OK;
    auto refuse = [&](int code) { for (size_t i = 0; i < groups; i++) { ok[i] = false; if (status) status[i] = code; } return code; };
    if (device && (prep_form < 0 || prep_form > 2)) return refuse(KZG355_BADARGS);
    if (npg == 0) {                                               // verify_cell_kzg_proof_batch of no cells: true
        for (size_t i = 0; i < groups; i++) { ok[i] = true; if (status) status[i] = KZG355_OK; }
        if (dbg) memset(dbg, 0, (size_t)CELL_DEBUG_BYTES * groups);
        return KZG355_OK;
    }
    if (!commitments || !cell_indices || !cells || !proofs) return refuse(KZG355_BADARGS);
    if (device && (((uintptr_t)commitments & 15) || ((uintptr_t)cells & 15) || ((uintptr_t)proofs & 15) || ((uintptr_t)cell_indices & 7)))
        return refuse(KZG355_BADARGS);
    if (npg > CELL_MAX_CELLS || groups > CELL_MAX_CELLS || npg * groups > CELL_MAX_CELLS) return refuse(KZG355_BADARGS);
    if (is_small(cs)) return refuse(KZG355_BADARGS);             // the cell layout is defined for FIELD_ELEMENTS_PER_BLOB = 4096 only
    WsGuard g(cs);
    if (!g.w) return refuse(KZG355_NO_DEVICE);
    kzg355_settings *s = g.s; Workspace *w = g.w;
    int rc;
    if ((rc = ensure_cell_setup(s, w))) return refuse(rc);
    const int n = (int)npg, G = (int)groups, T = cell_terms(n);
    const size_t N = npg * groups;
    const int seg_cap = n < CELLS_PER_EXT_BLOB ? n : CELLS_PER_EXT_BLOB;
    hipStream_t st = w->stream;

    // ---- prepare: dedup, column sort, transcripts -- by the host from the caller's arrays, by the host from a copy of them, or on the device
    const bool dev_prep = device && !cell_device_call_prepares_on_host(s, npg, groups, prep_form);
    CellHostPrep hp;
    if (!device) {
        cell_host_prep(s, commitments, cell_indices, cells, proofs, npg, groups, hp);
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
        cell_host_prep(s, b_c, b_idx, b_cells, b_p, npg, groups, hp);
    }
    // meta buffer of the device preparation: the host's layout with a fixed seg_cap segments per group, then the unique-commitment counts and
    // (tables too large for LDS) the dedup tables
    const int tab_size = dev_prep ? cell_prep_table_slots(n) : 0;
    const size_t gtab_ints = tab_size > CELL_PREP_LDS_SLOTS ? (size_t)tab_size * groups : 0;
    const int S = dev_prep ? G * seg_cap : hp.S;
    const size_t meta_ints = dev_prep ? (size_t)4 * S + (G + 1) + 3 * N + groups + gtab_ints : hp.meta.size();

    // ---- device.  (The workspace's buffers by role: blobs = cells, commitments = unique commitments, q = meta, z = r powers, y = column
    // coefficients, scal_a = lincomb scalars, partials = lincomb terms, lc_partials = the three sums per group, out48 = r | debug output.)
    if ((!device && ((rc = w->blobs.ensure((size_t)CELL_BYTES * N)) || (rc = w->proofs.ensure(48 * N)))) || (rc = w->commitments.ensure(48 * N)) ||
        (rc = w->pts.ensure(sizeof(G1Affine) * 2 * N)) || (rc = w->digests.ensure(32 * groups)) || (rc = w->q.ensure(sizeof(int) * meta_ints)) ||
        (rc = w->z.ensure(sizeof(Fr) * N)) || (rc = w->y.ensure(sizeof(Fr) * CELL_FE * (size_t)(S > 0 ? S : 1))) ||
        (rc = w->scal_a.ensure(sizeof(uint32_t) * 8 * (size_t)T * groups)) || (rc = w->partials.ensure(sizeof(G1Jac) * (size_t)T * groups)) ||
        (rc = w->lc_partials.ensure(sizeof(G1Jac) * 3 * groups)) || (rc = w->pair_pts.ensure(sizeof(PairPt) * 2 * groups)) ||
        (rc = w->ok.ensure(sizeof(int) * groups)) || (rc = w->err.ensure(sizeof(int) * groups)) || (rc = w->h_ok.ensure(sizeof(int) * groups)) ||
        (rc = w->h_err.ensure(sizeof(int) * groups)) || (rc = w->out48.ensure((size_t)(32 + CELL_DEBUG_BYTES) * groups)) ||
        (rc = w->h_out.ensure((size_t)CELL_DEBUG_BYTES * groups)))
        return refuse(rc);
    Fp *f12 = nullptr;
    if (w->pair_f.ensure(pairing_f12_bytes(G)) == KZG355_OK) f12 = w->pair_f.as<Fp>();
    w->in_flight = true;
    Timed tm(s, w);
    const int4 *d_segs = w->q.as<int4>();
    const int *d_gseg = w->q.as<int>() + 4 * (size_t)S, *d_cell = d_gseg + G + 1, *d_cidx = d_cell + N, *d_perm = d_cidx + N;
    const uint8_t *d_cells = device ? cells : w->blobs.as<uint8_t>(), *d_proofs = device ? proofs : w->proofs.as<uint8_t>();
    uint8_t *d_r = w->out48.as<uint8_t>(), *d_dbg = dbg ? d_r + 32 * groups : nullptr;
    HIPCHK(hipMemsetAsync(w->err.p, 0, sizeof(int) * groups, st));
    if (dev_prep) {
        int *m = w->q.as<int>() + 4 * (size_t)S;
        int *d_ucount = m + (G + 1) + 3 * N, *d_gtab = gtab_ints ? d_ucount + groups : nullptr;
        tm.begin("cell_prep");
        launch_cell_prep(commitments, cell_indices, n, G, tab_size, d_gtab, w->commitments.as<uint8_t>(), w->q.as<int4>(), m, m + (G + 1), m + (G + 1) + N,
                         m + (G + 1) + 2 * N, d_ucount, w->err.as<int>(), st);
        tm.end();
        tm.begin("cell_rhash");
        launch_cell_rhash(w->commitments.as<uint8_t>(), cell_indices, cells, proofs, d_cidx, d_ucount, n, G, G >= s->rhash_lanes_from, w->digests.as<uint8_t>(),
                          st);
        tm.end();
        s->n_cell_device_prep.fetch_add(1);
    } else {
        HIPCHK(hipMemcpyAsync(w->commitments.p, hp.uc.data(), 48 * N, hipMemcpyHostToDevice, st));
        if (!device) HIPCHK(hipMemcpyAsync(w->proofs.p, proofs, 48 * N, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(w->q.p, hp.meta.data(), sizeof(int) * hp.meta.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(w->digests.p, hp.dig.data(), 32 * groups, hipMemcpyHostToDevice, st));
        if (!device) HIPCHK(hipMemcpyAsync(w->blobs.p, cells, (size_t)CELL_BYTES * N, hipMemcpyHostToDevice, st));
    }
    tm.begin("cell_points");
    launch_decompress_points(w->commitments.as<uint8_t>(), d_proofs, (int)N, n, w->pts.as<G1Affine>(), w->err.as<int>(), st);
    launch_subgroup_points(w->pts.as<G1Affine>(), (int)N, n, w->err.as<int>(), st);
    tm.end();
    tm.begin("cell_scalars");
    launch_cell_scalars(w->digests.as<uint8_t>(), d_cell, d_cidx, n, G, s->cell_consts.as<CellConsts>(), w->z.as<Fr>(), w->scal_a.as<uint32_t>(), d_r, st);
    tm.end();
    tm.begin("cell_interp");
    launch_cell_interp(d_cells, d_perm, d_segs, S, d_gseg, w->z.as<Fr>(), s->cell_consts.as<CellConsts>(), n, G, w->y.as<Fr>(),
                       w->scal_a.as<uint32_t>(), w->err.as<int>(), st);
    tm.end();
    tm.begin("cell_lincomb");
    launch_cell_lincomb(w->pts.as<G1Affine>(), s->cell_mono.as<G1Affine>(), w->scal_a.as<uint32_t>(), n, G, w->partials.as<G1Jac>(), w->lc_partials.as<G1Jac>(),
                        d_r, w->pair_pts.as<PairPt>(), d_dbg, st);
    tm.end();
    tm.begin("cell_pairing");
    launch_pairing(w->pair_pts.as<PairPt>(), s->cell_t, G, w->ok.as<int>(), st, s->pairing_two_wave_upto, f12, s->pairing_hard12_from, s->miller_segments);
    tm.end();
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w->h_ok.p, w->ok.p, sizeof(int) * groups, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(w->h_err.p, w->err.p, sizeof(int) * groups, hipMemcpyDeviceToHost, st));
    if (dbg) HIPCHK(hipMemcpyAsync(w->h_out.p, d_dbg, (size_t)CELL_DEBUG_BYTES * groups, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    w->in_flight = false;
    tm.collect();
    if (dbg) memcpy(dbg, w->h_out.p, (size_t)CELL_DEBUG_BYTES * groups);
    int first = KZG355_OK;
    for (int i = 0; i < G; i++) {
        const int stt = !dev_prep && hp.hg[i].bad_index ? KZG355_BADARGS : status_from_err(w->h_err.as<int>()[i]);
        if (status) status[i] = stt;
        ok[i] = stt == KZG355_OK && w->h_ok.as<int>()[i] != 0;
        if (stt != KZG355_OK && first == KZG355_OK) first = stt;
    }
    return first;
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
