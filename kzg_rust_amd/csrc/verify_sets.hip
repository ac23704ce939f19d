// verify_sets.hip -- the C entry points of kzg355_verify_blob_kzg_proof_batch_many_sets (include/kzg355.h): verify_blob_kzg_proof_batch on batches
// of different blob counts in one call (host side of libkzg355.so; see engine.h).  Every batch keeps its own transcript, challenge r, pairing and
// verdict: per batch the answer is that of kzg355_verify_blob_kzg_proof_batch on its slice.  Stage 1 is per blob and runs as it always has, with
// one blob per "batch"; stage 2 runs on the `_sets` entries of its kernels (verify_sets_enqueue, verify_stages.hip).  Work and device memory
// follow the sum of the counts.
#include "engine.h"
#include <algorithm>

namespace kzg355_impl {

static const size_t BLOB_SETS_MAX_BLOBS = 32768;                  // blobs per launch set unless the handle was told otherwise

// `groups` non-empty batches on the device of cs (a replica, for a handle over several devices), batch g being blobs [boff[g], boff[g + 1]) of the
// three arrays (boff strictly increasing from 0): launch sets of whole batches, taken in order while the set's blobs stay within the handle's
// blob_sets_max_blobs (kzg355_settings_set_blob_sets_max_blobs; a larger batch is a set of its own).  The host form stages the blobs set by set
// and, like host_pipeline, never holds more than chunk_bytes of them per set nor more than chunks_in_flight sets on the device; the device
// form reads the caller's arrays in place.
static int sets_single(bool *ok, int *status, uint8_t *dump, const uint8_t *blobs, const uint8_t *commitments, const uint8_t *proofs, const size_t *boff,
                       size_t groups, const kzg355_settings *cs, bool device) {
    kzg355_settings *s = const_cast<kzg355_settings *>(cs);
    const size_t BB = blob_bytes_of(cs);
    size_t limit = s->blob_sets_max_blobs;
    if (!device) limit = std::min(limit, std::max<size_t>(1, s->chunk_bytes / BB));
    std::vector<size_t> cut{0};                                   // launch set k is batches cut[k] .. cut[k + 1] - 1
    for (size_t g0 = 0; g0 < groups;) {
        size_t g1 = g0 + 1;                                       // (one batch always goes)
        while (g1 < groups && boff[g1 + 1] - boff[g0] <= limit) g1++;
        cut.push_back(g1);
        g0 = g1;
    }
    const size_t nsets = cut.size() - 1;
    const size_t W = device ? 1 : std::min(nsets, (size_t)s->chunks_in_flight);
    InFlight in_flight;
    if (!device) in_flight.enter(s->calls_in_flight);
    GuardList guards;
    std::vector<Timed> tms;
    for (size_t i = 0; i < W; i++) {
        if (!guards.add(cs)) return KZG355_NO_DEVICE;
        tms.emplace_back(s, guards.back()->w);
    }
    std::vector<size_t> pend(W, nsets);                           // the set in flight on each workspace (nsets: none)
    int first = KZG355_OK;
    auto collect = [&](size_t slot) -> int {
        const size_t k = pend[slot];
        if (k == nsets) return KZG355_OK;
        pend[slot] = nsets;
        const size_t g0 = cut[k];
        const int rc = verify_sets_collect(guards[slot]->w, tms[slot], ok + g0, status ? status + g0 : nullptr, dump ? dump + 128 * g0 : nullptr,
                                           (int)(cut[k + 1] - g0));
        if (call_failed(rc)) return rc;
        if (rc != KZG355_OK && first == KZG355_OK) first = rc;
        return KZG355_OK;
    };
    std::vector<size_t> sub;
    for (size_t k = 0; k < nsets; k++) {
        const size_t slot = k % W, g0 = cut[k], G = cut[k + 1] - g0, b0 = boff[g0], nb = boff[cut[k + 1]] - b0;
        Workspace *w = guards[slot]->w;
        int rc;
        if ((rc = collect(slot))) return rc;                      // frees this slot's device buffers
        sub.resize(G + 1);
        for (size_t i = 0; i <= G; i++) sub[i] = boff[g0 + i] - b0;
        s->n_blob_sets_blobs.fetch_add((long)nb);
        const uint8_t *hb = blobs + BB * b0, *hc = commitments + 48 * b0, *hp = proofs + 48 * b0;
        HostFront hf;
        HostFront *hfp = nullptr;
        if (device) {
            hfp = nsets == 1 ? resident_front(s, hf, hc, nb, &in_flight) : nullptr;
        } else {
            // a call of one small set: the host threads hash the challenges while the copies and the point kernels are queued, and the blobs go up
            // inside the enqueue, behind the point kernels (host_pipeline's route for such a call)
            if (nsets == 1 && host_call_hashes_on_host(s, nb)) {
                if ((rc = w->h_digests.ensure(32 * nb)) || (rc = w->digests.ensure(32 * nb)) || (rc = w->blobs.ensure(BB * nb))) return rc;
                uint8_t *dig = w->h_digests.as<uint8_t>();
                const uint64_t n_fe = (uint64_t)s->t.n_fe; const int impl = s->sha_impl;
                auto job = [=](size_t j) { kzg_host::challenge_digests(dig + 64 * j, hb + BB * 2 * j, BB, hc + 96 * j, nb - 2 * j < 2 ? nb - 2 * j : 2, n_fe,
                        impl); };
                hf.job = s->host_pool->begin((nb + 1) / 2, job);
                hf.pool = s->host_pool; hf.h_blobs = hb; hf.bytes = BB * nb; hf.running = true;
                s->n_host_hashed++;
                hfp = &hf;
            } else if ((rc = stage_to_device(w, w->blobs, hb, BB * nb))) return rc;
            if ((rc = stage_to_device(w, w->commitments, hc, 48 * nb)) || (rc = stage_to_device(w, w->proofs, hp, 48 * nb))) return rc;
        }
        rc = verify_sets_enqueue(s, w, tms[slot], device ? hb : w->blobs.as<uint8_t>(), device ? hc : w->commitments.as<uint8_t>(),
                                 device ? hp : w->proofs.as<uint8_t>(), sub.data(), (int)G, hfp, nsets == 1, dump != nullptr);
        if (rc) return rc;                                        // (the guards wait for whatever is in flight)
        pend[slot] = k;
    }
    for (size_t j = 0; j < W; j++) {                              // the remaining sets, oldest first
        const int rc = collect((nsets + j) % W);
        if (rc) return rc;
    }
    return first;
}

// What is decided once for the whole call: everything that refuses it, from the counts alone, before an array is read or a device touched (the
// order of blob_sets_impl, blob_cells.hip).  An empty batch is true / OK on the spot (kzg.rs:653-655) and takes no part in a launch set: the rest
// are numbered anew, so that the offsets the kernels see are strictly increasing, and their results go back to their places.
static int sets_impl(bool *ok, int *status, uint8_t *dump, bool want_dump, const size_t *counts, const uint8_t *blobs, const uint8_t *commitments,
                     const uint8_t *proofs, size_t groups, const kzg355_settings *cs, bool device) {
    auto refuse = [&](int code) { return refuse_call(status, groups, code, ok); };
    if (!cs || !ok || (groups > 0 && !counts) || (want_dump && !dump)) return refuse(KZG355_BADARGS);
    if (groups == 0) return KZG355_OK;
    if (groups > MAX_BLOBS) return refuse(KZG355_BADARGS);
    size_t total = 0, live = 0;
    for (size_t g = 0; g < groups; g++) {
        if (counts[g] > MAX_BLOBS - total) return refuse(KZG355_BADARGS);       // the sum within MAX_BLOBS: it cannot wrap
        total += counts[g];
        live += counts[g] != 0;
    }
    if (total > 0 && (!blobs || !commitments || !proofs)) return refuse(KZG355_BADARGS);
    // 16-byte loads of the blobs (verify_many_device_impl)
    if (device && total > 0 && (((uintptr_t)blobs & 15) || ((uintptr_t)commitments & 3) || ((uintptr_t)proofs & 3))) return refuse(KZG355_BADARGS);
    // the non-empty batches: where each came from, and the blobs before each
    std::vector<size_t> from(live), boff(live + 1, 0);
    for (size_t g = 0, l = 0; g < groups; g++) {
        if (counts[g] == 0) {
            ok[g] = true;
            if (status) status[g] = KZG355_OK;
            if (dump) memset(dump + 128 * g, 0, 128);
            continue;
        }
        from[l] = g;
        boff[l + 1] = boff[l] + counts[g];
        l++;
    }
    if (live == 0) return KZG355_OK;
    // results in the order of the non-empty batches (std::vector<bool> has no bool array to hand out)
    std::unique_ptr<bool[]> l_ok(new bool[live]());
    std::vector<int> l_st(live, KZG355_OK);
    std::vector<uint8_t> l_dump(dump ? 128 * live : 0);
    const size_t BB = blob_bytes_of(cs);
    auto run = [&](const kzg355_settings *on, size_t l0, size_t k, bool dev) -> int {
        // batches l0 .. l0 + k - 1: their arrays start at blob boff[l0], their offsets count from there
        const size_t b0 = boff[l0];
        std::vector<size_t> sub(k + 1);
        for (size_t i = 0; i <= k; i++) sub[i] = boff[l0 + i] - b0;
        const int rc = sets_single(l_ok.get() + l0, l_st.data() + l0, dump ? l_dump.data() + 128 * l0 : nullptr, blobs + BB * b0, commitments + 48 * b0,
                                   proofs + 48 * b0, sub.data(), k, on, dev);
        return call_failed(rc) ? refuse_call(l_st.data() + l0, k, rc, l_ok.get() + l0) : rc;      // (a failure of the range is every batch's of the range)
    };
    // Device-resident arrays live on the handle's first device and stay there.  Host arrays on a handle over D devices: contiguous ranges of the
    // non-empty batches, balanced by BLOBS -- range d ends at the batch border nearest to d N / D on the prefix sums of the counts (the lower one
    // of two equally near).  A batch is never cut; a device whose two borders coincide gets nothing.
    int rc;
    if (cs->multi && !device && cs->multi->rep.size() > 1) {
        const size_t D = cs->multi->rep.size(), N = boff[live];
        std::vector<size_t> cut(D + 1, 0);
        cut[D] = live;
        for (size_t d = 1; d < D; d++) {
            // (products below 2^24 * 64: no overflow)
            const size_t hi = (size_t)(std::lower_bound(boff.begin(), boff.end(), (d * N + D - 1) / D) - boff.begin());      // first border at or above d N / D
            size_t best = hi;
            if (hi > 0 && d * N - boff[hi - 1] * D <= boff[hi] * D - d * N) best = hi - 1;
            cut[d] = std::max(best, cut[d - 1]);
        }
        rc = fan_out_cuts(cs, cut, [&](const kzg355_settings *rep, size_t l0, size_t k) -> int { return run(rep, l0, k, false); });
    } else {
        rc = run(cs, 0, live, device);
    }
    int first = KZG355_OK;
    for (size_t l = 0; l < live; l++) {
        const size_t g = from[l];
        ok[g] = l_ok[l];
        if (status) status[g] = l_st[l];
        if (dump) memcpy(dump + 128 * g, l_dump.data() + 128 * l, 128);
        if (l_st[l] != KZG355_OK && first == KZG355_OK) first = l_st[l];
    }
    return call_failed(rc) ? rc : first;
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_verify_blob_kzg_proof_batch_many_sets(bool *ok, int *status, const size_t *blob_counts, const uint8_t *blobs, const uint8_t *commitments,
                                                 const uint8_t *proofs, size_t groups, const kzg355_settings *s) {
    return sets_impl(ok, status, nullptr, false, blob_counts, blobs, commitments, proofs, groups, s, false);
}

int kzg355_verify_blob_kzg_proof_batch_many_sets_device(bool *ok, int *status, const size_t *blob_counts, const uint8_t *d_blobs,
                                                        const uint8_t *d_commitments, const uint8_t *d_proofs, size_t groups, const kzg355_settings *s) {
    return sets_impl(ok, status, nullptr, false, blob_counts, d_blobs, d_commitments, d_proofs, groups, s, true);
}

int kzg355_debug_batch_intermediates_sets(uint8_t *out, bool *ok, int *status, const size_t *blob_counts, const uint8_t *blobs, const uint8_t *commitments,
                                          const uint8_t *proofs, size_t groups, const kzg355_settings *s) {
    return sets_impl(ok, status, out, true, blob_counts, blobs, commitments, proofs, groups, s, false);
}

int kzg355_debug_batch_intermediates_sets_device(uint8_t *out, bool *ok, int *status, const size_t *blob_counts, const uint8_t *d_blobs,
                                                 const uint8_t *d_commitments, const uint8_t *d_proofs, size_t groups, const kzg355_settings *s) {
    return sets_impl(ok, status, out, true, blob_counts, d_blobs, d_commitments, d_proofs, groups, s, true);
}

int kzg355_settings_set_blob_sets_max_blobs(kzg355_settings *s, size_t max_blobs) {
    if (!s || max_blobs > MAX_BLOBS) return KZG355_BADARGS;
    for (kzg355_settings *rep : replicas_of(s)) rep->blob_sets_max_blobs = max_blobs ? max_blobs : BLOB_SETS_MAX_BLOBS;
    return KZG355_OK;
}

int kzg355_settings_blob_sets_blobs_per_device(const kzg355_settings *s, long *out, size_t cap) {
    if (!s || (!out && cap > 0)) return KZG355_BADARGS;
    const std::vector<kzg355_settings *> rep = replicas_of(const_cast<kzg355_settings *>(s));
    for (size_t d = 0; d < rep.size() && d < cap; d++) out[d] = rep[d]->n_blob_sets_blobs.load();
    return (int)rep.size();
}

#pragma GCC visibility pop
}  // extern "C"
