// point_eval.hip -- the EIP-4844 point-evaluation precompile (address 0x0A), batched: kzg355_point_evaluation_many and its device form, the one
// call as the EIP words it, and kzg_to_versioned_hash on host and device arrays (host side of libkzg355.so; see engine.h).
// Per launch set of at most 2^17 inputs: k_pe_unpack (k_point_eval.hip) hashes every commitment, compares the versioned hash and writes the
// 160-byte records; the records chain of kzg355_verify_kzg_proof_many (verify_records_impl: full validation, one record per batch) checks them;
// the host merges.  The precompile fails at the hash before it looks at anything else, so an input whose hash does not match reports nothing
// but that: false, KZG355_OK.  Such inputs still run through the chain with the others -- its answer for them is dropped in the merge.
#include "engine.h"
#include "point_eval.h"

namespace kzg355_impl {

static const size_t PE_SET = (size_t)1 << 17;      // inputs per launch set: the set size of verify_proofs_on_one_device

// n inputs on the one device of `cs` (a replica of a multi-device handle included); `inputs` is host memory, or with `device` set device memory
// on that device, which is only read.  The staging workspace lends its buffers and times pe_unpack; the chain runs on a second one.
static int point_eval_on_one_device(bool *ok, int *status, bool *hash_match, const uint8_t *inputs, bool device, size_t n, const kzg355_settings *cs) {
    WsGuard g(cs);
    if (!g.w) return KZG355_NO_DEVICE;
    kzg355_settings *s = g.s; Workspace *w = g.w;
    std::vector<int> own;                                         // the merge needs every status, whether the caller wants them or not
    if (!status) own.resize(n < PE_SET ? n : PE_SET);
    int first = KZG355_OK, rc;
    for (size_t lo = 0; lo < n; lo += PE_SET) {
        const size_t cnt = n - lo < PE_SET ? n - lo : PE_SET;
        if ((rc = w->records.ensure((size_t)RECORD_BYTES * cnt)) || (rc = w->small.ensure(sizeof(int) * cnt)) ||
                (rc = w->h_ok.ensure(sizeof(int) * cnt))) return rc;
        const uint8_t *d_in = inputs + (size_t)PE_INPUT_BYTES * lo;
        Timed tm(s, w);
        w->in_flight = true;                                      // (a failure below drains the stream: WsGuard)
        if (!device) {
            if ((rc = w->h_stage.ensure((size_t)PE_INPUT_BYTES * cnt)) || (rc = w->blobs.ensure((size_t)PE_INPUT_BYTES * cnt))) return rc;
            memcpy(w->h_stage.p, d_in, (size_t)PE_INPUT_BYTES * cnt);
            HIPCHK(hipMemcpyAsync(w->blobs.p, w->h_stage.p, (size_t)PE_INPUT_BYTES * cnt, hipMemcpyHostToDevice, w->stream));
            d_in = w->blobs.as<uint8_t>();
        }
        tm.begin("pe_unpack"); launch_pe_unpack(d_in, (int)cnt, w->records.as<uint8_t>(), w->small.as<int>(), w->stream); tm.end();
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(w->h_ok.p, w->small.p, sizeof(int) * cnt, hipMemcpyDeviceToHost, w->stream));
        if ((rc = launch_set_wait(w, tm))) return rc;
        int *st = status ? status + lo : own.data();
        rc = verify_records_impl(ok + lo, st, nullptr, w->records.as<uint8_t>(), 1, cnt, 1, cs);
        if (call_failed(rc)) return rc;
        const int *m = w->h_ok.as<int>();
        for (size_t i = 0; i < cnt; i++) {
            if (hash_match) hash_match[lo + i] = m[i] != 0;
            if (!m[i]) st[i] = KZG355_OK;
            if (!m[i] || st[i] != KZG355_OK) ok[lo + i] = false;      // (the chain leaves the verdict of a unit that is not OK unwritten)
            if (st[i] != KZG355_OK && first == KZG355_OK) first = st[i];
        }
    }
    return first;
}

// what both _many forms refuse as a whole, from the arguments alone: every status marked, every verdict and match false
static int point_eval_refuse(bool *ok, int *status, bool *hash_match, size_t n) {
    if (hash_match) for (size_t i = 0; i < n; i++) hash_match[i] = false;
    return refuse_call(status, n, KZG355_BADARGS, ok);
}

}  // namespace kzg355_impl

extern "C" {
#pragma GCC visibility push(default)

int kzg355_kzg_to_versioned_hash_many(uint8_t *out, const uint8_t *commitments, size_t n) {
    if (n == 0) return KZG355_OK;
    if (!out || !commitments || n > MAX_BLOBS) return KZG355_BADARGS;
    for (size_t i = 0; i < n; i++) {
        uint32_t c[PE_POINT_WORDS], vh[PE_HASH_WORDS];
        memcpy(c, commitments + 48 * i, 48);
        pe_versioned_hash(vh, c, PeHostCompress());
        memcpy(out + 32 * i, vh, 32);
    }
    return KZG355_OK;
}

int kzg355_kzg_to_versioned_hash_many_device(uint8_t *d_out, const uint8_t *d_commitments, size_t n, const kzg355_settings *cs) {
    if (n == 0) return KZG355_OK;
    if (!cs || !d_out || !d_commitments || n > MAX_BLOBS || ((uintptr_t)d_out & 15) || ((uintptr_t)d_commitments & 3)) return KZG355_BADARGS;
    WsGuard g(cs);
    if (!g.w) return KZG355_NO_DEVICE;
    Workspace *w = g.w;
    Timed tm(g.s, w);
    w->in_flight = true;
    tm.begin("versioned_hash"); launch_versioned_hash(d_commitments, (int)n, d_out, w->stream); tm.end();
    HIPCHK(hipGetLastError());
    return launch_set_wait(w, tm);
}

int kzg355_point_evaluation_many(bool *ok, int *status, bool *hash_match, const uint8_t *inputs, size_t n, const kzg355_settings *cs) {
    if (n == 0) return KZG355_OK;
    if (!cs || !ok || !inputs || n > MAX_BLOBS) return point_eval_refuse(ok, status, hash_match, n);
    // independent inputs: contiguous ranges per device, as kzg355_verify_kzg_proof_many cuts its checks
    if (cs->multi && cs->multi->rep.size() > 1 && n >= cs->multi->rep.size())
        return fan_out(cs, cs->multi->rep.size(), n, [&](const kzg355_settings *rep, size_t i0, size_t cnt) {
            return point_eval_on_one_device(ok + i0, status ? status + i0 : nullptr, hash_match ? hash_match + i0 : nullptr,
                    inputs + (size_t)PE_INPUT_BYTES * i0, false, cnt, rep);
        });
    return point_eval_on_one_device(ok, status, hash_match, inputs, false, n, cs);
}

int kzg355_point_evaluation_many_device(bool *ok, int *status, bool *hash_match, const uint8_t *d_inputs, size_t n, const kzg355_settings *cs) {
    if (n == 0) return KZG355_OK;
    if (!cs || !ok || !d_inputs || n > MAX_BLOBS || ((uintptr_t)d_inputs & 15)) return point_eval_refuse(ok, status, hash_match, n);
    return point_eval_on_one_device(ok, status, hash_match, d_inputs, true, n, cs);
}

int kzg355_point_evaluation(uint8_t out[64], const uint8_t *input, size_t input_len, const kzg355_settings *cs) {
    if (!cs || !out || !input || input_len != (size_t)PE_INPUT_BYTES) return KZG355_BADARGS;
    bool ok = false, match = false;
    int st = KZG355_OK;
    const int rc = kzg355_point_evaluation_many(&ok, &st, &match, input, 1, cs);
    if (rc != KZG355_OK) return rc;
    if (!match || !ok) return KZG355_BADARGS;
    // u256be(FIELD_ELEMENTS_PER_BLOB) | u256be(BLS_MODULUS)
    static const uint8_t BLS_MODULUS[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                            0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
    memset(out, 0, 24);
    put_u64be(out + 24, (uint64_t)cs->t.n_fe);
    memcpy(out + 32, BLS_MODULUS, 32);
    return KZG355_OK;
}

#pragma GCC visibility pop
}  // extern "C"
