// kzg355.hpp -- header-only C++ mirror of the reference's public surface over the C ABI (include/kzg355.h).
//
// The reference is compiled code (Rust): `pub struct Kzg` with eight associated functions plus the byte newtypes
// (pawanjay176/kzg_rust src/kzg.rs:10-22, 88-279, 983-1079).  This header restates that surface for C++ callers with
// the same names, argument meaning and error behaviour, so a test written against the reference reads the same here:
//
//     auto s = kzg355::Kzg::load_trusted_setup_file("trusted_setup.txt");          // Result<KzgSettings>
//     auto c = kzg355::Kzg::blob_to_kzg_commitment(blob, s.value());                // Result<KzgCommitment>
//     auto ok = kzg355::Kzg::verify_blob_kzg_proof_batch(blobs, commitments, proofs, s.value());   // Result<bool>
//
// `Result<T>` is Ok(T) or Err(Error) like Rust's; all arithmetic happens in libkzg355.so on the GPU (no CPU fallback).
#pragma once
#include <cstring>
#include <stdexcept>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "kzg355.h"

namespace kzg355 {

constexpr size_t BYTES_PER_FIELD_ELEMENT = KZG355_BYTES_PER_FIELD_ELEMENT;   // consts.rs:5
constexpr size_t BYTES_PER_COMMITMENT = KZG355_BYTES_PER_COMMITMENT;         // consts.rs:8
constexpr size_t BYTES_PER_PROOF = KZG355_BYTES_PER_PROOF;                   // consts.rs:11
constexpr size_t FIELD_ELEMENTS_PER_BLOB = KZG355_FIELD_ELEMENTS_PER_BLOB;   // consts.rs:13
constexpr size_t BYTES_PER_BLOB = KZG355_BYTES_PER_BLOB;                     // consts.rs:16

// enum Error (kzg.rs:10-22)
struct Error {
    enum Kind { BadArgs = 1, InternalError = 2, InvalidBytesLength = 3, InvalidHexFormat = 4, InvalidTrustedSetup = 5, NoDevice = 6, NoMemory = 7, DeviceError = 8 } kind;
    std::string message;
};

template <class T> class Result {
    bool ok_;
    T value_{};
    Error err_{Error::InternalError, ""};
public:
    Result(T v) : ok_(true), value_(std::move(v)) {}
    Result(Error e) : ok_(false), err_(std::move(e)) {}
    bool is_ok() const { return ok_; }
    bool is_err() const { return !ok_; }
    T &value() { return value_; }
    const T &value() const { return value_; }
    const Error &error() const { return err_; }
    T unwrap() && { if (!ok_) throw std::runtime_error("unwrap on Err: " + err_.message); return std::move(value_); }
};

inline Error from_status(int rc, const char *what) {
    Error::Kind k = (rc >= 1 && rc <= 8) ? (Error::Kind)rc : Error::InternalError;
    return Error{k, std::string(what) + ": status " + std::to_string(rc)};
}

// hex_to_bytes (kzg.rs:82-86): with or without the 0x prefix
inline Result<std::vector<uint8_t>> hex_to_bytes(const std::string &hex_str) {
    size_t off = hex_str.rfind("0x", 0) == 0 ? 2 : 0;
    size_t n = hex_str.size() - off;
    if (n % 2) return Error{Error::InvalidHexFormat, "Failed to decode hex: odd length"};
    std::vector<uint8_t> out(n / 2);
    auto val = [](char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; };
    for (size_t i = 0; i < n / 2; i++) {
        int hi = val(hex_str[off + 2 * i]), lo = val(hex_str[off + 2 * i + 1]);
        if (hi < 0 || lo < 0) return Error{Error::InvalidHexFormat, "Failed to decode hex: invalid character"};
        out[i] = (uint8_t)(hi * 16 + lo);
    }
    return out;
}

template <size_t N, Error::Kind LENGTH_ERROR> struct FixedBytes {
    std::vector<uint8_t> bytes = std::vector<uint8_t>(N);
    static Result<FixedBytes> from_bytes(const uint8_t *b, size_t len) {
        if (len != N) return Error{LENGTH_ERROR, "Invalid byte length. Expected " + std::to_string(N) + " got " + std::to_string(len)};
        FixedBytes r; std::memcpy(r.bytes.data(), b, N); return r;
    }
    static Result<FixedBytes> from_bytes(const std::vector<uint8_t> &b) { return from_bytes(b.data(), b.size()); }
    static Result<FixedBytes> from_hex(const std::string &h) {
        auto b = hex_to_bytes(h);
        if (b.is_err()) return b.error();
        return from_bytes(b.value());
    }
    const uint8_t *data() const { return bytes.data(); }
    bool operator==(const FixedBytes &o) const { return bytes == o.bytes; }
};
using Bytes32 = FixedBytes<32, Error::BadArgs>;                         // kzg.rs:101-122 (length error is BadArgs)
using Bytes48 = FixedBytes<48, Error::InvalidBytesLength>;              // kzg.rs:124-152
using Blob = FixedBytes<BYTES_PER_BLOB, Error::InvalidBytesLength>;     // kzg.rs:154-178
using KzgCommitment = Bytes48;                                          // kzg.rs:180-191
using KzgProof = Bytes48;                                               // kzg.rs:193-204
using Cell = FixedBytes<KZG355_BYTES_PER_CELL, Error::InvalidBytesLength>;   // EIP-7594 cell: 64 field elements

// KzgSettings (kzg.rs:28-40): opaque device-resident handle, Drop frees it, shareable between threads
class KzgSettings {
    std::shared_ptr<kzg355_settings> h_;
public:
    KzgSettings() = default;
    explicit KzgSettings(kzg355_settings *raw) : h_(raw, [](kzg355_settings *p) { kzg355_free_trusted_setup(p); }) {}
    const kzg355_settings *raw() const { return h_.get(); }
    // KzgSettings::load_trusted_setup (kzg.rs:45-78)
    static Result<KzgSettings> load_trusted_setup(const std::vector<std::vector<uint8_t>> &g1, const std::vector<std::vector<uint8_t>> &g2) {
        std::vector<uint8_t> a, b;
        for (auto &x : g1) { if (x.size() != 48) return Error{Error::InvalidBytesLength, "g1 point length"}; a.insert(a.end(), x.begin(), x.end()); }
        for (auto &x : g2) { if (x.size() != 96) return Error{Error::InvalidBytesLength, "g2 point length"}; b.insert(b.end(), x.begin(), x.end()); }
        kzg355_settings *raw = nullptr;
        int rc = kzg355_load_trusted_setup(a.data(), g1.size(), b.data(), g2.size(), &raw);
        if (rc) return from_status(rc, "load_trusted_setup");
        return KzgSettings(raw);
    }
    // one count per device of the handle: the cell launch sets (verify, compute, recover) that device has run so far; empty without a handle
    std::vector<long> cell_calls_per_device() const {
        if (!h_) return {};
        std::vector<long> out((size_t)kzg355_settings_cell_calls_per_device(h_.get(), nullptr, 0));
        kzg355_settings_cell_calls_per_device(h_.get(), out.data(), out.size());
        return out;
    }
};

// pub struct Kzg (kzg.rs:983-1079)
struct Kzg {
    static Result<KzgSettings> load_trusted_setup_file(const std::string &path) {                         // kzg.rs:995
        kzg355_settings *raw = nullptr;
        int rc = kzg355_load_trusted_setup_file(path.c_str(), &raw);
        if (rc) return from_status(rc, "load_trusted_setup_file");
        return KzgSettings(raw);
    }
    static Result<KzgSettings> load_trusted_setup(const std::vector<std::vector<uint8_t>> &g1, const std::vector<std::vector<uint8_t>> &g2) {
        return KzgSettings::load_trusted_setup(g1, g2);                                                   // kzg.rs:1005
    }
    static Result<KzgCommitment> blob_to_kzg_commitment(const Blob &blob, const KzgSettings &s) {         // kzg.rs:1013
        KzgCommitment out;
        int rc = kzg355_blob_to_kzg_commitment(out.bytes.data(), blob.data(), s.raw());
        if (rc) return from_status(rc, "blob_to_kzg_commitment");
        return out;
    }
    static Result<std::pair<KzgProof, Bytes32>> compute_kzg_proof(const Blob &blob, const Bytes32 &z, const KzgSettings &s) {   // kzg.rs:1021
        KzgProof p; Bytes32 y;
        int rc = kzg355_compute_kzg_proof(p.bytes.data(), y.bytes.data(), blob.data(), z.data(), s.raw());
        if (rc) return from_status(rc, "compute_kzg_proof");
        return std::make_pair(p, y);
    }
    static Result<KzgProof> compute_blob_kzg_proof(const Blob &blob, const KzgCommitment &c, const KzgSettings &s) {            // kzg.rs:1030
        KzgProof p;
        int rc = kzg355_compute_blob_kzg_proof(p.bytes.data(), blob.data(), c.data(), s.raw());
        if (rc) return from_status(rc, "compute_blob_kzg_proof");
        return p;
    }
    static Result<bool> verify_kzg_proof(const KzgCommitment &c, const Bytes32 &z, const Bytes32 &y, const KzgProof &p, const KzgSettings &s) {   // kzg.rs:1039
        bool ok = false;
        int rc = kzg355_verify_kzg_proof(&ok, c.data(), z.data(), y.data(), p.data(), s.raw());
        if (rc) return from_status(rc, "verify_kzg_proof");
        return ok;
    }
    static Result<bool> verify_blob_kzg_proof(const Blob &blob, const KzgCommitment &c, const KzgProof &p, const KzgSettings &s) {              // kzg.rs:1050
        bool ok = false;
        int rc = kzg355_verify_blob_kzg_proof(&ok, blob.data(), c.data(), p.data(), s.raw());
        if (rc) return from_status(rc, "verify_blob_kzg_proof");
        return ok;
    }
    static Result<bool> verify_blob_kzg_proof_batch(const std::vector<Blob> &blobs, const std::vector<KzgCommitment> &cs,
                                                    const std::vector<KzgProof> &ps, const KzgSettings &s) {                                    // kzg.rs:1066
        // `&[Blob]` is a slice of separately boxed blobs (kzg.rs:155-157): gather into one staging buffer
        std::vector<uint8_t> b(blobs.size() * BYTES_PER_BLOB), c(cs.size() * 48), p(ps.size() * 48);
        for (size_t i = 0; i < blobs.size(); i++) std::memcpy(&b[i * BYTES_PER_BLOB], blobs[i].data(), BYTES_PER_BLOB);
        for (size_t i = 0; i < cs.size(); i++) std::memcpy(&c[i * 48], cs[i].data(), 48);
        for (size_t i = 0; i < ps.size(); i++) std::memcpy(&p[i * 48], ps[i].data(), 48);
        bool ok = false;
        int rc = kzg355_verify_blob_kzg_proof_batch(&ok, b.data(), blobs.size(), c.data(), cs.size(), p.data(), ps.size(), s.raw());
        if (rc) return from_status(rc, "verify_blob_kzg_proof_batch");
        return ok;
    }

    // EIP-7594 verify_cell_kzg_proof_batch (consensus specs fulu/polynomial-commitments-sampling.md; no reference counterpart)
    static Result<bool> verify_cell_kzg_proof_batch(const std::vector<KzgCommitment> &cs, const std::vector<size_t> &cell_indices,
                                                    const std::vector<Cell> &cells, const std::vector<KzgProof> &ps, const KzgSettings &s) {
        const size_t n = cs.size();
        if (cell_indices.size() != n || cells.size() != n || ps.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> c(n * 48), cl(n * KZG355_BYTES_PER_CELL), p(n * 48);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&c[i * 48], cs[i].data(), 48);
            std::memcpy(&cl[i * KZG355_BYTES_PER_CELL], cells[i].data(), KZG355_BYTES_PER_CELL);
            std::memcpy(&p[i * 48], ps[i].data(), 48);
        }
        bool ok = false;
        int rc = kzg355_verify_cell_kzg_proof_batch(&ok, c.data(), cell_indices.data(), cl.data(), p.data(), n, s.raw());
        if (rc) return from_status(rc, "verify_cell_kzg_proof_batch");
        return ok;
    }

    // One independent verify_cell_kzg_proof_batch per group, the groups of any sizes (an empty one is true), all in one set of launches.  One
    // Result per group; a group whose four lengths differ is BadArgs for the call.
    struct CellGroup {
        std::vector<KzgCommitment> commitments;
        std::vector<size_t> cell_indices;
        std::vector<Cell> cells;
        std::vector<KzgProof> proofs;
    };
    static Result<std::vector<Result<bool>>> verify_cell_kzg_proof_batch_many_sets(const std::vector<CellGroup> &groups, const KzgSettings &s) {
        const size_t G = groups.size();
        std::vector<size_t> counts, indices;
        std::vector<uint8_t> c, cl, p;
        for (const CellGroup &g : groups) {
            const size_t n = g.commitments.size();
            if (g.cell_indices.size() != n || g.cells.size() != n || g.proofs.size() != n) return Error{Error::BadArgs, "length mismatch"};
            counts.push_back(n);
            indices.insert(indices.end(), g.cell_indices.begin(), g.cell_indices.end());
            for (size_t i = 0; i < n; i++) {
                c.insert(c.end(), g.commitments[i].data(), g.commitments[i].data() + 48);
                cl.insert(cl.end(), g.cells[i].data(), g.cells[i].data() + KZG355_BYTES_PER_CELL);
                p.insert(p.end(), g.proofs[i].data(), g.proofs[i].data() + 48);
            }
        }
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        indices.push_back(0);
        c.push_back(0); cl.push_back(0); p.push_back(0);
        std::unique_ptr<bool[]> ok(new bool[G + 1]());
        std::vector<int> st(G + 1, 0);
        int rc = kzg355_verify_cell_kzg_proof_batch_many_sets(ok.get(), st.data(), counts.data(), c.data(), indices.data(), cl.data(), p.data(), G, s.raw());
        st.resize(G);
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_cell_kzg_proof_batch_many_sets");
        std::vector<Result<bool>> out;
        for (size_t g = 0; g < G; g++) {
            if (st[g]) out.push_back(from_status(st[g], "verify_cell")); else out.push_back(bool(ok[g]));
        }
        return out;
    }

    // blobs against their EIP-7594 cell proofs (128 per blob, blob after blob in cell order): the Fulu counterpart of verify_blob_kzg_proof_batch,
    // exactly verify_cell_kzg_proof_batch over all 128 cells of every blob with the cells computed on the device
    static Result<bool> verify_blob_cell_proofs_batch(const std::vector<Blob> &blobs, const std::vector<KzgCommitment> &cs,
                                                      const std::vector<KzgProof> &cell_proofs, const KzgSettings &s) {
        std::vector<uint8_t> b(blobs.size() * BYTES_PER_BLOB), c(cs.size() * 48), p(cell_proofs.size() * 48);
        for (size_t i = 0; i < blobs.size(); i++) std::memcpy(&b[i * BYTES_PER_BLOB], blobs[i].data(), BYTES_PER_BLOB);
        for (size_t i = 0; i < cs.size(); i++) std::memcpy(&c[i * 48], cs[i].data(), 48);
        for (size_t i = 0; i < cell_proofs.size(); i++) std::memcpy(&p[i * 48], cell_proofs[i].data(), 48);
        bool ok = false;
        int rc = kzg355_verify_blob_cell_proofs_batch(&ok, b.data(), blobs.size(), c.data(), cs.size(), p.data(), cell_proofs.size(), s.raw());
        if (rc) return from_status(rc, "verify_blob_cell_proofs_batch");
        return ok;
    }

    // blob transactions of different blob counts in one call: one independent verify_blob_cell_proofs_batch per group, all non-empty groups in
    // one set of launches (an empty group is true); a group whose three lengths do not fit is BadArgs before the library is called
    struct BlobGroup {
        std::vector<Blob> blobs;
        std::vector<KzgCommitment> commitments;
        std::vector<KzgProof> cell_proofs;
    };
    static Result<std::vector<Result<bool>>> verify_blob_cell_proofs_batch_many_sets(const std::vector<BlobGroup> &groups, const KzgSettings &s) {
        const size_t G = groups.size();
        std::vector<size_t> counts;
        std::vector<uint8_t> b, c, p;
        for (const BlobGroup &g : groups) {
            const size_t n = g.blobs.size();
            if (g.commitments.size() != n || g.cell_proofs.size() != (size_t)KZG355_CELLS_PER_EXT_BLOB * n) return Error{Error::BadArgs, "length mismatch"};
            counts.push_back(n);
            for (size_t i = 0; i < n; i++) {
                b.insert(b.end(), g.blobs[i].data(), g.blobs[i].data() + BYTES_PER_BLOB);
                c.insert(c.end(), g.commitments[i].data(), g.commitments[i].data() + 48);
            }
            for (const KzgProof &x : g.cell_proofs) p.insert(p.end(), x.data(), x.data() + 48);
        }
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        b.push_back(0); c.push_back(0); p.push_back(0);
        std::unique_ptr<bool[]> ok(new bool[G + 1]());
        std::vector<int> st(G + 1, 0);
        int rc = kzg355_verify_blob_cell_proofs_batch_many_sets(ok.get(), st.data(), counts.data(), b.data(), c.data(), p.data(), G, s.raw());
        st.resize(G);
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_blob_cell_proofs_batch_many_sets");
        std::vector<Result<bool>> out;
        for (size_t g = 0; g < G; g++) {
            if (st[g]) out.push_back(from_status(st[g], "verify_blob_cells")); else out.push_back(bool(ok[g]));
        }
        return out;
    }

    // verify_blob_kzg_proof_batch on batches of different blob counts in one call: one independent check per group, each with its own challenge r
    // (an empty group is true); a group whose three lengths differ is BadArgs before the library is called (kzg.rs:644-651)
    struct ProofGroup {
        std::vector<Blob> blobs;
        std::vector<KzgCommitment> commitments;
        std::vector<KzgProof> proofs;
    };
    static Result<std::vector<Result<bool>>> verify_blob_kzg_proof_batch_many_sets(const std::vector<ProofGroup> &groups, const KzgSettings &s) {
        std::vector<size_t> counts;
        std::vector<uint8_t> b, c, p;
        for (const ProofGroup &g : groups) {
            const size_t n = g.blobs.size();
            if (g.commitments.size() != n || g.proofs.size() != n) return Error{Error::BadArgs, "length mismatch"};
            counts.push_back(n);
            for (size_t i = 0; i < n; i++) {
                b.insert(b.end(), g.blobs[i].data(), g.blobs[i].data() + BYTES_PER_BLOB);
                c.insert(c.end(), g.commitments[i].data(), g.commitments[i].data() + 48);
                p.insert(p.end(), g.proofs[i].data(), g.proofs[i].data() + 48);
            }
        }
        b.push_back(0); c.push_back(0); p.push_back(0);            // (data() of an empty vector may be null)
        return blob_sets_call(counts, b.data(), c.data(), p.data(), s, false);
    }
    // the same on device memory (the handle's first device): the three arrays batch after batch with no padding, blob_counts on the host
    static Result<std::vector<Result<bool>>> verify_blob_kzg_proof_batch_many_sets_device(const uint8_t *d_blobs, const uint8_t *d_commitments,
                                                                                         const uint8_t *d_proofs, const std::vector<size_t> &blob_counts,
                                                                                         const KzgSettings &s) {
        return blob_sets_call(blob_counts, d_blobs, d_commitments, d_proofs, s, true);
    }

    // EIP-7594 compute_cells_and_kzg_proofs: the 128 cells of the blob's 2x extension and their 128 proofs, in cell order
    static Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>> compute_cells_and_kzg_proofs(const Blob &blob, const KzgSettings &s) {
        std::vector<uint8_t> c((size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL), p((size_t)KZG355_CELLS_PER_EXT_BLOB * 48);
        int rc = kzg355_compute_cells_and_kzg_proofs(c.data(), p.data(), blob.data(), s.raw());
        if (rc) return from_status(rc, "compute_cells_and_kzg_proofs");
        std::pair<std::vector<Cell>, std::vector<KzgProof>> out;
        for (int k = 0; k < KZG355_CELLS_PER_EXT_BLOB; k++) {
            out.first.push_back(Cell::from_bytes(&c[(size_t)k * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
            out.second.push_back(KzgProof::from_bytes(&p[(size_t)k * 48], 48).value());
        }
        return out;
    }

    // EIP-7594 recover_cells_and_kzg_proofs: all 128 cells and proofs of a blob from 64..128 of its cells at strictly ascending indices
    static Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>> recover_cells_and_kzg_proofs(const std::vector<size_t> &cell_indices,
                                                                                                    const std::vector<Cell> &cells, const KzgSettings &s) {
        const size_t n = cells.size();
        if (cell_indices.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> in(n * KZG355_BYTES_PER_CELL), c((size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL),
            p((size_t)KZG355_CELLS_PER_EXT_BLOB * 48);
        for (size_t i = 0; i < n; i++) std::memcpy(&in[i * KZG355_BYTES_PER_CELL], cells[i].data(), KZG355_BYTES_PER_CELL);
        int rc = kzg355_recover_cells_and_kzg_proofs(c.data(), p.data(), cell_indices.data(), in.data(), n, s.raw());
        if (rc) return from_status(rc, "recover_cells_and_kzg_proofs");
        std::pair<std::vector<Cell>, std::vector<KzgProof>> out;
        for (int k = 0; k < KZG355_CELLS_PER_EXT_BLOB; k++) {
            out.first.push_back(Cell::from_bytes(&c[(size_t)k * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
            out.second.push_back(KzgProof::from_bytes(&p[(size_t)k * 48], 48).value());
        }
        return out;
    }

    // One independent recover_cells_and_kzg_proofs per unit (cell_indices, cells) in one set of launches: every blob brings its own index set.
    // One Result per unit; a unit whose two lengths differ is BadArgs for the call.
    using RecoverUnit = std::pair<std::vector<size_t>, std::vector<Cell>>;
    static Result<std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>>> recover_cells_and_kzg_proofs_many_sets(
        const std::vector<RecoverUnit> &units, const KzgSettings &s) {
        const size_t m = units.size();
        std::vector<size_t> counts, indices;
        std::vector<uint8_t> in;
        for (const RecoverUnit &u : units) {
            if (u.first.size() != u.second.size()) return Error{Error::BadArgs, "length mismatch"};
            counts.push_back(u.first.size());
            indices.insert(indices.end(), u.first.begin(), u.first.end());
            for (const Cell &c : u.second) in.insert(in.end(), c.data(), c.data() + KZG355_BYTES_PER_CELL);
        }
        const size_t per_cells = (size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL, per_proofs = (size_t)KZG355_CELLS_PER_EXT_BLOB * 48;
        std::vector<uint8_t> c(per_cells * (m + 1)), p(per_proofs * (m + 1));
        std::vector<int> st(m + 1, 0);
        indices.push_back(0);                                      // (data() of an empty vector may be null)
        in.push_back(0);
        int rc = kzg355_recover_cells_and_kzg_proofs_many_sets(c.data(), p.data(), st.data(), counts.data(), indices.data(), in.data(), m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_cells_and_kzg_proofs_many_sets");
        std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>> out;
        for (size_t i = 0; i < m; i++) {
            if (st[i]) { out.push_back(from_status(st[i], "recover_cells")); continue; }
            std::pair<std::vector<Cell>, std::vector<KzgProof>> r;
            for (int k = 0; k < KZG355_CELLS_PER_EXT_BLOB; k++) {
                r.first.push_back(Cell::from_bytes(&c[per_cells * i + (size_t)k * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
                r.second.push_back(KzgProof::from_bytes(&p[per_proofs * i + (size_t)k * 48], 48).value());
            }
            out.push_back(std::move(r));
        }
        return out;
    }

    // ---- the compute and recover calls with the blobs' commitments: the FK20 chain computes them on its way to the proofs (slot 63 of the
    // convolution whose other slots give the proofs), so no second call and no wide MSM table is needed
    struct CommitmentCellsProofs {
        KzgCommitment commitment;
        std::vector<Cell> cells;
        std::vector<KzgProof> proofs;
    };
    // per unit its status, or what the three host output buffers of a *_commitments_* call hold for it
    static std::vector<Result<CommitmentCellsProofs>> unpack_commitments_cells_proofs(const std::vector<int> &st, const std::vector<uint8_t> &k,
                                                                                     const std::vector<uint8_t> &c, const std::vector<uint8_t> &p,
                                                                                     const char *what) {
        const size_t per_cells = (size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL, per_proofs = (size_t)KZG355_CELLS_PER_EXT_BLOB * 48;
        std::vector<Result<CommitmentCellsProofs>> out;
        for (size_t i = 0; i < st.size(); i++) {
            if (st[i]) { out.push_back(from_status(st[i], what)); continue; }
            CommitmentCellsProofs r;
            r.commitment = KzgCommitment::from_bytes(&k[48 * i], 48).value();
            for (int j = 0; j < KZG355_CELLS_PER_EXT_BLOB; j++) {
                r.cells.push_back(Cell::from_bytes(&c[per_cells * i + (size_t)j * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
                r.proofs.push_back(KzgProof::from_bytes(&p[per_proofs * i + (size_t)j * 48], 48).value());
            }
            out.push_back(std::move(r));
        }
        return out;
    }
    static Result<std::vector<Result<CommitmentCellsProofs>>> compute_commitment_cells_and_kzg_proofs_many(const std::vector<Blob> &blobs,
                                                                                                           const KzgSettings &s) {
        const size_t n = blobs.size();
        std::vector<uint8_t> in((size_t)KZG355_BYTES_PER_BLOB * n + 1), k(48 * (n + 1)),
            c((size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL * (n + 1)), p((size_t)KZG355_CELLS_PER_EXT_BLOB * 48 * (n + 1));
        for (size_t i = 0; i < n; i++) std::memcpy(&in[(size_t)KZG355_BYTES_PER_BLOB * i], blobs[i].data(), KZG355_BYTES_PER_BLOB);
        std::vector<int> st(n + 1, 0);
        int rc = kzg355_compute_commitments_cells_and_kzg_proofs_many(k.data(), c.data(), p.data(), st.data(), in.data(), n, s.raw());
        st.resize(n);
        if (whole_call_failed(rc, st)) return from_status(rc, "compute_commitment_cells_and_kzg_proofs_many");
        return unpack_commitments_cells_proofs(st, k, c, p, "compute_cells");
    }
    static Result<CommitmentCellsProofs> compute_commitment_cells_and_kzg_proofs(const Blob &blob, const KzgSettings &s) {
        auto res = compute_commitment_cells_and_kzg_proofs_many(std::vector<Blob>{blob}, s);
        if (res.is_err()) return res.error();
        return std::move(res.value()[0]);
    }
    // m blobs known at the same cell_indices: cells holds blob after blob, cell_indices.size() cells each
    static Result<std::vector<Result<CommitmentCellsProofs>>> recover_commitment_cells_and_kzg_proofs_many(const std::vector<size_t> &cell_indices,
                                                                                                           const std::vector<Cell> &cells, size_t m,
                                                                                                           const KzgSettings &s) {
        const size_t n = cell_indices.size();
        if (cells.size() != n * m) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> in(cells.size() * KZG355_BYTES_PER_CELL + 1), k(48 * (m + 1)),
            c((size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL * (m + 1)), p((size_t)KZG355_CELLS_PER_EXT_BLOB * 48 * (m + 1));
        for (size_t i = 0; i < cells.size(); i++) std::memcpy(&in[i * KZG355_BYTES_PER_CELL], cells[i].data(), KZG355_BYTES_PER_CELL);
        std::vector<size_t> idx(cell_indices);
        idx.push_back(0);                                          // (data() of an empty vector may be null)
        std::vector<int> st(m + 1, 0);
        int rc = kzg355_recover_commitments_cells_and_kzg_proofs_many(k.data(), c.data(), p.data(), st.data(), idx.data(), in.data(), n, m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_commitment_cells_and_kzg_proofs_many");
        return unpack_commitments_cells_proofs(st, k, c, p, "recover_cells");
    }
    static Result<CommitmentCellsProofs> recover_commitment_cells_and_kzg_proofs(const std::vector<size_t> &cell_indices, const std::vector<Cell> &cells,
                                                                                 const KzgSettings &s) {
        if (cell_indices.size() != cells.size()) return Error{Error::BadArgs, "length mismatch"};
        auto res = recover_commitment_cells_and_kzg_proofs_many(cell_indices, cells, 1, s);
        if (res.is_err()) return res.error();
        return std::move(res.value()[0]);
    }
    static Result<std::vector<Result<CommitmentCellsProofs>>> recover_commitment_cells_and_kzg_proofs_many_sets(const std::vector<RecoverUnit> &units,
                                                                                                                const KzgSettings &s) {
        const size_t m = units.size();
        std::vector<size_t> counts, indices;
        std::vector<uint8_t> in;
        for (const RecoverUnit &u : units) {
            if (u.first.size() != u.second.size()) return Error{Error::BadArgs, "length mismatch"};
            counts.push_back(u.first.size());
            indices.insert(indices.end(), u.first.begin(), u.first.end());
            for (const Cell &c : u.second) in.insert(in.end(), c.data(), c.data() + KZG355_BYTES_PER_CELL);
        }
        std::vector<uint8_t> k(48 * (m + 1)), c((size_t)KZG355_CELLS_PER_EXT_BLOB * KZG355_BYTES_PER_CELL * (m + 1)),
            p((size_t)KZG355_CELLS_PER_EXT_BLOB * 48 * (m + 1));
        std::vector<int> st(m + 1, 0);
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        indices.push_back(0);
        in.push_back(0);
        int rc = kzg355_recover_commitments_cells_and_kzg_proofs_many_sets(k.data(), c.data(), p.data(), st.data(), counts.data(), indices.data(),
                                                                           in.data(), m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_commitment_cells_and_kzg_proofs_many_sets");
        return unpack_commitments_cells_proofs(st, k, c, p, "recover_cells");
    }

    // The cells of a blob at chosen indices (each < 128, any order, repeats allowed) and their proofs, entry j what compute_cells_and_kzg_proofs
    // returns at cell_indices[j]: every index through its own quotient and one MSM instead of the FK20 chain
    static Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>> compute_cell_kzg_proofs_at(const Blob &blob, const std::vector<size_t> &cell_indices,
                                                                                                  const KzgSettings &s) {
        const size_t k = cell_indices.size();
        std::vector<uint8_t> c((k + 1) * KZG355_BYTES_PER_CELL), p((k + 1) * 48);
        std::vector<size_t> indices(cell_indices);
        indices.push_back(0);                                      // (data() of an empty vector may be null)
        int rc = kzg355_compute_cell_kzg_proofs_at(c.data(), p.data(), blob.data(), indices.data(), k, s.raw());
        if (rc) return from_status(rc, "compute_cell_kzg_proofs_at");
        std::pair<std::vector<Cell>, std::vector<KzgProof>> out;
        for (size_t j = 0; j < k; j++) {
            out.first.push_back(Cell::from_bytes(&c[j * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
            out.second.push_back(KzgProof::from_bytes(&p[j * 48], 48).value());
        }
        return out;
    }

    // One independent compute_cell_kzg_proofs_at per blob, each with its own index list (which may be empty), in one set of launches.  One Result
    // per blob; blobs and index_lists of different lengths are BadArgs for the call.
    static Result<std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>>> compute_cell_kzg_proofs_at_many(
        const std::vector<Blob> &blobs, const std::vector<std::vector<size_t>> &index_lists, const KzgSettings &s) {
        const size_t n = blobs.size();
        if (index_lists.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<size_t> counts, indices;
        std::vector<uint8_t> in(n * BYTES_PER_BLOB + 1);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&in[i * BYTES_PER_BLOB], blobs[i].data(), BYTES_PER_BLOB);
            counts.push_back(index_lists[i].size());
            indices.insert(indices.end(), index_lists[i].begin(), index_lists[i].end());
        }
        const size_t total = indices.size();
        std::vector<uint8_t> c((total + 1) * KZG355_BYTES_PER_CELL), p((total + 1) * 48);
        std::vector<int> st(n + 1, 0);
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        indices.push_back(0);
        int rc = kzg355_compute_cell_kzg_proofs_at_many(c.data(), p.data(), st.data(), in.data(), n, counts.data(), indices.data(), s.raw());
        st.resize(n);
        if (whole_call_failed(rc, st)) return from_status(rc, "compute_cell_kzg_proofs_at_many");
        std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>> out;
        size_t off = 0;
        for (size_t i = 0; i < n; off += counts[i], i++) {
            if (st[i]) { out.push_back(from_status(st[i], "compute_cell_kzg_proofs_at")); continue; }
            std::pair<std::vector<Cell>, std::vector<KzgProof>> r;
            for (size_t j = off; j < off + counts[i]; j++) {
                r.first.push_back(Cell::from_bytes(&c[j * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
                r.second.push_back(KzgProof::from_bytes(&p[j * 48], 48).value());
            }
            out.push_back(std::move(r));
        }
        return out;
    }

    // The cells of the recovered blob at want_indices (each < 128, any order, repeats allowed) and their proofs, entry j what
    // recover_cells_and_kzg_proofs returns at want_indices[j] for the same input: every wanted index through its own quotient and one MSM
    static Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>> recover_cells_and_kzg_proofs_at(const std::vector<size_t> &cell_indices,
                                                                                                       const std::vector<Cell> &cells,
                                                                                                       const std::vector<size_t> &want_indices,
                                                                                                       const KzgSettings &s) {
        const size_t n = cell_indices.size(), k = want_indices.size();
        if (cells.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> in(n * KZG355_BYTES_PER_CELL + 1), c((k + 1) * KZG355_BYTES_PER_CELL), p((k + 1) * 48);
        for (size_t i = 0; i < n; i++) std::memcpy(&in[i * KZG355_BYTES_PER_CELL], cells[i].data(), KZG355_BYTES_PER_CELL);
        std::vector<size_t> known(cell_indices), want(want_indices);
        known.push_back(0);                                        // (data() of an empty vector may be null)
        want.push_back(0);
        int rc = kzg355_recover_cells_and_kzg_proofs_at(c.data(), p.data(), known.data(), in.data(), n, want.data(), k, s.raw());
        if (rc) return from_status(rc, "recover_cells_and_kzg_proofs_at");
        std::pair<std::vector<Cell>, std::vector<KzgProof>> out;
        for (size_t j = 0; j < k; j++) {
            out.first.push_back(Cell::from_bytes(&c[j * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
            out.second.push_back(KzgProof::from_bytes(&p[j * 48], 48).value());
        }
        return out;
    }

    // One independent recover_cells_and_kzg_proofs_at per unit (cell_indices, cells, want_indices) in one set of launches (want_indices may be
    // empty: the blob is still recovered and checked).  One Result per unit; a unit whose first two lengths differ is BadArgs for the call.
    struct RecoverAtUnit { std::vector<size_t> cell_indices; std::vector<Cell> cells; std::vector<size_t> want_indices; };
    static Result<std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>>> recover_cells_and_kzg_proofs_at_many_sets(
        const std::vector<RecoverAtUnit> &units, const KzgSettings &s) {
        const size_t m = units.size();
        std::vector<size_t> counts, indices, want_counts, want;
        std::vector<uint8_t> in;
        for (const RecoverAtUnit &u : units) {
            if (u.cell_indices.size() != u.cells.size()) return Error{Error::BadArgs, "length mismatch"};
            counts.push_back(u.cell_indices.size());
            indices.insert(indices.end(), u.cell_indices.begin(), u.cell_indices.end());
            for (const Cell &x : u.cells) in.insert(in.end(), x.data(), x.data() + KZG355_BYTES_PER_CELL);
            want_counts.push_back(u.want_indices.size());
            want.insert(want.end(), u.want_indices.begin(), u.want_indices.end());
        }
        const size_t total = want.size();
        std::vector<uint8_t> c((total + 1) * KZG355_BYTES_PER_CELL), p((total + 1) * 48);
        std::vector<int> st(m + 1, 0);
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        indices.push_back(0);
        in.push_back(0);
        want_counts.push_back(0);
        want.push_back(0);
        int rc = kzg355_recover_cells_and_kzg_proofs_at_many_sets(c.data(), p.data(), st.data(), counts.data(), indices.data(), in.data(),
                                                                  want_counts.data(), want.data(), m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_cells_and_kzg_proofs_at_many_sets");
        std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>> out;
        size_t off = 0;
        for (size_t i = 0; i < m; off += want_counts[i], i++) {
            if (st[i]) { out.push_back(from_status(st[i], "recover_cells_and_kzg_proofs_at")); continue; }
            std::pair<std::vector<Cell>, std::vector<KzgProof>> r;
            for (size_t j = off; j < off + want_counts[i]; j++) {
                r.first.push_back(Cell::from_bytes(&c[j * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
                r.second.push_back(KzgProof::from_bytes(&p[j * 48], 48).value());
            }
            out.push_back(std::move(r));
        }
        return out;
    }

    // ---- the three cell calls on device-resident data (kzg355.h: pointer and alignment rules).  The d_* arguments are device pointers on the
    // handle's device; one Result per unit, an Err of the call itself only for whole-call failures (whole_call_failed, below).
    static Result<std::vector<Result<bool>>> verify_cell_kzg_proof_batch_many_device(const uint8_t *d_commitments, const size_t *d_cell_indices,
                                                                                     const uint8_t *d_cells, const uint8_t *d_proofs, size_t n_per_group,
                                                                                     size_t groups, const KzgSettings &s) {
        std::unique_ptr<bool[]> ok(new bool[groups + 1]());
        std::vector<int> st(groups + 1, 0);
        int rc = kzg355_verify_cell_kzg_proof_batch_many_device(ok.get(), st.data(), d_commitments, d_cell_indices, d_cells, d_proofs, n_per_group, groups,
                                                                s.raw());
        st.resize(groups);
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_cell_kzg_proof_batch_many_device");
        std::vector<Result<bool>> out;
        for (size_t g = 0; g < groups; g++) {
            if (st[g]) out.push_back(from_status(st[g], "verify_cell")); else out.push_back(bool(ok[g]));
        }
        return out;
    }
    // groups of different sizes: group g is cell_counts[g] entries of the four device arrays, group after group; the counts are host memory
    static Result<std::vector<Result<bool>>> verify_cell_kzg_proof_batch_many_sets_device(const std::vector<size_t> &cell_counts, const uint8_t *d_commitments,
                                                                                          const size_t *d_cell_indices, const uint8_t *d_cells,
                                                                                          const uint8_t *d_proofs, const KzgSettings &s) {
        const size_t groups = cell_counts.size();
        std::unique_ptr<bool[]> ok(new bool[groups + 1]());
        std::vector<int> st(groups + 1, 0);
        int rc = kzg355_verify_cell_kzg_proof_batch_many_sets_device(ok.get(), st.data(), cell_counts.data(), d_commitments, d_cell_indices, d_cells, d_proofs,
                                                                     groups, s.raw());
        st.resize(groups);
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_cell_kzg_proof_batch_many_sets_device");
        std::vector<Result<bool>> out;
        for (size_t g = 0; g < groups; g++) {
            if (st[g]) out.push_back(from_status(st[g], "verify_cell")); else out.push_back(bool(ok[g]));
        }
        return out;
    }
    // statuses per blob (KZG355_OK or that blob's error); cells and proofs land in the caller's device buffers (either may be null, not both)
    static Result<std::vector<int>> compute_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out, const uint8_t *d_blobs, size_t n,
                                                                             const KzgSettings &s) {
        std::vector<int> st(n + 1, 0);
        int rc = kzg355_compute_cells_and_kzg_proofs_many_device(d_cells_out, d_proofs_out, st.data(), d_blobs, n, s.raw());
        st.resize(n);
        if (whole_call_failed(rc, st)) return from_status(rc, "compute_cells_and_kzg_proofs_many_device");
        return st;
    }
    static Result<std::vector<int>> recover_cells_and_kzg_proofs_many_device(uint8_t *d_cells_out, uint8_t *d_proofs_out,
                                                                             const std::vector<size_t> &cell_indices, const uint8_t *d_cells, size_t m,
                                                                             const KzgSettings &s) {
        std::vector<int> st(m + 1, 0);
        int rc = kzg355_recover_cells_and_kzg_proofs_many_device(d_cells_out, d_proofs_out, st.data(), cell_indices.data(), d_cells, cell_indices.size(), m,
                                                                 s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_cells_and_kzg_proofs_many_device");
        return st;
    }

    // blob i known at cell_counts[i] cells: its indices (host) and its cells (device) follow those of blob i - 1
    static Result<std::vector<int>> recover_cells_and_kzg_proofs_many_sets_device(uint8_t *d_cells_out, uint8_t *d_proofs_out,
                                                                                  const std::vector<size_t> &cell_counts,
                                                                                  const std::vector<size_t> &cell_indices, const uint8_t *d_cells,
                                                                                  const KzgSettings &s) {
        const size_t m = cell_counts.size();
        size_t total = 0;
        for (size_t c : cell_counts) {
            if (c > cell_indices.size() - total) return Error{Error::BadArgs, "length mismatch"};
            total += c;
        }
        if (total != cell_indices.size()) return Error{Error::BadArgs, "length mismatch"};
        std::vector<int> st(m + 1, 0);
        int rc = kzg355_recover_cells_and_kzg_proofs_many_sets_device(d_cells_out, d_proofs_out, st.data(), cell_counts.data(), cell_indices.data(), d_cells,
                                                                      m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_cells_and_kzg_proofs_many_sets_device");
        return st;
    }

    // the three calls above with the blobs' commitments (48 bytes per blob) written to d_commitments_out as well; any of the three outputs may be
    // null, not all
    static Result<std::vector<int>> compute_commitment_cells_and_kzg_proofs_many_device(uint8_t *d_commitments_out, uint8_t *d_cells_out,
                                                                                        uint8_t *d_proofs_out, const uint8_t *d_blobs, size_t n,
                                                                                        const KzgSettings &s) {
        std::vector<int> st(n + 1, 0);
        int rc = kzg355_compute_commitments_cells_and_kzg_proofs_many_device(d_commitments_out, d_cells_out, d_proofs_out, st.data(), d_blobs, n, s.raw());
        st.resize(n);
        if (whole_call_failed(rc, st)) return from_status(rc, "compute_commitment_cells_and_kzg_proofs_many_device");
        return st;
    }
    static Result<std::vector<int>> recover_commitment_cells_and_kzg_proofs_many_device(uint8_t *d_commitments_out, uint8_t *d_cells_out,
                                                                                        uint8_t *d_proofs_out, const std::vector<size_t> &cell_indices,
                                                                                        const uint8_t *d_cells, size_t m, const KzgSettings &s) {
        std::vector<int> st(m + 1, 0);
        int rc = kzg355_recover_commitments_cells_and_kzg_proofs_many_device(d_commitments_out, d_cells_out, d_proofs_out, st.data(), cell_indices.data(),
                                                                             d_cells, cell_indices.size(), m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_commitment_cells_and_kzg_proofs_many_device");
        return st;
    }
    static Result<std::vector<int>> recover_commitment_cells_and_kzg_proofs_many_sets_device(uint8_t *d_commitments_out, uint8_t *d_cells_out,
                                                                                             uint8_t *d_proofs_out, const std::vector<size_t> &cell_counts,
                                                                                             const std::vector<size_t> &cell_indices,
                                                                                             const uint8_t *d_cells, const KzgSettings &s) {
        const size_t m = cell_counts.size();
        size_t total = 0;
        for (size_t c : cell_counts) {
            if (c > cell_indices.size() - total) return Error{Error::BadArgs, "length mismatch"};
            total += c;
        }
        if (total != cell_indices.size()) return Error{Error::BadArgs, "length mismatch"};
        std::vector<int> st(m + 1, 0);
        int rc = kzg355_recover_commitments_cells_and_kzg_proofs_many_sets_device(d_commitments_out, d_cells_out, d_proofs_out, st.data(),
                                                                                  cell_counts.data(), cell_indices.data(), d_cells, m, s.raw());
        st.resize(m);
        if (whole_call_failed(rc, st)) return from_status(rc, "recover_commitment_cells_and_kzg_proofs_many_sets_device");
        return st;
    }

    // ---- throughput extensions (no reference counterpart): many independent single-proof units per call; one Result per unit, an Err of the
    // call itself only for whole-call failures (no device, out of memory, a length mismatch)
    static bool whole_call_failed(int rc, const std::vector<int> &st) {
        if (rc == KZG355_INTERNAL || rc == KZG355_NO_DEVICE || rc == KZG355_NO_MEMORY || rc == KZG355_DEVICE_ERROR) return true;
        if (rc == KZG355_OK) return false;
        for (int x : st) if (x) return false;
        return true;
    }
    // what the two verify_blob_kzg_proof_batch_many_sets forms share: the call and its per-group results
    static Result<std::vector<Result<bool>>> blob_sets_call(const std::vector<size_t> &blob_counts, const uint8_t *blobs, const uint8_t *commitments,
                                                           const uint8_t *proofs, const KzgSettings &s, bool device) {
        const size_t G = blob_counts.size();
        std::vector<size_t> counts(blob_counts);
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        std::unique_ptr<bool[]> ok(new bool[G + 1]());
        std::vector<int> st(G + 1, 0);
        int rc = device ? kzg355_verify_blob_kzg_proof_batch_many_sets_device(ok.get(), st.data(), counts.data(), blobs, commitments, proofs, G, s.raw())
                        : kzg355_verify_blob_kzg_proof_batch_many_sets(ok.get(), st.data(), counts.data(), blobs, commitments, proofs, G, s.raw());
        st.resize(G);
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_blob_kzg_proof_batch_many_sets");
        std::vector<Result<bool>> out;
        for (size_t g = 0; g < G; g++) {
            if (st[g]) out.push_back(from_status(st[g], "verify")); else out.push_back(bool(ok[g]));
        }
        return out;
    }
    static Result<std::vector<Result<bool>>> verify_kzg_proof_many(const std::vector<KzgCommitment> &cs, const std::vector<Bytes32> &zs,
                                                                   const std::vector<Bytes32> &ys, const std::vector<KzgProof> &ps, const KzgSettings &s) {
        const size_t n = cs.size();
        if (zs.size() != n || ys.size() != n || ps.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> c(n * 48 + 1), z(n * 32 + 1), y(n * 32 + 1), p(n * 48 + 1);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&c[i * 48], cs[i].data(), 48); std::memcpy(&z[i * 32], zs[i].data(), 32);
            std::memcpy(&y[i * 32], ys[i].data(), 32); std::memcpy(&p[i * 48], ps[i].data(), 48);
        }
        std::unique_ptr<bool[]> ok(new bool[n + 1]());
        std::vector<int> st(n, 0);
        int rc = kzg355_verify_kzg_proof_many(ok.get(), st.data(), c.data(), z.data(), y.data(), p.data(), n, s.raw());
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_kzg_proof_many");
        std::vector<Result<bool>> out;
        for (size_t i = 0; i < n; i++) { if (st[i]) out.emplace_back(from_status(st[i], "verify")); else out.emplace_back(ok[i]); }
        return out;
    }
    static Result<std::vector<Result<bool>>> verify_blob_kzg_proof_many(const std::vector<Blob> &blobs, const std::vector<KzgCommitment> &cs,
                                                                        const std::vector<KzgProof> &ps, const KzgSettings &s) {
        const size_t n = blobs.size();
        if (cs.size() != n || ps.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> b(n * BYTES_PER_BLOB + 1), c(n * 48 + 1), p(n * 48 + 1);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&b[i * BYTES_PER_BLOB], blobs[i].data(), BYTES_PER_BLOB); std::memcpy(&c[i * 48], cs[i].data(), 48);
            std::memcpy(&p[i * 48], ps[i].data(), 48);
        }
        std::unique_ptr<bool[]> ok(new bool[n + 1]());
        std::vector<int> st(n, 0);
        int rc = kzg355_verify_blob_kzg_proof_many(ok.get(), st.data(), b.data(), c.data(), p.data(), n, s.raw());
        if (whole_call_failed(rc, st)) return from_status(rc, "verify_blob_kzg_proof_many");
        std::vector<Result<bool>> out;
        for (size_t i = 0; i < n; i++) { if (st[i]) out.emplace_back(from_status(st[i], "verify")); else out.emplace_back(ok[i]); }
        return out;
    }
    static Result<std::vector<Result<std::pair<KzgProof, Bytes32>>>> compute_kzg_proof_many(const std::vector<Blob> &blobs, const std::vector<Bytes32> &zs,
                                                                                           const KzgSettings &s) {
        const size_t n = blobs.size();
        if (zs.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<uint8_t> b(n * BYTES_PER_BLOB + 1), z(n * 32 + 1), pr(n * 48 + 1), ys(n * 32 + 1);
        for (size_t i = 0; i < n; i++) { std::memcpy(&b[i * BYTES_PER_BLOB], blobs[i].data(), BYTES_PER_BLOB); std::memcpy(&z[i * 32], zs[i].data(), 32); }
        std::vector<int> st(n, 0);
        int rc = kzg355_compute_kzg_proof_many(pr.data(), ys.data(), st.data(), b.data(), z.data(), n, s.raw());
        if (whole_call_failed(rc, st)) return from_status(rc, "compute_kzg_proof_many");
        std::vector<Result<std::pair<KzgProof, Bytes32>>> out;
        for (size_t i = 0; i < n; i++) {
            if (st[i]) { out.emplace_back(from_status(st[i], "proof")); continue; }
            KzgProof p; Bytes32 y;
            std::memcpy(p.bytes.data(), &pr[i * 48], 48); std::memcpy(y.bytes.data(), &ys[i * 32], 32);
            out.emplace_back(std::make_pair(p, y));
        }
        return out;
    }

    // The blob opened at the points zs (any order, repeats allowed, inside the domain or not; at most 4096): entry j is what compute_kzg_proof returns
    // for (blob, zs[j]), every point through its own quotient and one MSM, and the blob is handed over once
    static Result<std::pair<std::vector<KzgProof>, std::vector<Bytes32>>> compute_kzg_proofs_at(const Blob &blob, const std::vector<Bytes32> &zs,
                                                                                                const KzgSettings &s) {
        const size_t k = zs.size();
        std::vector<uint8_t> z(k * 32 + 1), pr(k * 48 + 1), ys(k * 32 + 1);      // (data() of an empty vector may be null)
        for (size_t j = 0; j < k; j++) std::memcpy(&z[j * 32], zs[j].data(), 32);
        int rc = kzg355_compute_kzg_proofs_at(pr.data(), ys.data(), blob.data(), z.data(), k, s.raw());
        if (rc) return from_status(rc, "compute_kzg_proofs_at");
        std::pair<std::vector<KzgProof>, std::vector<Bytes32>> out;
        for (size_t j = 0; j < k; j++) {
            KzgProof p; Bytes32 y;
            std::memcpy(p.bytes.data(), &pr[j * 48], 48); std::memcpy(y.bytes.data(), &ys[j * 32], 32);
            out.first.push_back(p); out.second.push_back(y);
        }
        return out;
    }

    // One independent compute_kzg_proofs_at per blob, each with its own list of points (which may be empty), in one set of launches.  One Result per
    // blob; blobs and point_lists of different lengths are BadArgs for the call.
    static Result<std::vector<Result<std::pair<std::vector<KzgProof>, std::vector<Bytes32>>>>> compute_kzg_proofs_at_many(
        const std::vector<Blob> &blobs, const std::vector<std::vector<Bytes32>> &point_lists, const KzgSettings &s) {
        const size_t n = blobs.size();
        if (point_lists.size() != n) return Error{Error::BadArgs, "length mismatch"};
        std::vector<size_t> counts;
        std::vector<uint8_t> in(n * BYTES_PER_BLOB + 1), z;
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&in[i * BYTES_PER_BLOB], blobs[i].data(), BYTES_PER_BLOB);
            counts.push_back(point_lists[i].size());
            for (const Bytes32 &x : point_lists[i]) z.insert(z.end(), x.data(), x.data() + 32);
        }
        const size_t total = z.size() / 32;
        std::vector<uint8_t> pr((total + 1) * 48), ys((total + 1) * 32);
        std::vector<int> st(n + 1, 0);
        counts.push_back(0);                                       // (data() of an empty vector may be null)
        z.push_back(0);
        int rc = kzg355_compute_kzg_proofs_at_many(pr.data(), ys.data(), st.data(), in.data(), n, counts.data(), z.data(), s.raw());
        st.resize(n);
        if (whole_call_failed(rc, st)) return from_status(rc, "compute_kzg_proofs_at_many");
        std::vector<Result<std::pair<std::vector<KzgProof>, std::vector<Bytes32>>>> out;
        size_t off = 0;
        for (size_t i = 0; i < n; off += counts[i], i++) {
            if (st[i]) { out.push_back(from_status(st[i], "compute_kzg_proofs_at")); continue; }
            std::pair<std::vector<KzgProof>, std::vector<Bytes32>> r;
            for (size_t j = off; j < off + counts[i]; j++) {
                KzgProof p; Bytes32 y;
                std::memcpy(p.bytes.data(), &pr[j * 48], 48); std::memcpy(y.bytes.data(), &ys[j * 32], 32);
                r.first.push_back(p); r.second.push_back(y);
            }
            out.push_back(std::move(r));
        }
        return out;
    }

    // ---- the EIP-4844 point-evaluation precompile (address 0x0A): an input is versioned_hash (32) | z (32) | y (32) | commitment (48) | proof (48)
    using PointEvaluationInput = FixedBytes<KZG355_BYTES_PER_POINT_EVALUATION_INPUT, Error::BadArgs>;
    // per input: what verify_kzg_proof_many gives for its four fields, and whether its versioned hash is that of its commitment.  No match: false,
    // and nothing else about the input is reported (the precompile fails at the hash before it looks at the rest)
    struct PointEvaluation { Result<bool> result; bool hash_match; };
    // 0x01 || sha256(commitment)[1:] per commitment, on the host: no handle, no device, nothing validated
    static Result<std::vector<Bytes32>> kzg_to_versioned_hash_many(const std::vector<KzgCommitment> &cs) {
        const size_t n = cs.size();
        std::vector<uint8_t> c(n * 48 + 1), h(n * 32 + 1);
        for (size_t i = 0; i < n; i++) std::memcpy(&c[i * 48], cs[i].data(), 48);
        int rc = kzg355_kzg_to_versioned_hash_many(h.data(), c.data(), n);
        if (rc) return from_status(rc, "kzg_to_versioned_hash_many");
        std::vector<Bytes32> out(n);
        for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &h[i * 32], 32);
        return out;
    }
    static Result<Bytes32> kzg_to_versioned_hash(const KzgCommitment &c) {
        auto r = kzg_to_versioned_hash_many({c});
        if (r.is_err()) return r.error();
        return r.value()[0];
    }
    // d_commitments (n * 48 bytes, 4-byte aligned) -> d_out (n * 32 bytes, 16-byte aligned), device memory on the handle's first device
    static Result<bool> kzg_to_versioned_hash_many_device(uint8_t *d_out, const uint8_t *d_commitments, size_t n, const KzgSettings &s) {
        int rc = kzg355_kzg_to_versioned_hash_many_device(d_out, d_commitments, n, s.raw());
        if (rc) return from_status(rc, "kzg_to_versioned_hash_many_device");
        return true;
    }
    // what the two point_evaluation_many forms share: the call and its per-input results
    static Result<std::vector<PointEvaluation>> point_evaluation_call(const uint8_t *inputs, size_t n, const KzgSettings &s, bool device) {
        std::unique_ptr<bool[]> ok(new bool[n + 1]()), match(new bool[n + 1]());
        std::vector<int> st(n, 0);
        int rc = device ? kzg355_point_evaluation_many_device(ok.get(), st.data(), match.get(), inputs, n, s.raw())
                        : kzg355_point_evaluation_many(ok.get(), st.data(), match.get(), inputs, n, s.raw());
        if (whole_call_failed(rc, st)) return from_status(rc, "point_evaluation_many");
        std::vector<PointEvaluation> out;
        for (size_t i = 0; i < n; i++) {
            if (st[i]) out.push_back(PointEvaluation{from_status(st[i], "point_evaluation"), match[i]});
            else out.push_back(PointEvaluation{bool(ok[i]), match[i]});
        }
        return out;
    }
    static Result<std::vector<PointEvaluation>> point_evaluation_many(const std::vector<PointEvaluationInput> &inputs, const KzgSettings &s) {
        const size_t n = inputs.size();
        std::vector<uint8_t> in(n * KZG355_BYTES_PER_POINT_EVALUATION_INPUT + 1);
        for (size_t i = 0; i < n; i++) std::memcpy(&in[i * KZG355_BYTES_PER_POINT_EVALUATION_INPUT], inputs[i].data(), KZG355_BYTES_PER_POINT_EVALUATION_INPUT);
        return point_evaluation_call(in.data(), n, s, false);
    }
    // d_inputs: n * 192 bytes of device memory on the handle's first device, 16-byte aligned, only read
    static Result<std::vector<PointEvaluation>> point_evaluation_many_device(const uint8_t *d_inputs, size_t n, const KzgSettings &s) {
        return point_evaluation_call(d_inputs, n, s, true);
    }
    // one precompile call as the EIP words it: u256be(FIELD_ELEMENTS_PER_BLOB) | u256be(BLS_MODULUS) on success; BadArgs on a length other than 192,
    // a hash mismatch, an invalid input or a false proof
    static Result<std::vector<uint8_t>> point_evaluation(const uint8_t *input, size_t input_len, const KzgSettings &s) {
        std::vector<uint8_t> out(64);
        int rc = kzg355_point_evaluation(out.data(), input, input_len, s.raw());
        if (rc) return from_status(rc, "point_evaluation");
        return out;
    }
    static Result<std::vector<uint8_t>> point_evaluation(const std::vector<uint8_t> &input, const KzgSettings &s) {
        return point_evaluation(input.data(), input.size(), s);
    }
};

}  // namespace kzg355
