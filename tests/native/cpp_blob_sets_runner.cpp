// cpp_blob_sets_runner -- drives Kzg::verify_blob_kzg_proof_batch_many_sets of the C++ mirror (include/kzg355.hpp) for tests/test_gpu_blob_sets.py.
//   usage: cpp_blob_sets_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <groups.bin>
//   groups.bin: per group u32le n, then n blobs (131072 each), n commitments (48 each), n proofs (48 each); ALL groups go into one call
//   prints one line per group: "true" | "false" | "err <kind>"; then "mismatch <kind>" for a group whose three lengths differ
#include <fstream>
#include <iostream>
#include <iterator>
#include "../../include/kzg355.hpp"

using namespace kzg355;

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc < 4) { std::cerr << "usage: cpp_blob_sets_runner <g1.bin> <g2.bin> <groups.bin>\n"; return 2; }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), in = slurp(argv[3]);
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    std::vector<Kzg::ProofGroup> groups;
    size_t at = 0;
    while (at + 4 <= in.size()) {
        uint32_t n = 0;
        for (int i = 0; i < 4; i++) n |= (uint32_t)in[at + i] << (8 * i);
        at += 4;
        if (at + (size_t)n * (BYTES_PER_BLOB + 96) > in.size()) { std::cerr << "truncated input\n"; return 2; }
        Kzg::ProofGroup g;
        for (uint32_t b = 0; b < n; b++, at += BYTES_PER_BLOB) g.blobs.push_back(Blob::from_bytes(&in[at], BYTES_PER_BLOB).value());
        for (uint32_t b = 0; b < n; b++, at += 48) g.commitments.push_back(KzgCommitment::from_bytes(&in[at], 48).value());
        for (uint32_t b = 0; b < n; b++, at += 48) g.proofs.push_back(KzgProof::from_bytes(&in[at], 48).value());
        groups.push_back(g);
    }
    auto v = Kzg::verify_blob_kzg_proof_batch_many_sets(groups, s);
    if (v.is_err()) { std::cout << "call err " << v.error().kind << "\n"; return 0; }
    for (const auto &r : v.value()) {
        if (r.is_err()) std::cout << "err " << r.error().kind << "\n";
        else std::cout << (r.value() ? "true" : "false") << "\n";
    }
    // the mirror's own argument check: a group whose three lengths differ never reaches the library
    for (size_t g = groups.size(); g-- > 0;) {
        if (groups[g].proofs.empty()) continue;
        groups[g].proofs.pop_back();
        auto w = Kzg::verify_blob_kzg_proof_batch_many_sets(groups, s);
        std::cout << "mismatch " << (w.is_err() ? (int)w.error().kind : -1) << "\n";
        break;
    }
    return 0;
}
