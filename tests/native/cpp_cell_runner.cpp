// cpp_cell_runner -- drives Kzg::verify_cell_kzg_proof_batch of the C++ mirror (include/kzg355.hpp) for tests/test_gpu_cells.py.
//   usage: cpp_cell_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <batches.bin>
//   batches.bin: per batch u32le n, then n records of commitment (48) | u64le cell index | cell (2048) | proof (48)
//   prints one line per batch: "true" | "false" | "err <kind>"
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
    if (argc < 4) { std::cerr << "usage: cpp_cell_runner <g1.bin> <g2.bin> <batches.bin>\n"; return 2; }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), in = slurp(argv[3]);
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    size_t at = 0;
    const size_t rec = 48 + 8 + KZG355_BYTES_PER_CELL + 48;
    while (at + 4 <= in.size()) {
        uint32_t n = 0;
        for (int i = 0; i < 4; i++) n |= (uint32_t)in[at + i] << (8 * i);
        at += 4;
        if (at + (size_t)n * rec > in.size()) { std::cerr << "truncated input\n"; return 2; }
        std::vector<KzgCommitment> cs; std::vector<size_t> idx; std::vector<Cell> cells; std::vector<KzgProof> ps;
        for (uint32_t k = 0; k < n; k++, at += rec) {
            const uint8_t *r = &in[at];
            cs.push_back(KzgCommitment::from_bytes(r, 48).value());
            uint64_t ix = 0;
            for (int i = 0; i < 8; i++) ix |= (uint64_t)r[48 + i] << (8 * i);
            idx.push_back((size_t)ix);
            cells.push_back(Cell::from_bytes(r + 56, KZG355_BYTES_PER_CELL).value());
            ps.push_back(KzgProof::from_bytes(r + 56 + KZG355_BYTES_PER_CELL, 48).value());
        }
        auto v = Kzg::verify_cell_kzg_proof_batch(cs, idx, cells, ps, s);
        if (v.is_err()) std::cout << "err " << v.error().kind << "\n";
        else std::cout << (v.value() ? "true" : "false") << "\n";
    }
    return 0;
}
